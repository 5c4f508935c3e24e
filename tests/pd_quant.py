"""What tests/test_pd_quant_host.py (CPU) and tests/test_gpu_pd_quant.py (GPU) share: person_detect-shaped models (side 96, width
1.0, full-range weights: the only shapes the fused table launches penta_rr / quad_rr / quad_mm / stage_6x6x128 / pair_front_tail
exist for) under the activation-quantisation plans of tools/tflite_writer.pd_quant_plan, and their six input images."""
import os
import sys

import numpy as np

from tests.synth import structured_images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import tflite_writer as tw  # noqa: E402

# name: (plan, element type, pairs in the 6x6x128 run, generator seed); the seeds are ones with which test_pd_quant_host's
# conditions on the oracle's tensors hold (about one seed in four leaves both of the head's classes varying over the images)
MODELS = {
    "shifted-i8": ("shifted", tw.INT8, 5, 13),
    "shifted-u8": ("shifted", tw.UINT8, 5, 22),
    "varied-i8": ("varied", tw.INT8, 5, 21),
    "varied-u8": ("varied", tw.UINT8, 5, 16),
    "stage-i8": ("stage", tw.INT8, 5, 3),
    "stage-u8": ("stage", tw.UINT8, 5, 12),
    "one_odd-i8": ("one_odd", tw.INT8, 5, 17),
    "stage-n2-i8": ("stage", tw.INT8, 2, 4),
}
NAMES = tuple(MODELS)
F32_IN_Q = (0.0125, 20)   # shifted-i8's input quantisation (mid + 20): another stem fill and input quantiser behind the f32 entry
STRUCTURED = (22, 25)     # tests.synth.structured_images: the noisy diagonal ramp and the noisy 4-pixel checkerboard
# Full-range weights everywhere but in the last 1x1 (256 -> 256 channels).  The host's bound of its accumulators is the sum of
# |w| over 256 taps times the largest |x - zero point| (up to 255): with uniform weights in +-128 about half of the channels pass
# 2^22, the operator loses the bit-pattern epilogue (ops.hip prepare_conv), and a pair + tail launch in the convert form does not
# take the pair in front of it -- pair_front_tail would never run.  +-64 is the widest that stays below whatever is drawn:
# 256 * 64 * 255 = 4 177 920 < 4 194 304.
LAST_PW_WMAX = 64
_blobs = {}


def last_pw(nst):
    return 2 * (8 + nst)


def limits(elem):
    return (0, 256) if elem == tw.UINT8 else (-128, 128)


def plan(name):
    p, elem, nst, _ = MODELS[name]
    return tw.pd_quant_plan(p, elem, nst)


def blob(name):
    if name not in _blobs:
        p, elem, nst, seed = MODELS[name]
        _blobs[name] = tw.person_detect_like(np.random.default_rng(seed), 96, 1.0, elem, False, nst, wmax={last_pw(nst): LAST_PW_WMAX},
                                             quant=plan(name), in_q=F32_IN_Q if name == "shifted-i8" else None)
    return _blobs[name]


def inputs(name):
    """[6, 96 * 96] in the model's element type: constant lo, constant hi - 1, two of uniform noise, two structured images"""
    elem, seed = MODELS[name][1], MODELS[name][3]
    lo, hi = limits(elem)
    dt = np.uint8 if elem == tw.UINT8 else np.int8
    rng = np.random.default_rng(100 + seed)
    x = np.empty((6, 96 * 96), dt)
    x[0], x[1] = lo, hi - 1
    x[2:4] = rng.integers(lo, hi, (2, 96 * 96)).astype(dt)
    st = structured_images(96)[list(STRUCTURED)]
    x[4:6] = st.view(np.uint8) ^ np.uint8(0x80) if elem == tw.UINT8 else st
    return x


def conv_like(ops):
    """indices of the operators with a clamp and a zero point of their own (stem, pairs, head)"""
    return [i for i, o in enumerate(ops) if o["name"] in ("conv_2d", "depthwise_conv_2d")]


def clamp(O, op, elem):
    """an operator's output clamp [lo, hi] in the element domain: what the oracle's activation makes of the type's limits"""
    lo, hi = limits(elem)
    dt = np.uint8 if elem == tw.UINT8 else np.int8
    if op["act"] == 0:
        return lo, hi - 1
    if op["act"] == 1:
        return O.relu(lo, op["out_zp"], dt), hi - 1
    return O.relu6(lo, op["out_scale"], op["out_zp"], dt), O.relu6(hi - 1, op["out_scale"], op["out_zp"], dt)


def launches(nst):
    """first and last operator of the five fused table launches of a model with `nst` pairs in the 6x6x128 run"""
    end = 12 + 2 * nst
    return {"penta_rr": (0, 4), "quad_rr": (5, 8), "quad_mm": (9, 12), "stage": (13, end), "pair_front_tail": (end + 1, end + 8)}
