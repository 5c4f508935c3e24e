"""The PAD + VALID convolution geometries that the host planner test (tests/test_pad_conv_plan_host.py) and the GPU tests
(tests/test_gpu_pad_conv.py) share, and the two-operator models written from them."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# name: (depthwise, H, W, C, K, stride, (top, bottom, left, right), N (Conv2D), filter zero points off the middle)
CASES = {
    "conv3s2_6x6x3": (False, 6, 6, 3, 3, 2, (0, 1, 0, 1), 8, False),
    "conv7s2_14x14x3": (False, 14, 14, 3, 7, 2, (3, 3, 3, 3), 8, False),
    "conv3s2_8x8x16": (False, 8, 8, 16, 3, 2, (0, 1, 0, 1), 32, False),
    "conv3s1_5x5x20": (False, 5, 5, 20, 3, 1, (1, 1, 1, 1), 12, False),
    "dw3s2_8x8x16": (True, 8, 8, 16, 3, 2, (0, 1, 0, 1), 16, False),
    "dw3s2_7x7x16": (True, 7, 7, 16, 3, 2, (1, 1, 1, 1), 16, False),
    "dw5s2_9x9x8": (True, 9, 9, 8, 5, 2, (1, 2, 1, 2), 8, False),
    "dw3s2_8x8x24_wz": (True, 8, 8, 24, 3, 2, (0, 1, 0, 1), 24, True),
}
# Refused by every planner, by their limits: the image rows are 85 bytes, no whole dwords, so conv_gemm_plan and dw_gemm_plan say no
# ((W C) % 4); conv_mm_plan says no (C % 16); and conv_rows_plan, which takes such rows, stops below 16 channels
REFUSED = {"conv3s1_5x5x17": (False, 5, 5, 17, 3, 1, (1, 1, 1, 1), 8, False)}


def out_hw(case):
    dw, H, W, C, K, S, (t, b, l, r), N, wz = case
    return (H + t + b - K) // S + 1, (W + l + r - K) // S + 1


def layers(case, rng, elem):
    """-> build_model's arguments for [PAD, the VALID convolution]"""
    import tflite_writer as tw
    dw, H, W, C, K, S, (t, b, l, r), N, wz = case
    lo, hi = (0, 256) if elem == tw.UINT8 else (-128, 128)
    in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, hi - 20)))
    pad = tw._pad_layer((H, W, C), in_q, ((t, b), (l, r)))
    conv = tw._conv_layer(rng, (H + t + b, W + l + r, C), in_q, dw, N, K, S, "valid", "relu6", elem, "all" if wz else "none")
    return (1, H, W, C), in_q, [pad, conv]


def images(rng, in_shape, in_q, dt, batch=5):
    """batch 5: image 0 all-minimum, image 1 all-maximum, image 2 the zero point everywhere except its outermost rows and columns (a
    window placed one off changes bytes), the rest random"""
    lo, hi = (0, 256) if dt == np.uint8 else (-128, 128)
    x = rng.integers(lo, hi, (batch,) + tuple(in_shape[1:])).astype(dt)
    x[0], x[1] = lo, hi - 1
    edge = x[2].copy()
    edge[edge == in_q[1]] = lo if in_q[1] != lo else hi - 1
    x[2] = in_q[1]
    for sl in ((0, slice(None)), (-1, slice(None)), (slice(None), 0), (slice(None), -1)):
        x[2][sl] = edge[sl]
    return x
