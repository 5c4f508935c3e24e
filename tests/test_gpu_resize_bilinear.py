"""RESIZE_BILINEAR on the GPU: resize_bl_c4 (k_resize_bilinear.hip) and resize_bl_generic byte for byte against tests/bilinear_ref,
through ops.prepare_resize_bilinear; the bilinear decoder models against the oracle's convolutions composed with bilinear_ref."""
import os
import sys

import numpy as np
import pytest

from tests import bilinear_ref as B
from tests.conftest import ROOT
from tests.test_gpu_tconv import mf  # noqa: F401  (the module-scoped fixture: the package on a machine with a GPU)

sys.path.insert(0, os.path.join(ROOT, "tools"))
import tflite_writer as tw  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32

#         (H, W, C)     (sy, sx)  kernel
SHAPES = {
    "v16":     ((3, 5, 16),   (2, 2), "resize_bl_c4<v16>"),
    "dwords":  ((4, 3, 8),    (3, 1), "resize_bl_c4"),        # the f = 0 phase, DD = 12 (the multiply-shift), y only
    "bytes":   ((2, 7, 5),    (2, 3), "resize_bl_generic"),
    "clamped": ((1, 1, 16),   (2, 2), "resize_bl_c4<v16>"),   # every tap clamped
    "row-x4":  ((1, 6, 4),    (4, 4), "resize_bl_c4"),        # one row, factor 4, one dword per pixel
    "x-only":  ((5, 4, 32),   (1, 2), "resize_bl_c4<v16>"),
    "banded":  ((41, 33, 32), (2, 2), "resize_bl_c4<v16>"),   # halo rows cross band edges, the clamp sits at the image's edges only
}
CASES = [(k, False) for k in SHAPES] + [(k, True) for k in list(SHAPES)[:3]]


def _input(key, u8, special=None):
    shape = SHAPES[key][0]
    x = np.random.default_rng(sum(shape)).integers(-128, 128, (3,) + shape).astype(np.int8)
    if special == "all-min":
        x[:] = -128
    elif special == "checkerboard":   # -128 / 127 alternating over rows and pixels: the accumulator's bounds side by side
        x[:] = np.where((np.add.outer(np.arange(shape[0]), np.arange(shape[1])) % 2 == 0)[None, :, :, None], -128, 127)
    return (x.astype(np.int16) + 128).astype(np.uint8) if u8 else x


def _check(mf, key, u8, special=None):
    import torch
    from microflow_rs_amd import _lib
    shape, factors, kernel = SHAPES[key]
    x = _input(key, u8, special)
    want = B.resize_bilinear(x, *factors)
    # exact ties on both sides of zero: a property of the input, from the reference alone (none in a 1 x 1 image: its taps are one pixel)
    if not u8 and special is None and factors in ((2, 2), (4, 4)) and shape[:2] != (1, 1):
        acc, dd = B.accumulate(x, *factors), 4 * factors[0] * factors[1]
        tie = np.abs(acc) % dd == dd // 2
        assert (tie & (acc > 0)).any() and (tie & (acc < 0)).any()
    op = mf.ops.prepare_resize_bilinear(shape, factors, dtype=x.dtype)
    assert op.kernel == kernel, op.kernel
    if key == "banded":
        p = op.tile_plan()
        assert p["bands"] > 1 and shape[0] % p["band_rows"] != 0 and p["images"] == 1, p
    assert np.array_equal(mf.ops.resize_bilinear(mf.Tensor4D(x, [0.5], [7]), factors).buffer, want)
    tdt = torch.uint8 if u8 else torch.int8
    buf, xt = torch.full((want.size + 512,), 77, dtype=tdt, device="cuda"), torch.as_tensor(x).cuda()
    for generic in (False, True):
        op.set_generic(generic)
        assert not generic or op.kernel == "resize_bl_generic"
        _lib.check(_lib.lib().mf_op_run(op._h, xt.data_ptr(), 3, buf.data_ptr() + 256, torch.cuda.current_stream().cuda_stream))
        got = buf.cpu().numpy()
        assert np.array_equal(got[256:-256], want.reshape(-1)), (generic, int((got[256:-256] != want.reshape(-1)).sum()))
        assert (got[:256] == 77).all() and (got[-256:] == 77).all()
        buf[256:-256] = 77


@pytest.mark.parametrize("key,u8", CASES, ids=["%s-%s" % (k, "u8" if u else "i8") for k, u in CASES])
def test_resize_bilinear_is_the_contract_and_writes_nothing_else(mf, key, u8):
    _check(mf, key, u8)


@pytest.mark.parametrize("special", ["all-min", "checkerboard"])
@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
def test_the_range_bounds(mf, special, u8):
    _check(mf, "v16", u8, special)


def test_a_workgroup_walks_many_steps(mf):
    """More steps than the launch can have workgroups, so every workgroup stages over a tile it has read; a ragged last step."""
    import torch
    batch, unique = 70003, 61
    x = np.random.default_rng(9).integers(-128, 128, (unique, 3, 5, 16)).astype(np.int8)
    want = B.resize_bilinear(x, 2, 2)
    idx = torch.arange(batch) % unique
    op = mf.ops.prepare_resize_bilinear((3, 5, 16), (2, 2))
    assert op.kernel == "resize_bl_c4<v16>" and batch % op.tile_plan()["images"] != 0, (op.kernel, op.tile_plan())
    got = op(torch.as_tensor(x)[idx].cuda())
    bad = (got != torch.as_tensor(want)[idx].cuda()).flatten(1).any(1).nonzero().flatten()
    assert bad.numel() == 0, bad[:8].tolist()


def _oracle(O, shape, q, layers, elem, t):
    m = O.Model(tw.build_model((1,) + tuple(shape), q, layers, elem))
    return np.stack([m.run_quantized(v.reshape(-1)).reshape(-1) for v in t])


@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
@pytest.mark.parametrize("name", ["autoencoder", "seg_head"])
def test_the_bilinear_models_run_as_the_composed_operators(mf, name, u8):
    """[conv, resize_bilinear, conv, conv]: the oracle's model of the head, bilinear_ref, the oracle's model of the tail.  seg_head: the resize
    is the last operator.  run_quantized and predict, fused and unfused; the resize keeps its own launch either way."""
    from oracle import oracle as O
    elem, dt = (tw.UINT8, np.uint8) if u8 else (tw.INT8, np.int8)
    rng = np.random.default_rng(30)
    if name == "autoencoder":
        in_q, layers = tw.upsample_autoencoder_layers(rng, (16, 16, 4), (8,), elem=elem, interpolation="bilinear")
    else:
        in_q, layers = tw.seg_head_layers(rng, (16, 16, 4), (8, 16), 4, elem=elem)
    at = [L["op"] for L in layers].index("resize_bilinear")
    m = mf.model(tw.build_model((1, 16, 16, 4), in_q, layers, elem))
    xq = (np.random.default_rng(5).integers(-128, 128, (5, 16, 16, 4)) + (128 if u8 else 0)).astype(dt)
    mid_shape, mid_q, up = layers[at - 1]["out_shape"][1:], layers[at - 1]["out_q"], layers[at]["out_shape"][1:]
    t = _oracle(O, (16, 16, 4), in_q, layers[:at], elem, xq).reshape((5,) + tuple(mid_shape))
    t = B.resize_bilinear(t, up[0] // mid_shape[0], up[1] // mid_shape[1])
    want = (_oracle(O, up, mid_q, layers[at + 1:], elem, t) if at + 1 < len(layers) else t).reshape(5, -1)
    xf = ((xq.astype(f32) - f32(in_q[1])) * f32(in_q[0])).astype(f32)   # (exactly representable: predict quantises it back to xq)
    yf = (want.astype(f32) - f32(m.output_zero_point)) * f32(m.output_scale)
    for fusion in (True, False):
        m.set_fusion(fusion)
        got = m.run_quantized(xq).reshape(5, -1)
        assert np.array_equal(got, want), (fusion, int((got != want).sum()))
        assert m.op(at)["kernel"].startswith("resize_bl_c4"), m.op(at)["kernel"]
        assert np.array_equal(m.predict(xf).reshape(5, -1), yf), fusion
