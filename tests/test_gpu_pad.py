"""The PAD operator on the device against np.pad (tests/pad_ref.py) and against pad_generic of the same handle, with guard bytes on
either side of the output; and MEAN heads against the oracle's average_pool_2d, routed as their AveragePool2D (+ Reshape) twins."""
import os
import sys

import numpy as np
import pytest

from tests import pad_cases as P
from tests import pad_ref
from tests.conftest import ROOT, ROUTING_SWITCHED

sys.path.insert(0, os.path.join(ROOT, "tools"))
import tflite_writer as tw  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
# (H, W, C), (top, bottom, left, right), the kernel of the default routing
SHAPES = [
    ((5, 6, 4), (0, 1, 0, 1), "pad_c4"),
    ((5, 5, 16), (1, 1, 1, 1), "pad_c4<v16>"),
    ((7, 5, 3), (3, 3, 3, 3), "pad_generic"),          # the byte-wise route
    ((4, 6, 1), (2, 0, 0, 3), "pad_generic"),
    ((6, 6, 20), (0, 0, 0, 0), "pad_c4"),              # a copy
    ((3, 40, 32), (1, 2, 2, 1), "pad_c4<v16>"),        # a row longer than one wave of 16-byte words
]


def _run(op, x, out_elems, dt):
    """the operator through mf_op_run into the middle of a buffer of sentinels: -> (the output, the guards are intact)"""
    import torch
    from microflow_rs_amd import _lib
    tdt = torch.uint8 if dt == np.uint8 else torch.int8
    xt = torch.as_tensor(x).cuda()
    n = x.shape[0] * out_elems
    buf = torch.full((GUARD + n + GUARD,), 0x5A, dtype=tdt, device="cuda")
    out = buf[GUARD:GUARD + n]
    assert xt.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    _lib.check(_lib.lib().mf_op_run(op._h, xt.data_ptr(), x.shape[0], out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    return h[GUARD:GUARD + n], bool((h[:GUARD] == 0x5A).all() and (h[GUARD + n:] == 0x5A).all())


@pytest.mark.parametrize("dt", [np.int8, np.uint8], ids=["i8", "u8"])
@pytest.mark.parametrize("shape,pads,kernel", SHAPES, ids=["%dx%dx%d" % s[0] for s in SHAPES])
def test_pad_operator(shape, pads, kernel, dt):
    from microflow_rs_amd import ops
    lo, hi = (0, 255) if dt == np.uint8 else (-128, 127)
    t, b, l, r = pads
    H, W, C = shape
    out_elems = (H + t + b) * (W + l + r) * C
    for zp in (lo, hi, lo + 93):      # both ends of T and one inside
        x = P.images(np.random.default_rng(11), (1,) + shape, (0.05, zp), dt)
        want = pad_ref.pad(x, ((t, b), (l, r)), zp).reshape(-1)
        op = ops.prepare_pad(shape, ((t, b), (l, r)), zp, dtype=dt)
        if not ROUTING_SWITCHED:
            assert op.kernel == kernel
        got, intact = _run(op, x, out_elems, dt)
        assert intact, "a guard byte was written"
        assert np.array_equal(got, want), (zp, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
        op.set_generic(True)
        assert op.kernel == "pad_generic"
        gen, intact = _run(op, x, out_elems, dt)
        op.set_generic(False)
        assert intact and np.array_equal(gen, want), (zp, "pad_generic", int((gen != want).sum()))
        # the Python mirror of the reference surface: numpy in, numpy out
        from microflow_rs_amd.tensor import Tensor4D
        y = ops.pad(Tensor4D(x, [0.05], [zp]), ((t, b), (l, r)))
        assert y.buffer.shape == (5, H + t + b, W + l + r, C) and np.array_equal(np.asarray(y.buffer).reshape(-1), want)
        assert list(y.scale) == [0.05] and list(y.zero_point) == [zp]


def test_pad_refuses_bad_arguments():
    from microflow_rs_amd import _lib, ops
    for pads in (((-1, 0), (0, 0)), ((0, 0), (0, -2))):
        with pytest.raises(_lib.MicroflowError) as e:
            ops.prepare_pad((4, 4, 4), pads, 0)
        assert e.value.status == _lib.MF_ERR_INVALID_ARG


def _names(m):
    return [m.op(i)["kernel"] for i in range(m.num_ops)]


@pytest.mark.parametrize("elem", [tw.INT8, tw.UINT8], ids=["i8", "u8"])
@pytest.mark.parametrize("keep", [False, True], ids=["flat", "keep_dims"])
@pytest.mark.parametrize("shape", [(3, 3, 16), (7, 5, 20)], ids=["3x3x16", "7x5x20"])
def test_mean_heads(O, shape, keep, elem):
    """MEAN + FullyConnected + Softmax: the oracle's bytes at every operator, and the launches of the AveragePool2D (+ Reshape) twin"""
    import microflow_rs_amd as mf
    rng = np.random.default_rng(5)
    dt = np.uint8 if elem == tw.UINT8 else np.int8
    lo = 0 if elem == tw.UINT8 else -128
    H, W, C = shape
    in_q, q = (0.05, lo + 90), (0.031, lo + 140)
    head = [dict(op="mean", keep_dims=keep, out_shape=(1, 1, 1, C) if keep else (1, C), out_q=q)]
    if keep:
        head.append(dict(op="reshape", out_shape=(1, C), out_q=q))
    head += [tw._fc_layer(rng, C, 10, q, "none", elem), dict(op="softmax", out_shape=(1, 10), out_q=(1.0 / 256.0, lo))]
    twin = pad_ref.twin_layers(head, (1, H, W, C))
    x = P.images(rng, (1, H, W, C), in_q, dt)
    outs = pad_ref.segments(tw, O, (1, H, W, C), in_q, head, elem)(x.reshape(5, -1))
    m, mt = mf.Model(tw.build_model((1, H, W, C), in_q, head, elem)), mf.Model(tw.build_model((1, H, W, C), in_q, twin, elem))
    m.prepare(5), mt.prepare(5)
    assert m.op(0)["kind"] == 40
    got = np.asarray(m.run_quantized(x)).reshape(5, -1)
    assert np.array_equal(got, outs[-1]), _names(m)
    assert np.array_equal(np.asarray(mt.run_quantized(x)).reshape(5, -1), outs[-1])
    for i in range(m.num_ops):
        assert np.array_equal(np.asarray(m.run_until(x, i)).reshape(5, -1), outs[i]), (i, m.op(i)["kernel"])
    m.set_fusion(False)
    assert np.array_equal(np.asarray(m.run_quantized(x)).reshape(5, -1), outs[-1])
    m.set_fusion(True)
    if not ROUTING_SWITCHED:
        twin_names = [k for i, k in enumerate(_names(mt)) if mt.op(i)["name"] != "reshape" or keep]
        assert _names(m) == twin_names, (_names(m), _names(mt))
