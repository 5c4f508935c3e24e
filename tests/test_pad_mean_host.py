"""PAD (builtin 34) and MEAN (builtin 40) in the loader, without a GPU: the writer's models parse and report their kinds, every
refusal of include/microflow_amd.h answers with its code and its reason, a MEAN parses to the constants of the AveragePool2D
(+ Reshape) it stands for, and the generated Keras-style models load.  (Before these operators existed, loading the first model
here failed with `unsupported operator: 34` / `40`.)"""
import os
import sys

import numpy as np
import pytest

from tests import pad_ref
from tests.conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import tflite_writer as tw  # noqa: E402

Q = (0.05, -3)


def _load(layers, in_shape=(1, 6, 6, 4), in_q=Q, elem=tw.INT8):
    import microflow_rs_amd as mf
    return mf.model(tw.build_model(in_shape, in_q, layers, elem))


def _pad(**kw):
    d = dict(op="pad", pads=((0, 1), (0, 1)), out_shape=(1, 7, 7, 4), out_q=Q)
    d.update(kw)
    return d


def _mean(**kw):
    d = dict(op="mean", keep_dims=False, out_shape=(1, 4), out_q=(0.04, 2))
    d.update(kw)
    return d


def _refused(layers, status, *words, **kw):
    from microflow_rs_amd import _lib
    with pytest.raises(_lib.MicroflowError) as e:
        _load(layers, **kw)
    assert e.value.status == status, e.value
    for w in words:
        assert w in e.value.message, e.value.message


def test_pad_and_mean_models_load_and_report_their_kinds():
    from microflow_rs_amd import _lib
    m = _load([_pad(), _mean()])
    a, b = m.ops
    assert (a["kind"], a["name"], b["kind"], b["name"]) == (34, "pad", 40, "mean")
    assert (_lib.MF_OP_PAD, _lib.MF_OP_MEAN) == (34, 40)
    assert a["in_shape"] == (1, 6, 6, 4) and a["out_shape"] == (1, 7, 7, 4) and a["out_elems"] == 196
    assert a["in_scale"] == a["out_scale"] and a["in_zp"] == a["out_zp"] == -3
    assert m.op_pads(0) == ((0, 1), (0, 1))
    # the MEAN reports the global pool's geometry
    assert b["in_shape"] == (1, 7, 7, 4) and b["out_shape"] == (1, 4)
    assert (b["KH"], b["KW"], b["sh"], b["sw"], b["pad"], b["act"]) == (7, 7, 1, 1, 1, 0)
    with pytest.raises(_lib.MicroflowError) as e:
        m.op_pads(1)
    assert e.value.status == _lib.MF_ERR_INVALID_ARG


@pytest.mark.parametrize("elem", [tw.INT8, tw.UINT8], ids=["i8", "u8"])
@pytest.mark.parametrize("ptype", [tw.INT32, tw.INT64], ids=["int32", "int64"])
def test_pad_operand_types_and_all_four_sides(elem, ptype):
    q = (0.05, 200 if elem == tw.UINT8 else -128)
    m = _load([_pad(pads=((3, 0), (2, 5)), out_shape=(1, 9, 13, 4), out_q=q, pad_type=ptype)], in_q=q, elem=elem)
    assert m.op_pads(0) == ((3, 0), (2, 5)) and m.op(0)["out_zp"] == q[1] and m.output_shape == (1, 9, 13, 4)


def test_pad_refusals():
    from microflow_rs_amd import _lib
    U, I = _lib.MF_ERR_UNSUPPORTED, _lib.MF_ERR_INVALID_MODEL
    _refused([_pad(out_q=(0.05, -4))], U, "unsupported operator: 34", "PAD", "quantisation differ")
    _refused([_pad(out_q=(float(np.nextafter(np.float32(0.05), np.float32(1))), -3))], U, "unsupported operator: 34", "quantisation differ")
    _refused([_pad(pad_const=False)], U, "unsupported operator: 34", "not constant")
    _refused([_pad(out_q=((0.05, 0.05, 0.05, 0.05), (-3, -3, -3, -3)))], U, "unsupported operator: 34", "per-channel")
    _refused([_pad(paddings=((1, 0), (0, 1), (0, 1), (0, 0)), out_shape=(2, 7, 7, 4))], U, "unsupported operator: 34", "batch or channel pad")
    _refused([_pad(paddings=((0, 0), (0, 1), (0, 1), (0, 4)), out_shape=(1, 7, 7, 8))], U, "unsupported operator: 34", "batch or channel pad")
    _refused([_pad(pad_type=tw.INT8)], U, "unsupported operator: 34", "INT32 or INT64")
    _refused([_pad(paddings=((0, 1), (0, 1)))], U, "unsupported operator: 34", "[4, 2]")
    _refused([_pad(code="padv2")], U, "unsupported operator: 60", "PADV2")
    _refused([_pad(code="mirror_pad")], U, "unsupported operator: 100", "MIRROR_PAD")
    _refused([_pad(paddings=((0, 0), (0, -1), (0, 1), (0, 0)), out_shape=(1, 5, 7, 4))], I, "negative pad")
    _refused([_pad(out_shape=(1, 7, 8, 4))], I, "not input + pads")
    # rank 2: no H and W to pad
    _refused([dict(op="reshape", out_shape=(1, 144), out_q=Q), _pad(out_shape=(1, 144))], U, "unsupported operator: 34", "rank must be 4")


def test_mean_refusals():
    from microflow_rs_amd import _lib
    U, I = _lib.MF_ERR_UNSUPPORTED, _lib.MF_ERR_INVALID_MODEL
    _refused([_mean(axes=(1,), keep_dims=True, out_shape=(1, 1, 6, 4))], U, "unsupported operator: 40", "MEAN", "axes other than {1, 2}")
    _refused([_mean(axes=(2, 3), keep_dims=True, out_shape=(1, 6, 1, 1))], U, "unsupported operator: 40", "axes other than {1, 2}")
    _refused([_mean(axes=(0, 1, 2), out_shape=(1, 4))], U, "unsupported operator: 40", "axes other than {1, 2}")
    _refused([_mean(axes_const=False)], U, "unsupported operator: 40", "not constant")
    _refused([_mean(axes_type=tw.INT64)], U, "unsupported operator: 40", "INT32")
    _refused([_mean(keep_dims=True)], I, "keep_dims")                       # (the output shape is the other form's)
    _refused([_mean(out_shape=(1, 1, 1, 4))], I, "keep_dims")
    _refused([dict(op="reshape", out_shape=(1, 144), out_q=Q), _mean(out_shape=(1, 144))], U, "unsupported operator: 40", "rank must be 4")


@pytest.mark.parametrize("axes", [(1, 2), (2, 1), (-3, -2), (-2, 1), (1, 2, 1)])
@pytest.mark.parametrize("keep", [False, True], ids=["flat", "keep_dims"])
def test_mean_axes_in_any_order_and_negative(axes, keep):
    m = _load([_mean(axes=axes, keep_dims=keep, out_shape=(1, 1, 1, 4) if keep else (1, 4))])
    assert m.op(0)["kind"] == 40 and m.op(0)["out_shape"] == ((1, 1, 1, 4) if keep else (1, 4))


@pytest.mark.parametrize("elem", [tw.INT8, tw.UINT8], ids=["i8", "u8"])
@pytest.mark.parametrize("keep", [False, True], ids=["flat", "keep_dims"])
@pytest.mark.parametrize("shape", [(3, 3, 16), (7, 5, 20)])
def test_a_mean_parses_to_its_average_pool_twin(shape, keep, elem):
    """the same weights: every operator of the MEAN model has bit-equal constants and the geometry of the operator it stands for in
    the model written with AveragePool2D (+ Reshape)"""
    import microflow_rs_amd as mf
    rng = np.random.default_rng(7)
    lo = 0 if elem == tw.UINT8 else -128
    in_q, q = (0.05, lo + 90), (0.031, lo + 140)
    H, W, C = shape
    head = [dict(op="mean", keep_dims=keep, out_shape=(1, 1, 1, C) if keep else (1, C), out_q=q)]
    if keep:
        head.append(dict(op="reshape", out_shape=(1, C), out_q=q))
    head += [tw._fc_layer(rng, C, 10, q, "none", elem), dict(op="softmax", out_shape=(1, 10), out_q=(1.0 / 256.0, lo))]
    twin = pad_ref.twin_layers(head, (1, H, W, C))
    a, b = mf.model(tw.build_model((1, H, W, C), in_q, head, elem)), mf.model(tw.build_model((1, H, W, C), in_q, twin, elem))
    assert twin[0]["op"] == "average_pool_2d" and b.num_ops == a.num_ops + (0 if keep else 1)
    ia = 0
    for ib in range(b.num_ops):
        ob = b.op(ib)
        if ib == 1 and not keep:
            assert ob["name"] == "reshape"    # the MEAN's rank-2 output stands where this Reshape is
            continue
        oa = a.op(ia)
        assert oa["kind"] == (40 if ia == 0 else ob["kind"]) and ob["kind"] == (1 if ia == 0 else oa["kind"])
        for key in ("in_shape", "KH", "KW", "pad", "act", "n_c0", "n_c1", "in_scale", "out_scale", "in_zp", "out_zp", "out_elems"):
            assert oa[key] == ob[key], (ia, key, oa[key], ob[key])
        if ia == 0:
            assert oa["out_elems"] == C and (oa["sh"], oa["sw"]) == (1, 1)
        for ca, cb in zip(a.op_constants(ia), b.op_constants(ib)):
            assert np.asarray(ca).tobytes() == np.asarray(cb).tobytes(), (ia, ca, cb)
        ia += 1
    assert ia == a.num_ops


def test_the_keras_style_generators_load():
    import microflow_rs_amd as mf
    for elem in (tw.INT8, tw.UINT8):
        m = mf.model(tw.keras_mobilenet_v2(np.random.default_rng(3), 32, 0.25, elem, last=64))
        names = [o["name"] for o in m.ops]
        assert names[:2] == ["pad", "conv_2d"] and names[-3:] == ["mean", "fully_connected", "softmax"]
        assert names.count("pad") >= 3 and names.count("add") >= 3 and "average_pool_2d" not in names
        for i, o in enumerate(m.ops):
            if o["name"] == "pad":   # every PAD stands in front of a stride-2 VALID convolution, Keras' placement
                nxt = m.op(i + 1)
                assert nxt["name"] in ("conv_2d", "depthwise_conv_2d") and nxt["pad"] == 1 and (nxt["sh"], nxt["sw"]) == (2, 2)
                assert m.op_pads(i) in (((0, 1), (0, 1)), ((1, 1), (1, 1)))
        r = mf.model(tw.keras_resnet_stem(np.random.default_rng(3), 32, elem))
        assert [o["name"] for o in r.ops] == ["pad", "conv_2d", "pad", "max_pool_2d"]
        assert r.op_pads(0) == ((3, 3), (3, 3)) and r.op_pads(2) == ((1, 1), (1, 1)) and r.output_shape == (1, 8, 8, 64)
