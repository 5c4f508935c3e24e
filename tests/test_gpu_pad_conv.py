"""PAD + VALID Conv2D / DepthwiseConv2D as one launch, and the joins of the new group with its neighbours.

Every operator's tensor against np.pad with the zero point between runs of oracle operators (tests/pad_ref.py), under every way
of running a model: the default routing, mf_model_run_until at the PAD and at the convolution, fusion off, shape-generic, graph
replay.  Batch 5 (tests/pad_cases.images): an all-minimum image, an all-maximum one, one that is the zero point except on its
outermost rows and columns -- a window placed one off changes its bytes -- and two random ones; i8 and u8."""
import os
import sys

import numpy as np
import pytest

from tests import composed as C
from tests import pad_cases as P
from tests.conftest import ROOT, ROUTING_SWITCHED
from tests.pad_run import ELEMS, FUSED, Prepared, check_every_way, names

sys.path.insert(0, os.path.join(ROOT, "tools"))
import tflite_writer as tw  # noqa: E402

pytestmark = pytest.mark.gpu

# (Prepared, check_every_way and names live in tests/pad_run.py, shared with tests/test_gpu_pad_conv_steps.py)
_prepared = {}


def _case(O, name, ek):
    key = (name, ek)
    if key not in _prepared:
        elem, dt = ELEMS[ek]
        case = dict(P.CASES, **P.REFUSED)[name]
        _prepared[key] = Prepared(O, P.layers(case, np.random.default_rng(17), elem), elem, dt)
    return _prepared[key]


@pytest.mark.parametrize("ek", list(ELEMS))
@pytest.mark.parametrize("name", list(P.CASES) + list(P.REFUSED))
def test_pad_conv_bytes_every_way(O, name, ek):
    check_every_way(_case(O, name, ek))


@pytest.mark.parametrize("ek", list(ELEMS))
@pytest.mark.parametrize("name", list(P.CASES))
def test_pad_conv_is_one_launch(O, name, ek):
    """the PAD reports the launch, prefixed pad+, and the convolution that it was swallowed"""
    p = _case(O, name, ek)
    if ROUTING_SWITCHED:
        return
    got = names(p.m)
    assert got[0].startswith("pad+") and got[1] == FUSED, got
    case = P.CASES[name]
    want = {True: ("pad+dw_mm_rt", "pad+dw_gemm_rt"), False: ("pad+conv_rows_lds", "pad+conv_mm_rt", "pad+conv_gemm_rt")}[case[0]]
    assert got[0].startswith(want), got
    if case[8]:
        assert "wzp" in got[0], got   # filter zero points stay inside the launch
    before = p.m.device_ops()
    import torch
    xd = torch.as_tensor(p.x).cuda()
    out = torch.empty((5,) + tuple(p.m.output_shape[1:]), dtype=xd.dtype, device="cuda")
    p.m.run_quantized(xd, out=out)
    assert p.m.device_ops() - before == (1 if p.dt == np.int8 else 3)  # (u8: the two passes between real bytes and the internal domain)
    p.m.set_fusion(False)
    try:
        off = names(p.m)
    finally:
        p.m.set_fusion(True)
    assert off[0].startswith("pad_") and off[1] != FUSED, off


@pytest.mark.parametrize("ek", list(ELEMS))
def test_a_geometry_no_planner_takes_keeps_two_launches(O, ek):
    p = _case(O, "conv3s1_5x5x17", ek)
    if not ROUTING_SWITCHED:
        got = names(p.m)
        assert got[0] == "pad_generic" and got[1] not in (FUSED, "") and not got[1].startswith("pad+"), got


# ---- joins -------------------------------------------------------------------------------------------------------------------------
def _q(rng, lo, hi):
    return (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, hi - 20)))


def join_expand_pad_dw_project(rng, elem):
    """1x1 expand -> PAD -> depthwise 3x3 s2 VALID -> 1x1 project: MobileNet-v2's stride-2 block as Keras writes it"""
    lo, hi = (0, 256) if elem == tw.UINT8 else (-128, 128)
    in_q = _q(rng, lo, hi)
    a = tw._conv_layer(rng, (8, 8, 8), in_q, False, 48, 1, 1, "same", "relu6", elem)
    p = tw._pad_layer((8, 8, 48), a["out_q"], ((0, 1), (0, 1)))
    d = tw._conv_layer(rng, (9, 9, 48), a["out_q"], True, 48, 3, 2, "valid", "relu6", elem)
    c = tw._conv_layer(rng, (4, 4, 48), d["out_q"], False, 16, 1, 1, "same", "none", elem)
    return (1, 8, 8, 8), in_q, [a, p, d, c]


def join_pad_conv_maxpool(rng, elem):
    """PAD + Conv2D 3x3 s2 VALID -> MaxPool2D 2x2 s2"""
    lo, hi = (0, 256) if elem == tw.UINT8 else (-128, 128)
    in_q = _q(rng, lo, hi)
    p = tw._pad_layer((8, 8, 16), in_q, ((0, 1), (0, 1)))
    c = tw._conv_layer(rng, (9, 9, 16), in_q, False, 32, 3, 2, "valid", "relu", elem)
    mp = dict(op="max_pool_2d", filter=(2, 2), padding="valid", strides=(2, 2), act="none", out_shape=(1, 2, 2, 32), out_q=c["out_q"])
    return (1, 8, 8, 16), in_q, [p, c, mp]


def join_pad_reads_a_fork_tensor(rng, elem):
    """Conv2D 1x1 -> T; T -> PAD 1 all round -> Conv2D 3x3 s1 VALID -> ADD with T: the PAD's input has to stay in memory for the ADD"""
    lo, hi = (0, 256) if elem == tw.UINT8 else (-128, 128)
    in_q = _q(rng, lo, hi)
    a = tw._conv_layer(rng, (6, 6, 8), in_q, False, 16, 1, 1, "same", "relu6", elem)
    p = tw._pad_layer((6, 6, 16), a["out_q"], ((1, 1), (1, 1)))
    c = tw._conv_layer(rng, (8, 8, 16), a["out_q"], False, 16, 3, 1, "valid", "none", elem)
    add = tw._add_layer(rng, 0, (1, 6, 6, 16), c["out_q"], a["out_q"], "relu", elem)
    return (1, 6, 6, 8), in_q, [a, p, c, add]


JOINS = {
    "expand_pad_dw_project": join_expand_pad_dw_project,
    "pad_conv_maxpool": join_pad_conv_maxpool,
    "pad_reads_a_fork_tensor": join_pad_reads_a_fork_tensor,
    "keras_resnet_stem": lambda rng, elem: tw.keras_resnet_stem_layers(rng, 16, elem, filters=16),
    "keras_mobilenet_v2": lambda rng, elem: tw.keras_mobilenet_v2_layers(rng, 32, 0.25, elem),
}


def _join(O, name, ek):
    key = ("join", name, ek)
    if key not in _prepared:
        elem, dt = ELEMS[ek]
        _prepared[key] = Prepared(O, JOINS[name](np.random.default_rng(23), elem), elem, dt)
    return _prepared[key]


@pytest.mark.parametrize("ek", list(ELEMS))
@pytest.mark.parametrize("name", list(JOINS))
def test_joins_bytes_every_way(O, name, ek):
    check_every_way(_join(O, name, ek))


@pytest.mark.parametrize("ek", list(ELEMS))
def test_join_routing(O, ek):
    if ROUTING_SWITCHED:
        return
    got = names(_join(O, "expand_pad_dw_project", ek).m)
    # no block_band_rt over the padded tensor, no rule-1 pair of the depthwise and the project: the pad group took the depthwise
    assert not any("block_band" in k for k in got), got
    assert got[1].startswith(("pad+dw_mm_rt", "pad+dw_gemm_rt")) and got[2] == FUSED and got[0] != FUSED and got[3] not in (FUSED, ""), got
    got = names(_join(O, "pad_conv_maxpool", ek).m)
    assert got[0].startswith("pad+conv_") and got[1] == FUSED and got[2].startswith("maxpool_"), got
    got = names(_join(O, "pad_reads_a_fork_tensor", ek).m)
    assert got[1].startswith("pad+conv_") and got[2] == FUSED and got[3].startswith("add_"), got
    got = names(_join(O, "keras_resnet_stem", ek).m)
    assert got[0].startswith("pad+conv_rows_lds") and got[1] == FUSED and got[2].startswith("pad_c4") and got[3].startswith("maxpool_"), got
    m = _join(O, "keras_mobilenet_v2", ek).m
    got = names(m)
    for i in range(m.num_ops):
        if m.op(i)["name"] == "pad":   # the stem and every stride-2 block: one launch for the PAD and its convolution
            assert got[i].startswith("pad+") and got[i + 1] == FUSED, (i, got[i], got[i + 1])


@pytest.mark.parametrize("ek", list(ELEMS))
def test_pad_as_operator_0_through_predict(O, ek):
    """f32 in, f32 out with a PAD first: the separate quantise pass, then the launches; bit for bit"""
    import torch
    p = _join(O, "keras_resnet_stem", ek)
    m, n = p.m, p.n
    scale, zp = np.float32(p.in_q[0]), int(p.in_q[1])
    jitter = np.random.default_rng(77).uniform(-0.3, 0.3, p.x.shape)
    xf = (scale * (p.x.astype(np.float64) - zp + jitter)).astype(np.float32)
    assert np.array_equal(C.quantize(xf, scale, zp, p.dt), p.x)
    want = C.dequantize(O, p.want, m.output_scale, m.output_zero_point, p.dt)
    got = m.predict(torch.as_tensor(xf).cuda()).cpu().numpy().reshape(n, -1)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), names(m)
    got = np.asarray(m.predict(xf)).reshape(n, -1)   # host buffers
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
