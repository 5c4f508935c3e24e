"""Graph models run every way a model can be run (tests/composed_graph.py: the curated joins and the seeded graph grammar;
tests/graph_ref.py: every operator's expected tensor).  The checks are tests/test_gpu_composed.py's own, over models with joins, side
operators, PAD, MEAN, TRANSPOSE_CONV, dilated and grouped convolutions and resizes: the bytes with fusion on, off and shape-generic;
run_until at EVERY operator (a side operator and a join among them); predict and predict_quantized bit for bit; ragged batches on the
device; a consistent routing report; graph replay, sliding windows and the per-operator timing sweep on the joins.

A wrong fork buffer (csrc/model.cpp run_step), a group that swallowed a fork tensor (csrc/model_groups.cpp) or fork buffers sized for
a smaller tensor (csrc/tflite.cpp max_fork_elems) yields a wrong tensor only in such a composition."""
import math

import numpy as np
import pytest

from tests import composed as C
from tests import composed_graph as CG
from tests import test_gpu_composed as T
from tests.conftest import ROUTING_SWITCHED

pytestmark = pytest.mark.gpu

CASES = CG.cases()
IDS = [c.name for c in CASES]
ROUTED = [c for c in CG.JOINS if c.expect or c.never]

_prepared = {}


def _of(O, case):
    if case.name not in _prepared:
        _prepared[case.name] = T.Prepared(case, O)
    return _prepared[case.name]


@pytest.fixture(params=CASES, ids=IDS)
def p(request, O):
    return _of(O, request.param)


def test_bytes_with_fusion_on_off_and_generic(p):
    T.check_bytes_every_way(p)


def test_run_until_at_every_operator(p):
    T.check_run_until_every_operator(p)


def test_predict_and_predict_quantized_bit_for_bit(p):
    T.check_predict_bit_for_bit(p)


def test_batches_1_17_257_on_the_device(p):
    T.check_batches_on_the_device(p)


def test_the_routing_report_is_consistent(p):
    T.check_routing_report(p)


@pytest.mark.parametrize("case", ROUTED, ids=[c.name for c in ROUTED])
def test_joins_report_the_kernels_of_their_families(O, case):
    """a join with an `expect`: tests/test_gpu_composed.check_expected_kernels.  One with a `never` alone, whose launches are left
    open: none of them shows a forbidden prefix"""
    if ROUTING_SWITCHED:
        return
    p = _of(O, case)
    if case.expect:
        T.check_expected_kernels(p)
    ns = T.names(p.m)
    for bad in case.never:
        assert not any(nm.startswith(bad) for nm in ns), (bad, ns)


@pytest.mark.parametrize("case", CG.JOINS, ids=[c.name for c in CG.JOINS])
def test_the_per_operator_sweep_walks_the_joins(O, case):
    """time_device's sweep takes run_step's launches with an event behind each: one finite duration per operator (a side operator's
    among them); the timed pass leaves the expected bytes, and the run after it too"""
    import torch
    p = _of(O, case)
    m, n = p.m, p.n
    x = torch.as_tensor(p.x).cuda()
    out = torch.zeros((n, p.want.shape[1]), dtype=x.dtype, device="cuda")
    avg, per = m.time_device(x, out, n, warmup=0, iters=1, per_op=True)
    torch.cuda.synchronize()
    assert math.isfinite(avg) and len(per) == m.num_ops and all(math.isfinite(t) and t >= 0 for t in per), (avg, per)
    assert np.array_equal(out.cpu().numpy(), p.want), T._where(out.cpu().numpy(), p.want)
    got = m.run_quantized(x).cpu().numpy().reshape(n, -1)
    assert np.array_equal(got, p.want), T._where(got, p.want)


@pytest.mark.parametrize("name", ["join-feeds-join-i8", "join-feeds-join-swap", "side3-concat-into-fork", "side1-concat-into-fork"])
def test_graph_replay(O, name):
    """eager, captured + replayed, replayed, replayed: the fork buffers a captured graph refers to are the ones the eager run wrote"""
    import torch
    p = _of(O, CG.BY_NAME[name])
    m, n = p.m, p.n
    x = torch.as_tensor(p.x).cuda()
    out = torch.empty((n, p.want.shape[1]), dtype=x.dtype, device="cuda")
    m.set_graph(True)
    try:
        before = m.graph_launches
        for it in range(4):
            out.zero_()
            m.run_quantized(x, out=out)
            assert np.array_equal(out.cpu().numpy(), p.want), (it,) + T._where(out.cpu().numpy(), p.want)
        assert m.graph_launches > before
    finally:
        m.set_graph(False)


@pytest.mark.parametrize("name", ["concat-of-join-i8", "input-skip-f32-i8", "input-skip-f32-u8"])
def test_windows_of_one_source(O, name):
    """predict_windows over a frame 3 rows and 2 columns larger than the image, hop 1 (4 x 3 = 12 windows), against predict on the
    materialised windows; predict itself on three of them against the expected tensors.  concat-of-join: skips that are not the model
    input.  input-skip-f32: the join reads the model input itself -- the windows are gathered (and quantised) into a dense chunk before
    the run (csrc/model.cpp model_run_windows), so such a model is accepted and its skip is that chunk"""
    import torch
    from microflow_rs_amd.windows import Windows
    p = _of(O, CG.BY_NAME[name])
    m = p.m
    H, W, Cc = m.input_shape[1:]
    win = Windows.image((H + 3, W + 2), (H, W), Cc, 1)
    assert win.total == 12
    scale, zp = np.float32(p.in_q[0]), int(p.in_q[1])
    lo = 0 if p.case.elem == C.U8 else -128
    src = (scale * (np.random.default_rng(78).integers(lo, lo + 256, win.source_elems) - zp + 0.25)).astype(np.float32)
    dense = win.materialize(src).reshape((12,) + tuple(m.input_shape))
    want = m.predict(torch.as_tensor(dense).cuda()).cpu().numpy().reshape(12, -1)
    got = m.predict_windows(torch.as_tensor(src).cuda(), win).cpu().numpy().reshape(12, -1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), T._where(got.view(np.uint32), want.view(np.uint32))
    idx = [0, 5, 11]
    xq = C.quantize(dense[idx].reshape(3, -1), scale, zp, p.case.dtype)
    q = C.expected(p.case, O, xq)[-1]
    ref = C.dequantize(O, q, m.output_scale, m.output_zero_point, p.case.dtype)
    assert np.array_equal(want[idx].view(np.uint32), ref.view(np.uint32))
