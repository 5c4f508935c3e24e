"""Models that join fused-group families, run every way a model can be run (tests/composed.py: the joins, the seeded grammar and the
expected tensors -- the oracle between max pools, the numpy restatement at them).

The family test files run one family per model, so a grouping rule that claims an operator another rule already took, or a pick of
the run loop that is wrong only where a run ends inside a group (run_until, the batch and pointer fallbacks), would yield a wrong
tensor only for a composition none of them writes.  Here every join and every seed: the bytes with fusion on, off and shape-generic;
run_until at EVERY operator; predict and predict_quantized bit for bit; ragged batches on the device; and a routing report that is
consistent with itself -- and, for the joins, with the kernels their families' own tests assert."""
import numpy as np
import pytest

from tests import composed as C
from tests.conftest import ROUTING_SWITCHED

pytestmark = pytest.mark.gpu

FUSED = C.FUSED
CASES = C.cases()
IDS = [c.name for c in CASES]
BATCHES = (1, 17, 257)


class Prepared:
    """one case on the device: prepared once, the expected tensors computed once and left unchanged"""
    def __init__(self, case, O):
        import microflow_rs_amd as mf
        self.case, self.O = case, O
        self.in_shape, self.in_q, self.layers = case.model()
        self.m = mf.Model(case.blob())
        self.m.prepare(1)
        self.n = case.rows
        self.x = case.inputs()
        self.outs = [t[:self.n] for t in C.expected_once(case, O)]
        self.want = self.outs[-1]


_prepared = {}


@pytest.fixture(params=CASES, ids=IDS)
def p(request, O):
    case = request.param
    if case.name not in _prepared:
        _prepared[case.name] = Prepared(case, O)
    return _prepared[case.name]


def _named(O, name):
    if name not in _prepared:
        _prepared[name] = Prepared(C.BY_NAME[name], O)
    return _prepared[name]


def names(m):
    return [m.op(i)["kernel"] for i in range(m.num_ops)]


def _where(got, want):
    bad = np.argwhere(got != want)
    return int(bad.shape[0]), bad[:6].tolist()


# ---- the checks (the tests below call them; so may a script that prints instead of asserting) -----------------------------------------
def check_bytes_every_way(p):
    m, n = p.m, p.n
    got = np.asarray(m.run_quantized(p.x)).reshape(n, -1)
    assert np.array_equal(got, p.want), ("fused", names(m)) + _where(got, p.want)
    m.set_fusion(False)
    try:
        got = np.asarray(m.run_quantized(p.x)).reshape(n, -1)
    finally:
        m.set_fusion(True)
    assert np.array_equal(got, p.want), ("fusion off",) + _where(got, p.want)
    m.set_generic(True)
    try:
        got = np.asarray(m.run_quantized(p.x)).reshape(n, -1)
    finally:
        m.set_generic(False)
    assert np.array_equal(got, p.want), ("generic",) + _where(got, p.want)


def check_run_until_every_operator(p):
    m, n = p.m, p.n
    assert len(p.outs) == m.num_ops
    for i in range(m.num_ops):
        got = np.asarray(m.run_until(p.x, i)).reshape(n, -1)
        d = m.op(i)
        assert np.array_equal(got, p.outs[i]), ("run_until", i, d["name"], d["kernel"]) + _where(got, p.outs[i])


def check_predict_bit_for_bit(p):
    """f32 in, f32 out on the device: quantise (maxpool_ref.quantize_scalar's formula), the expected bytes, the oracle's dequantize.
    The floats are the rows' bytes dequantised and moved by less than a third of a step, so they quantise back to those bytes"""
    import torch
    m, n, case = p.m, p.n, p.case
    scale, zp = np.float32(p.in_q[0]), int(p.in_q[1])
    jitter = np.random.default_rng(77).uniform(-0.3, 0.3, p.x.shape)
    xf = (scale * (p.x.astype(np.float64) - zp + jitter)).astype(np.float32)
    assert np.array_equal(C.quantize(xf, scale, zp, case.dtype), p.x)
    want = C.dequantize(p.O, p.want, m.output_scale, m.output_zero_point, case.dtype)
    got = m.predict_quantized(torch.as_tensor(p.x).cuda()).cpu().numpy().reshape(n, -1)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("predict_quantized",) + _where(got.view(np.uint32), want.view(np.uint32))
    got = m.predict(torch.as_tensor(xf.reshape((n,) + tuple(m.input_shape))).cuda()).cpu().numpy().reshape(n, -1)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("predict", names(m)) + _where(got.view(np.uint32), want.view(np.uint32))


def check_batches_on_the_device(p):
    """1, 17 and 257 rows resident on the device: the launches with fusion on give the layer-wise bytes on every row, and the expected
    ones on the rows that have them"""
    import torch
    m, n = p.m, p.n
    big = p.case.inputs(BATCHES[-1])
    assert np.array_equal(big[:n], p.x)
    for b in BATCHES:
        x = torch.as_tensor(big[:b]).cuda()
        assert x.data_ptr() % 16 == 0
        got = m.run_quantized(x).cpu().numpy().reshape(b, -1)
        m.set_fusion(False)
        try:
            off = m.run_quantized(x).cpu().numpy().reshape(b, -1)
        finally:
            m.set_fusion(True)
        assert np.array_equal(got, off), ("batch", b, names(m)) + _where(got, off)
        k = min(b, n)
        assert np.array_equal(got[:k], p.want[:k]), ("batch", b) + _where(got[:k], p.want[:k])


def check_routing_report(p):
    """the report is consistent with itself: a Reshape reports nothing and every other operator something; the first launching operator
    is not fused into a previous one; with fusion off nothing is"""
    m = p.m
    kinds = [o["kind"] for o in m.ops]

    def consistent(ns):
        first = True
        for i, (k, nm) in enumerate(zip(kinds, ns)):
            assert (nm == "") == (k == 22), (i, ns)
            if k != 22:
                assert not (first and nm == FUSED), ns
                first = False
    on = names(m)
    consistent(on)
    m.set_fusion(False)
    try:
        off = names(m)
    finally:
        m.set_fusion(True)
    consistent(off)
    assert FUSED not in off, off
    assert names(m) == on


def device_ops_of_one_run(m, x):
    before = m.device_ops()
    m.run_quantized(x)
    return m.device_ops() - before


def check_expected_kernels(p):
    """a join's prefix list under default routing, the prefixes it must never show, and fewer device operations with fusion on than off
    at batch 17 on a resident aligned input; a contested join shows one of its outcomes"""
    import torch
    m, case = p.m, p.case
    ns = names(m)
    for bad in case.never:
        assert not any(nm.startswith(bad) for nm in ns), (bad, ns)
    if case.contested:
        assert any(all(ns[i].startswith(pre) for i, pre in o.items()) for o in case.outcomes), ns
        return
    for i, pre in case.expect:
        assert ns[i].startswith(pre), (i, pre, ns)
    x = torch.as_tensor(case.inputs(17)).cuda()
    assert x.data_ptr() % 16 == 0
    m.run_quantized(x)                                       # (capacity for 17 rows exists before anything is counted)
    on = device_ops_of_one_run(m, x)
    m.set_fusion(False)
    try:
        off = device_ops_of_one_run(m, x)
    finally:
        m.set_fusion(True)
    assert 0 < on < off, (on, off, ns)


# ---- every join and every seed ---------------------------------------------------------------------------------------------------------
def test_bytes_with_fusion_on_off_and_generic(p):
    check_bytes_every_way(p)


def test_run_until_at_every_operator(p):
    check_run_until_every_operator(p)


def test_predict_and_predict_quantized_bit_for_bit(p):
    check_predict_bit_for_bit(p)


def test_batches_1_17_257_on_the_device(p):
    check_batches_on_the_device(p)


def test_the_routing_report_is_consistent(p):
    check_routing_report(p)


@pytest.mark.parametrize("case", C.JOINS, ids=[c.name for c in C.JOINS])
def test_joins_report_the_kernels_of_their_families(O, case):
    if ROUTING_SWITCHED:
        return
    check_expected_kernels(_named(O, case.name))


@pytest.mark.parametrize("case", C.JOINS, ids=[c.name for c in C.JOINS])
def test_the_per_operator_sweep_walks_the_joins(O, case):
    """time_device's sweep takes run_step's launches with an event behind each (no figure is looked at beyond being one): one finite
    duration per operator; the timed pass in front of it leaves the expected bytes, and the run after it too"""
    import math
    import torch
    p = _named(O, case.name)
    m, n = p.m, p.n
    x = torch.as_tensor(p.x).cuda()
    out = torch.zeros((n, p.want.shape[1]), dtype=x.dtype, device="cuda")
    avg, per = m.time_device(x, out, n, warmup=0, iters=1, per_op=True)
    torch.cuda.synchronize()
    assert math.isfinite(avg) and len(per) == m.num_ops and all(math.isfinite(t) and t >= 0 for t in per), (avg, per)
    assert np.array_equal(out.cpu().numpy(), p.want), _where(out.cpu().numpy(), p.want)
    got = m.run_quantized(x).cpu().numpy().reshape(n, -1)
    assert np.array_equal(got, p.want), _where(got, p.want)


# ---- graph replay and windows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["max-pairs-head-i8", "pair-block-pair"])
def test_graph_replay(O, name):
    import torch
    p = _named(O, name)
    m, n = p.m, p.n
    x = torch.as_tensor(p.x).cuda()
    out = torch.empty((n, p.want.shape[1]), dtype=x.dtype, device="cuda")
    m.set_graph(True)
    try:
        before = m.graph_launches
        for it in range(4):                                  # eager, captured + replayed, replayed, replayed
            out.zero_()
            m.run_quantized(x, out=out)
            assert np.array_equal(out.cpu().numpy(), p.want), it
        assert m.graph_launches > before
    finally:
        m.set_graph(False)


def test_windows_of_one_source(O):
    """predict_windows over a 28 x 31 frame, hop 1 in both directions (5 x 8 = 40 windows of 24 x 24), against predict on the
    materialised windows"""
    import torch
    from microflow_rs_amd.windows import Windows
    p = _named(O, "max-pairs-head-i8")
    m = p.m
    H, W, Cc = m.input_shape[1:]
    win = Windows.image((H + 4, W + 7), (H, W), Cc, 1)
    assert win.total == 40
    scale, zp = np.float32(p.in_q[0]), int(p.in_q[1])
    src = (scale * (np.random.default_rng(78).integers(-128, 128, win.source_elems) - zp + 0.25)).astype(np.float32)
    dense = win.materialize(src).reshape((40,) + tuple(m.input_shape))
    want = m.predict(torch.as_tensor(dense).cuda()).cpu().numpy().reshape(40, -1)
    got = m.predict_windows(torch.as_tensor(src).cuda(), win).cpu().numpy().reshape(40, -1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), _where(got.view(np.uint32), want.view(np.uint32))
    # ... and predict itself on three of them against the expected tensors
    idx = [0, 17, 39]
    xq = C.quantize(dense[idx].reshape(3, -1), scale, zp, p.case.dtype)
    q = C.expected(p.case, O, xq)[-1]
    ref = C.dequantize(O, q, m.output_scale, m.output_zero_point, p.case.dtype)
    assert np.array_equal(want[idx].view(np.uint32), ref.view(np.uint32))
