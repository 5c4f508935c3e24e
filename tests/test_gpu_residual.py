"""Models with skip connections on the device, run every way a model can be run.  The expected tensors are tests/add_ref.segments':
the oracle for every run of reference operators, the numpy restatement at every ADD, the saved skip tensor carried across.

The models: MobileNet-v2-style blocks with their adds (back-to-back adds, a block without one, a skip that is the model input), in both
element types; a ResNet-style pair of blocks (ADD with relu, one written [skip, running]); and two guard models in which a fused group
would swallow the tensor a later ADD reads -- the fork has to stay a launch's result."""
import os
import sys

import numpy as np
import pytest

from tests import add_ref as A
from tests import composed as C
from tests.conftest import ROOT, ROUTING_SWITCHED

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))

I8, U8 = 9, 3
FUSED = C.FUSED
ROWS = C.ROWS
BLOCKS = [(64, 3, 1, 16), (64, 3, 1, 16), (96, 3, 2, 24), (96, 3, 1, 24)]


def _guard_block(tw, rng):
    """conv 1x1 -> depthwise 3x3 (fork) -> conv 1x1 to the same channels -> add: the pair group and the expand block would swallow it"""
    q0 = (0.05, -3)
    layers = [tw._conv_layer(rng, (8, 8, 16), q0, False, 32, 1, 1, "same", "relu6")]
    layers.append(tw._conv_layer(rng, (8, 8, 32), layers[-1]["out_q"], True, 32, 3, 1, "same", "relu6"))
    layers.append(tw._conv_layer(rng, (8, 8, 32), layers[-1]["out_q"], False, 32, 1, 1, "same", "none"))
    layers.append(tw._add_layer(rng, 1, (1, 8, 8, 32), layers[2]["out_q"], layers[1]["out_q"], "none"))
    return (1, 8, 8, 16), q0, layers, 1


def _guard_pool(tw, rng):
    """conv 3x3 (fork) -> AveragePool 3x3 stride 1 SAME -> add: the Conv2D + AveragePool2D stage would swallow it"""
    q0 = (0.05, -3)
    layers = [tw._conv_layer(rng, (8, 8, 16), q0, False, 32, 3, 1, "same", "relu")]
    q = layers[0]["out_q"]
    layers.append(dict(op="average_pool_2d", filter=(3, 3), padding="same", strides=(1, 1), act="none", out_shape=(1, 8, 8, 32), out_q=q))
    layers.append(tw._add_layer(rng, 0, (1, 8, 8, 32), q, q, "none", swap=True))
    return (1, 8, 8, 16), q0, layers, 0


def _build(name):
    import tflite_writer as tw
    if name in ("ir-i8", "ir-u8"):
        elem = U8 if name == "ir-u8" else I8
        return tw.inverted_residual_layers(np.random.default_rng(3), (8, 8, 16), BLOCKS, elem=elem, residual=True) + (None, elem)
    if name == "resnet":
        return tw.resnet_like_layers(np.random.default_rng(4), (8, 8, 16), 2, swap=(1,)) + (None, I8)
    if name == "guard-block":
        return _guard_block(tw, np.random.default_rng(5)) + (I8,)
    return _guard_pool(tw, np.random.default_rng(6)) + (I8,)


NAMES = ["ir-i8", "ir-u8", "resnet", "guard-block", "guard-pool"]


class Prepared:
    """one model on the device: prepared once, the expected tensors computed once and left unchanged (tests/test_gpu_composed.py's
    shape, so that its checks apply)"""
    def __init__(self, name, O):
        import microflow_rs_amd as mf
        import tflite_writer as tw
        self.name, self.O = name, O
        self.in_shape, self.in_q, self.layers, self.fork, self.elem = _build(name)
        self.case = self
        self.dtype = np.uint8 if self.elem == U8 else np.int8
        self.m = mf.Model(tw.build_model(self.in_shape, self.in_q, self.layers, self.elem))
        self.m.prepare(1)
        self.n = self.rows = ROWS
        self.x = self.inputs()
        self.outs = A.segments(tw, O, self.in_shape, self.in_q, self.layers, self.elem)(self.x)
        for t in self.outs:
            t.setflags(write=False)
        self.want = self.outs[-1]
        self.adds = [i for i, L in enumerate(self.layers) if L["op"] == "add"]

    def inputs(self, n=None, seed=1):
        """composed.Case.inputs: row 0 all-minimum, row 1 all-maximum, the rest random"""
        n = ROWS if n is None else n
        lo = 0 if self.elem == U8 else -128
        x = np.random.default_rng(200000 + NAMES.index(self.name) * 31 + seed).integers(lo, lo + 256, (n, int(np.prod(self.in_shape))), dtype=np.int16)
        x[0] = lo
        if n > 1:
            x[1] = lo + 255
        return x.astype(self.dtype)


_prepared = {}


@pytest.fixture(params=NAMES)
def p(request, O):
    if request.param not in _prepared:
        _prepared[request.param] = Prepared(request.param, O)
    return _prepared[request.param]


def names(m):
    return [m.op(i)["kernel"] for i in range(m.num_ops)]


def test_the_expected_tensors_are_spread(p):
    """the sums are neither constant nor saturated away: every ADD's expected tensor takes several values on the random rows (the
    deepest sums of the small block model take about a dozen), and fewer than three quarters of them sit at the type's ends (behind
    a relu about half sit at the zero point, which is the type's minimum)"""
    lo = 0 if p.elem == U8 else -128
    for i in p.adds:
        t = np.asarray(p.outs[i])[2:5].astype(np.int64)
        assert np.unique(t).size >= 8 and ((t == lo) | (t == lo + 255)).mean() < 0.75, (i, np.unique(t).size)


def test_run_until_every_operator(p):
    from tests.test_gpu_composed import check_run_until_every_operator
    check_run_until_every_operator(p)
    for mode in ("set_fusion", "set_generic"):      # ... and where a run ends inside a span with the groups gone
        getattr(p.m, mode)(mode == "set_generic")
        try:
            check_run_until_every_operator(p)
        finally:
            getattr(p.m, mode)(mode != "set_generic")


def test_bytes_fused_unfused_and_generic(p):
    from tests.test_gpu_composed import check_bytes_every_way
    check_bytes_every_way(p)


def test_predict_and_predict_quantized(p):
    from tests.test_gpu_composed import check_predict_bit_for_bit
    check_predict_bit_for_bit(p)
    for mode in ("set_fusion", "set_generic"):
        getattr(p.m, mode)(mode == "set_generic")
        try:
            check_predict_bit_for_bit(p)
        finally:
            getattr(p.m, mode)(mode != "set_generic")
    # host-fed, as numpy arrays
    got = np.asarray(p.m.run_quantized(p.x)).reshape(p.n, -1)
    assert np.array_equal(got, p.want)


def test_the_fork_tensor_is_a_launch_result(p):
    """no group swallows a tensor a later ADD reads: the operator that produces it is not inside a launch that goes on behind it, and
    an ADD is always a launch of its own"""
    ns = names(p.m)
    for i in p.adds:
        assert ns[i] in ("add_c16", "add_c16<fma>") or (ROUTING_SWITCHED and ns[i] == "add_generic"), ns
        src = p.m.op_skip(i)[0]
        if src >= 0:
            assert src + 1 < len(ns) and ns[src + 1] != FUSED, (i, src, ns)
    if p.fork is not None:   # the guard models: the producer has a kernel of its own
        assert ns[p.fork] not in ("", FUSED) and ns[p.fork + 1] != FUSED, ns


def test_blocks_keep_their_launch_beside_the_adds(O):
    """inverted-residual blocks report what they report without the adds (block_band_rt where the shape has it)"""
    import microflow_rs_amd as mf
    import tflite_writer as tw
    if ROUTING_SWITCHED:
        pytest.skip("routing switched")
    if "ir-i8" not in _prepared:
        _prepared["ir-i8"] = Prepared("ir-i8", O)
    p = _prepared["ir-i8"]
    plain = mf.Model(tw.inverted_residual_net(np.random.default_rng(3), (8, 8, 16), BLOCKS, residual=False))
    plain.prepare(1)
    with_adds = [n for i, n in enumerate(names(p.m)) if i not in p.adds]
    cut = lambda ns: [n.split("<")[0] for n in ns]   # (the launch's family: what is inside <> depends on the draws)
    assert cut(with_adds)[:12] == cut(names(plain))[:12], (with_adds, names(plain))
    assert any(n.startswith("block_band_rt") for n in with_adds[:12]) == any(n.startswith("block_band_rt") for n in names(plain)[:12])


@pytest.mark.parametrize("name", ["ir-i8", "resnet", "guard-block", "guard-pool"])
def test_no_copy_is_enqueued_for_a_skip(name, O):
    """device_ops() across one device-resident, aligned i8 run grows by exactly the launches the report shows"""
    import torch
    if name not in _prepared:
        _prepared[name] = Prepared(name, O)
    p = _prepared[name]
    m = p.m
    x = torch.as_tensor(p.x).cuda()
    out = torch.empty((p.n, m.output_elems), dtype=torch.int8, device="cuda")
    assert x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    m.run_quantized(x, out=out)
    launches = sum(1 for n in names(m) if n not in ("", FUSED))
    before = m.device_ops()
    m.run_quantized(x, out=out)
    torch.cuda.synchronize()
    assert m.device_ops() - before == launches, (m.device_ops() - before, launches, names(m))
    assert np.array_equal(out.cpu().numpy(), p.want)


@pytest.mark.parametrize("batch", [1, 5, 4099])
def test_graph_replay(p, batch):
    import torch
    m = p.m
    big = p.inputs(batch)
    x = torch.as_tensor(big).cuda()
    tdt = torch.uint8 if p.elem == U8 else torch.int8
    eager = m.run_quantized(x).cpu().numpy().reshape(batch, -1)
    k = min(batch, p.n)
    assert np.array_equal(eager[:k], p.want[:k])
    out = torch.empty((batch, m.output_elems), dtype=tdt, device="cuda")
    m.set_graph(True)
    try:
        g0 = m.graph_launches
        for _ in range(4):
            out.zero_()
            m.run_quantized(x, out=out)
            assert np.array_equal(out.cpu().numpy().reshape(batch, -1), eager)
        assert m.graph_launches > g0
    finally:
        m.set_graph(False)


def test_time_device_has_a_slot_for_every_add(p):
    import torch
    m = p.m
    x = torch.as_tensor(p.inputs(64)).cuda()
    out = torch.empty((64, m.output_elems), dtype=x.dtype, device="cuda")
    avg, per = m.time_device(x, out, 64, warmup=1, iters=3, per_op=True)
    assert avg > 0 and len(per) == m.num_ops
    for i in p.adds:
        assert per[i] > 0, (i, per)
    if p.elem == I8:
        assert np.array_equal(out.cpu().numpy()[:p.n], p.want)


def test_run_windows_matches_the_materialised_batch(O):
    import torch
    import microflow_rs_amd as mf
    if "ir-i8" not in _prepared:
        _prepared["ir-i8"] = Prepared("ir-i8", O)
    p = _prepared["ir-i8"]
    w = mf.Windows.image((16, 16), (8, 8), 16, 4)
    src = np.random.default_rng(8).integers(-128, 128, (16, 16, 16)).astype(np.int8)
    batch = w.materialize(src)
    assert batch.shape == (9, 8 * 8 * 16)
    want = np.asarray(p.m.run_quantized(batch)).reshape(9, -1)
    got = p.m.run_windows(torch.as_tensor(src).cuda(), w).cpu().numpy().reshape(9, -1)
    assert np.array_equal(got, want)
    assert np.array_equal(np.asarray(p.m.run_windows(src, w)).reshape(9, -1), want)
