"""Models with CONCATENATION joins on the device, run every way a model can be run: SqueezeNet 1.1 at a 32x32 input
(tools/tflite_writer.squeezenet: eight fire modules at 7x7, 3x3 and 1x1) with the 1x1 expand as the side operator -- the fused
launch -- and with the 3x3 as the side operator -- two launches --, a two-fire twin at an 8x8 input, and an identity-skip block
concat(x1, g(x1)) with x1 = concat(x0, f(x0)), whose first join's output is the second one's skip.  Expected tensors:
tests/concat_ref.py, for every operator in file order; computed once per model and left unchanged.  Bit-exact throughout."""
import os
import sys

import numpy as np
import pytest

from tests import composed as C
from tests import concat_ref as CR
from tests.conftest import ROOT, ROUTING_SWITCHED

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))

I8, U8 = 9, 3
ROWS = 5
FUSED_SIDE = "(fused into its CONCATENATION)"
NAMES = ["squeezenet32-i8", "squeezenet32-u8", "squeezenet32-i8-31", "twin-i8", "twin-u8", "dense-i8", "dense-u8"]
TWIN = [[(16, 64, 64)], [(32, 128, 128)]]


def _build(name):
    import tflite_writer as tw
    elem = U8 if "u8" in name else I8
    if name.startswith("squeezenet32"):
        return tw.squeezenet_layers(np.random.default_rng(1), 32, 10, elem, order="31" if name.endswith("31") else "13") + (elem,)
    if name.startswith("twin"):
        return tw.squeezenet_layers(np.random.default_rng(2), 8, 10, elem, fires=TWIN) + (elem,)
    return tw.dense_net_layers(np.random.default_rng(3), (4, 4, 16), (16, 32), elem, swap=(1,), head=4) + (elem,)


class Prepared:
    """one model on the device (tests/test_gpu_composed.py's shape, so that its checks apply)"""
    def __init__(self, name, O):
        import microflow_rs_amd as mf
        import tflite_writer as tw
        self.name, self.O = name, O
        self.in_shape, self.in_q, self.layers, self.elem = _build(name)
        self.case = self
        self.dtype = np.uint8 if self.elem == U8 else np.int8
        self.m = mf.Model(tw.build_model(self.in_shape, self.in_q, self.layers, self.elem))
        self.m.prepare(1)
        self.n = self.rows = ROWS
        self.x = self.inputs()
        self.outs = CR.segments(tw, O, self.in_shape, self.in_q, self.layers, self.elem)(self.x)
        for t in self.outs:
            t.setflags(write=False)
        self.want = self.outs[-1]
        self.joins = [i for i, L in enumerate(self.layers) if L["op"] == "concatenation"]
        self.sides = [i for i, L in enumerate(self.layers) if "side_of" in L]

    def inputs(self, n=None, seed=1):
        """row 0 all-minimum, row 1 all-maximum, the rest random (composed.Case.inputs)"""
        n = ROWS if n is None else n
        lo = 0 if self.elem == U8 else -128
        x = np.random.default_rng(400000 + NAMES.index(self.name) * 31 + seed).integers(lo, lo + 256, (n, int(np.prod(self.in_shape))), dtype=np.int16)
        x[0] = lo
        if n > 1:
            x[1] = lo + 255
        return x.astype(self.dtype)


_prepared = {}


def _named(O, name):
    if name not in _prepared:
        _prepared[name] = Prepared(name, O)
    return _prepared[name]


@pytest.fixture(params=NAMES)
def p(request, O):
    return _named(O, request.param)


def names(m):
    return [m.op(i)["kernel"] for i in range(m.num_ops)]


def test_the_fire_modules_run_the_fused_launch(p):
    if ROUTING_SWITCHED:
        pytest.skip("routing switched")
    ns = names(p.m)
    assert len(p.joins) == {"squ": 8, "twi": 2, "den": 2}[p.name[:3]]
    for j in p.joins:
        s = p.m.op_skip(j)[0]
        if s in p.sides and p.layers[s]["filters"].shape[1] == 1:       # a 1x1 side expand: one launch at the join
            L = p.layers[s]
            run_c = p.layers[j]["out_shape"][3] - L["out_shape"][3]
            assert ns[j] == "side_concat_rt<%d,%d,%d>" % (L["filters"].shape[3], L["out_shape"][3], run_c) and ns[s] == FUSED_SIDE, ns
        else:                                                          # a 3x3 side expand, or an identity skip: the join's own kernel
            assert ns[j] == "concat_c4<v16>", ns
            if s in p.sides:
                assert ns[s] not in ("", FUSED_SIDE) and not ns[s].startswith("side_concat_rt"), ns
    if p.name.endswith("31"):
        assert not any(n.startswith("side_concat_rt") for n in ns), ns


def test_run_until_every_operator(p):
    """... the side operators' indices (their tensor, computed from the tensor they read) and the main operators behind them included,
    with the groups on, off, and on the generic kernels"""
    from tests.test_gpu_composed import check_run_until_every_operator
    check_run_until_every_operator(p)
    for mode in ("set_fusion", "set_generic"):
        getattr(p.m, mode)(mode == "set_generic")
        try:
            check_run_until_every_operator(p)
        finally:
            getattr(p.m, mode)(mode != "set_generic")


def test_bytes_fused_unfused_and_generic(p):
    from tests.test_gpu_composed import check_bytes_every_way
    check_bytes_every_way(p)


def test_both_expand_orders_give_the_same_bytes(O):
    """the writer draws the same operators in either file order: the model with the 3x3 expand on the skip edge (two launches) gives
    the bytes of the one with the 1x1 expand there (the fused launch)"""
    a, b = _named(O, "squeezenet32-i8"), _named(O, "squeezenet32-i8-31")
    got = np.asarray(b.m.run_quantized(a.x)).reshape(a.n, -1)
    assert np.array_equal(got, a.want)


def test_predict_and_predict_quantized(p):
    from tests.test_gpu_composed import check_predict_bit_for_bit
    check_predict_bit_for_bit(p)
    p.m.set_fusion(False)
    try:
        check_predict_bit_for_bit(p)
    finally:
        p.m.set_fusion(True)
    got = np.asarray(p.m.run_quantized(p.x)).reshape(p.n, -1)          # host-fed
    assert np.array_equal(got, p.want)


def test_host_fed_chunks(O):
    """a host batch large enough to be cut into chunks (the twin: 192 input bytes per inference)"""
    p = _named(O, "twin-i8")
    n = 600000
    x = np.tile(p.x, (n // p.n, 1))
    got = np.asarray(p.m.run_quantized(x)).reshape(n, -1)
    assert np.array_equal(got, np.tile(p.want, (n // p.n, 1)))


@pytest.mark.parametrize("batch", [5, 131])
def test_graph_replay(p, batch):
    """run, capture + replay, replay -- then the same at a second batch size on the same model"""
    import torch
    m = p.m
    big = p.inputs(batch)
    x = torch.as_tensor(big).cuda()
    eager = m.run_quantized(x).cpu().numpy().reshape(batch, -1)
    assert np.array_equal(eager[:p.n], p.want)
    out = torch.empty((batch, m.output_elems), dtype=x.dtype, device="cuda")
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


def test_predict_windows_over_a_small_source(O):
    import torch
    from microflow_rs_amd.windows import Windows
    p = _named(O, "twin-i8")
    m = p.m
    win = Windows.image((12, 13), (8, 8), 3, 1)
    assert win.total == 30
    scale, zp = np.float32(p.in_q[0]), int(p.in_q[1])
    src = (scale * (np.random.default_rng(79).integers(-128, 128, win.source_elems) - zp + 0.25)).astype(np.float32)
    dense = win.materialize(src).reshape((30,) + tuple(m.input_shape))
    xq = C.quantize(dense.reshape(30, -1), scale, zp, p.dtype)
    q = CR.segments(sys.modules["tflite_writer"], O, p.in_shape, p.in_q, p.layers, p.elem)(xq)[-1]
    want = C.dequantize(O, q, m.output_scale, m.output_zero_point, p.dtype)
    got = m.predict_windows(torch.as_tensor(src).cuda(), win).cpu().numpy().reshape(30, -1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    src_q = C.quantize(src, scale, zp, p.dtype)                        # the quantised source: the same windows, as bytes
    got = m.run_windows(torch.as_tensor(src_q).cuda(), win).cpu().numpy().reshape(30, -1)
    assert np.array_equal(got, q)


def test_time_device_has_a_slot_for_every_operator(p):
    import torch
    m = p.m
    x = torch.as_tensor(p.inputs(64)).cuda()
    out = torch.empty((64, m.output_elems), dtype=x.dtype, device="cuda")
    avg, per = m.time_device(x, out, 64, warmup=1, iters=3, per_op=True)
    assert avg > 0 and len(per) == m.num_ops
    for j in p.joins:           # the join's slot holds the launch; the side operator's own slot is there and empty of a launch
        assert per[j] > 0, (j, per)
    if p.elem == I8:
        assert np.array_equal(out.cpu().numpy()[:p.n], p.want)
