"""The graph models of tests/composed_graph.py without a GPU: the library parses every curated join and every seed's graph into the
operators they were written from (skip sources, operand order, side operators, groups, dilation, resize factors and pads included),
no expected tensor in front of a Softmax is saturated, the grammar covers what it is meant to cover, and tests/graph_ref.interpret
gives, byte for byte at every operator, what each older interpreter gives on a model of its own family."""
import os
import sys

import numpy as np
import pytest

from tests import composed as C
from tests import composed_graph as CG
from tests import graph_ref
from tests.conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = CG.cases()
IDS = [c.name for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_library_parses_what_was_written(case):
    import microflow_rs_amd as mf
    import tflite_writer as tw
    in_shape, in_q, layers = case.model()
    m = mf.Model(case.blob())
    assert m.dtype == case.dtype and m.num_ops == len(layers)
    assert tuple(m.input_shape) == tuple(in_shape)
    assert (m.input_scale, m.input_zero_point) == (np.float32(in_q[0]), in_q[1])
    cur, q = tuple(in_shape), in_q                  # the running tensor
    shape_of, q_of = {-1: cur}, {-1: q}
    for i, L in enumerate(layers):
        d = m.op(i)
        side = "side_of" in L
        src, q_src = (shape_of[L["side_of"]], q_of[L["side_of"]]) if side else (cur, q)
        assert d["kind"] == CG.KIND[L["op"]], (i, d)
        assert tuple(d["in_shape"]) == src and tuple(d["out_shape"]) == tuple(L["out_shape"]), (i, d, src)
        assert (d["in_scale"], d["in_zp"]) == (np.float32(q_src[0]), q_src[1]), (i, d)
        if L["op"] in ("conv_2d", "depthwise_conv_2d"):
            w = np.asarray(L["filters" if L["op"] == "conv_2d" else "weights"])
            assert (d["KH"], d["KW"]) == w.shape[1:3], (i, d)
            assert m.op_dilation(i) == tuple(L.get("dilation", (1, 1))), (i, m.op_dilation(i))
            assert d["groups"] == (src[3] // w.shape[3] if L["op"] == "conv_2d" else 1), (i, d)
        elif L["op"] == "transpose_conv":
            assert (d["KH"], d["KW"]) == np.asarray(L["filters"]).shape[1:3], (i, d)
        elif L["op"] in ("average_pool_2d", "max_pool_2d"):
            assert (d["KH"], d["KW"]) == tuple(L["filter"]), (i, d)
        elif L["op"] == "mean":
            assert (d["KH"], d["KW"]) == src[1:3], (i, d)
        elif L["op"] == "resize_nearest_neighbor":
            assert m.op_upsample(i) == (L["out_shape"][1] // src[1], L["out_shape"][2] // src[2]), (i, m.op_upsample(i))
        elif L["op"] == "pad":
            assert m.op_pads(i) == tuple(tuple(p) for p in L["pads"]), (i, m.op_pads(i))
        elif L["op"] in graph_ref.JOINS:            # the skip source (a side operator among them) and which input the running tensor is
            assert m.op_skip(i) == (L["skip"], 1 if L.get("swap") else 0), (i, m.op_skip(i))
        if side:
            assert m.op_source(i) == L["side_of"], (i, m.op_source(i))
        else:
            with pytest.raises(mf.MicroflowError):
                m.op_source(i)
        if "strides" in L:
            assert (d["sh"], d["sw"], d["pad"]) == (L["strides"][0], L["strides"][1], tw.PAD[L["padding"]]), (i, d)
        if L["op"] not in ("reshape", "softmax", "pad", "resize_nearest_neighbor", "mean", "concatenation"):
            assert d["act"] == tw.ACT[L.get("act")], (i, d)
        q_out = L.get("out_q") or q
        assert (d["out_scale"], d["out_zp"]) == (np.float32(q_out[0]), q_out[1]), (i, d)
        shape_of[i], q_of[i] = tuple(L["out_shape"]), q_out
        if not side:
            cur, q = shape_of[i], q_out
    assert tuple(m.output_shape) == cur


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_no_expected_tensor_in_front_of_a_softmax_is_saturated(O, case):
    """tests/test_composed_host.py's condition: over the three random rows every such tensor takes at least 8 distinct values and has at
    most 75 % of its elements at the type's two ends.  A case that fails gets another seed, never a looser bound"""
    outs = C.expected_once(case, O)
    in_shape, in_q, layers = case.model()
    assert len(outs) == len(layers)
    lo = 0 if case.elem == C.U8 else -128
    x = case.inputs(C.ROWS)
    assert (x[0] == lo).all() and (x[1] == lo + 255).all() and np.array_equal(x[:case.rows], case.inputs())
    for i, t in enumerate(outs):
        assert t.dtype == case.dtype and t.shape == (C.ROWS, int(np.prod(layers[i]["out_shape"]))), (i, t.dtype, t.shape)
    for i, distinct, ends in C.spread(case, outs):
        assert distinct >= 8 and ends <= 0.75, (case.name, i, layers[i]["op"], distinct, ends)


def features(case):
    """what a case exercises, as the set the grammar's coverage is stated in"""
    in_shape, _, layers = case.model()
    f = {("elem", case.elem), ("wzp", case.wzp)}
    chans, run = {-1: in_shape[-1]}, -1         # every tensor's channels; the layer whose output is the running tensor
    for i, L in enumerate(layers):
        f.add(("op", L["op"]))
        if "dilation" in L:
            f.add(("dilated", L["op"]))
        if L["op"] == "conv_2d" and np.asarray(L["filters"]).shape[3] != chans[L.get("side_of", run)]:
            f.add(("grouped",))
        chans[i] = L["out_shape"][-1]
        if "side_of" not in L:
            run = i
        if L["op"] in graph_ref.JOINS:
            f.add(("join", L["op"], bool(L.get("swap"))))
            s = L["skip"]
            if s >= 0 and "side_of" in layers[s]:
                f.add(("side at", L["op"]))
                f.add(("side placed", "in front of the join" if s == i - 1 else "behind the fork"))
                s = layers[s]["side_of"]
            if s < 0:
                f.add(("join reads the model input",))
            elif layers[s]["op"] in graph_ref.JOINS:
                f.add(("a join's result is the next skip",))
    return f


def test_the_cases_are_the_ones_the_suite_is_meant_to_have():
    assert len(CG.SEEDS) == 24 and len(set(CG.SEEDS)) == 24
    assert len(set(IDS)) == len(IDS) and not set(IDS) & {c.name for c in C.cases()}
    for c in CG.JOINS:
        assert not (c.expect and c.outcomes), c.name
    g = [CG.graph_grammar(s) for s in CG.SEEDS]
    got = set().union(*(features(c) for c in g))
    want = {("elem", C.I8), ("elem", C.U8), ("wzp", "none"), ("wzp", "conv"), ("wzp", "all"),
            ("op", "transpose_conv"), ("op", "resize_nearest_neighbor"), ("op", "pad"), ("op", "mean"), ("op", "max_pool_2d"), ("op", "average_pool_2d"),
            ("op", "depthwise_conv_2d"), ("op", "fully_connected"), ("op", "softmax"),
            ("dilated", "conv_2d"), ("dilated", "depthwise_conv_2d"), ("grouped",),
            ("join", "add", False), ("join", "add", True), ("join", "concatenation", False), ("join", "concatenation", True),
            ("side at", "add"), ("side at", "concatenation"), ("side placed", "in front of the join"), ("side placed", "behind the fork"),
            ("join reads the model input",), ("a join's result is the next skip",)}
    assert want <= got, sorted(want - got, key=str)
    kinds = {s[0] for c in g for s in c.segments}
    assert {"tconv", "resize", "pad", "mean", "mark", "add", "concat", "side"} <= kinds, kinds
    assert any(c.segments[-1][0] in ("add", "concat") for c in g) or any(c.segments[-1][0] in ("add", "concat") for c in CG.JOINS)
    for c in g:
        n_ops = len(c.model()[2])
        assert max(c.shape[:2]) <= 16 and c.shape[2] in C.CHANNELS, c.name
        assert all(max(L["out_shape"][1:3]) <= 16 for L in c.model()[2] if len(L["out_shape"]) == 4), c.name
        assert 3 <= sum(s[0] not in ("mark", "gap", "mean", "flatten", "fc", "softmax") for s in c.segments) and n_ops <= 16, (c.name, n_ops)


# ---- the new interpreter against the older ones, each on a model of its own family ---------------------------------------------------
def _family(name):
    """-> (in_shape, in_q, layers, elem, the older interpreter's run(xq) -> every operator's tensor, or only the last one's)"""
    import tflite_writer as tw
    from oracle import oracle as O
    from tests import add_ref, concat_ref, dilated_ref, grouped_ref, maxpool_ref, pad_ref, resize_ref, shortcut_ref, tconv_ref
    rng = np.random.default_rng
    I8, U8 = tw.INT8, tw.UINT8
    if name == "residual":          # test_gpu_residual's "resnet"
        s, q, ls = tw.resnet_like_layers(rng(4), (8, 8, 16), 2, swap=(1,))
        return s, q, ls, I8, add_ref.segments(tw, O, s, q, ls, I8)
    if name == "shortcut":          # test_gpu_shortcut's projection blocks, the side operator in front of its ADD
        s, q, ls = tw.resnet_like_layers(rng(7), (8, 8, 16), [(1, 16), (2, 32)], U8, side="last")
        return s, q, ls, U8, shortcut_ref.segments(tw, O, s, q, ls, U8)
    if name == "concat":            # test_gpu_squeezenet's dense blocks (test_gpu_concat's generator)
        s, q, ls = tw.dense_net_layers(rng(3), (4, 4, 16), (16, 32), I8, swap=(1,), head=4)
        return s, q, ls, I8, concat_ref.segments(tw, O, s, q, ls, I8)
    if name == "pad":               # test_gpu_pad's Keras MobileNet-v2: PAD, ADD and MEAN
        s, q, ls = tw.keras_mobilenet_v2_layers(rng(8), 16, 0.25, I8, classes=5, blocks=[(1, 16, 1, 1), (6, 24, 2, 2)], last=32)
        return s, q, ls, I8, pad_ref.segments(tw, O, s, q, ls, I8)
    if name == "maxpool":           # test_gpu_maxpool's LeNet with max pools
        s, q, ls = tw.lenet_layers(rng(5), pool="max")
        return s, q, ls, I8, maxpool_ref.segments(tw, O, s, q, ls, I8)
    if name == "unet1":             # test_gpu_upconv's unet1 (resize_ref.compose gives the model's output only)
        q, ls = tw.unet1_layers(rng(26), (16, 16, 4), (8, 16), U8)
        s = (1, 16, 16, 4)
        return s, q, ls, U8, lambda xq: [None] * (len(ls) - 1) + [resize_ref.compose(tw, O, s, q, ls, U8, xq.reshape((len(xq),) + s[1:]))]
    if name == "tcn":               # test_gpu_tcn's model: pad_ref.segments on dilated_ref.twin
        s, q, ls = tw.tcn_layers(rng(24), 40, 8, 16)
        return s, q, ls, I8, pad_ref.segments(tw, O, s, q, dilated_ref.twin(ls), I8)
    if name == "resnext":           # test_gpu_resnext's model: its own composition, concat_ref.segments on grouped_ref.twin with MEAN as the pool
        s, q, ls = tw.resnext_layers(rng(25), elem=U8)
        twin = grouped_ref.twin(ls, s[3])
        pool = pad_ref.twin_layers(twin, s)       # (MEAN is the last but one: the indices in front of it stay)
        k = [i for i, L in enumerate(ls) if L["op"] == "mean"][0]
        run = concat_ref.segments(tw, O, s, q, pool, U8)
        return s, q, ls, U8, lambda xq: (lambda o: o[:k] + o[k + 1:])(run(xq))
    assert name == "conv_autoencoder"   # test_gpu_tconv's composition by hand: the oracle per Conv2D, tconv_ref per TRANSPOSE_CONV
    q, ls = tw.conv_autoencoder_layers(rng(67), (16, 16, 4), (16, 32))
    s, F32 = (1, 16, 16, 4), np.float32

    def composed(xq):
        t, shape, qi, outs = xq, s, q, []
        for L in ls:
            if L["op"] == "transpose_conv":
                c0 = (F32(L["bscale"]) / F32(L["out_q"][0])) * (np.asarray(L["bias"], np.int32) - np.asarray(L["bzp"], np.int32)).astype(F32)
                c1 = (F32(qi[0]) * F32(L["fscale"])) / F32(L["out_q"][0])
                t = tconv_ref.transpose_conv(t.reshape((len(t),) + shape[1:]), np.asarray(L["filters"], np.int8), qi[1], np.full(1, 0), L["strides"],
                                             L["out_shape"][1:3], c0, c1, L["out_q"][1], L["out_q"][0], L["act"])
            else:
                t = O.Model(tw.build_model(shape, qi, [L], I8)).run_quantized_batch(t.reshape(len(t), -1))
            shape, qi = tuple(L["out_shape"]), L["out_q"]
            outs.append(np.asarray(t).reshape(len(xq), -1))
        return outs
    return s, q, ls, I8, composed


@pytest.mark.parametrize("name", ["residual", "shortcut", "concat", "pad", "maxpool", "unet1", "tcn", "resnext", "conv_autoencoder"])
def test_the_interpreter_agrees_with_the_older_ones(O, name):
    import tflite_writer as tw
    in_shape, in_q, layers, elem, old = _family(name)
    dt = np.uint8 if elem == tw.UINT8 else np.int8
    lo = 0 if elem == tw.UINT8 else -128
    x = np.random.default_rng(91).integers(lo, lo + 256, (3, int(np.prod(in_shape))), dtype=np.int16)
    x[0], x[1] = lo, lo + 255
    x = x.astype(dt)
    want = old(x)
    got = graph_ref.interpret(tw, O, in_shape, in_q, layers, elem)(x)
    assert len(got) == len(layers) == len(want)
    checked = 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == dt and g.shape == (3, int(np.prod(layers[i]["out_shape"]))), (i, g.dtype, g.shape)
        if w is not None:
            assert np.array_equal(g, np.asarray(w).reshape(3, -1)), (name, i, layers[i]["op"], int((g != np.asarray(w).reshape(3, -1)).sum()))
            checked += 1
    assert checked == (1 if name == "unet1" else len(layers))
