"""The composed models of tests/composed.py without a GPU: the writer still gives every existing generator's bytes
(tests/golden/writer_blobs.json, recorded before stack_layers and the per-layer helpers were added), the library parses every join and
every seed's stack into the operators they were written from, and no expected tensor in front of a Softmax is saturated -- a parity
check over a tensor that sits at the type's two ends proves nothing."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from tests import composed as C
from tests.conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

CASES = C.cases()
IDS = [c.name for c in CASES]


def test_every_existing_generator_writes_the_bytes_it_wrote():
    import routing_dump
    import tflite_writer as tw
    with open(os.path.join(GOLDEN, "writer_blobs.json")) as f:
        want = json.load(f)
    rng = np.random.default_rng
    got = {}
    for name, make in routing_dump.corpus():
        blob = make()
        if isinstance(blob, str):
            with open(blob, "rb") as f:
                blob = f.read()
        got["corpus/" + name] = hashlib.sha256(blob).hexdigest()
    got["lenet"] = hashlib.sha256(tw.lenet(rng(5))).hexdigest()
    got["ds_cnn"] = hashlib.sha256(tw.ds_cnn(rng(6))).hexdigest()
    got["random_cnn-1000"] = hashlib.sha256(tw.random_cnn(rng(1000))).hexdigest()
    assert sorted(got) == sorted(want)
    assert got == want, sorted(k for k in got if got[k] != want[k])


def test_the_cases_are_the_ones_the_suite_is_meant_to_have():
    assert len(C.SEEDS) == 24 and len(set(C.SEEDS)) == 24
    assert len(set(IDS)) == len(IDS)
    for c in C.JOINS:
        assert bool(c.expect) != bool(c.outcomes), c.name          # a prefix list, or the outcomes of a contested join
    # the grammar covers both element types, every zero-point mode, both pools, every ending and every length of the conv-like part
    g = [C.grammar(s) for s in C.SEEDS]
    assert {c.elem for c in g} == {C.I8, C.U8} and {c.wzp for c in g} == {"none", "conv", "all"}
    kinds = {s[0] for c in g for s in c.segments}
    assert kinds == {"conv", "dw", "avgpool", "maxpool", "gap", "flatten", "fc", "softmax"}, kinds
    assert any(c.segments[-1][0] in ("conv", "dw", "avgpool", "maxpool") for c in g)           # a stack without a head
    assert any(("conv", 8, 1, 1, "same", "none") in c.segments and c.segments[-1] == ("softmax",) for c in g)   # person_detect's tail
    for c in g:
        assert max(c.shape[:2]) <= 16 and c.shape[2] in C.CHANNELS, c.name


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_library_parses_what_was_written(case):
    import microflow_rs_amd as mf
    import tflite_writer as tw
    in_shape, in_q, layers = case.model()
    m = mf.Model(case.blob())
    assert m.dtype == case.dtype and m.num_ops == len(layers)
    assert tuple(m.input_shape) == tuple(in_shape)
    assert (m.input_scale, m.input_zero_point) == (np.float32(in_q[0]), in_q[1])
    cur, q = tuple(in_shape), in_q
    for i, L in enumerate(layers):
        d = m.op(i)
        assert d["kind"] == C.KIND[L["op"]], (i, d)
        assert tuple(d["in_shape"]) == cur and tuple(d["out_shape"]) == tuple(L["out_shape"]), (i, d, cur)
        if L["op"] in ("conv_2d", "depthwise_conv_2d"):
            w = np.asarray(L["filters" if L["op"] == "conv_2d" else "weights"])
            assert (d["KH"], d["KW"]) == w.shape[1:3], (i, d)
        elif L["op"] in ("average_pool_2d", "max_pool_2d"):
            assert (d["KH"], d["KW"]) == tuple(L["filter"]), (i, d)
        if "strides" in L:
            assert (d["sh"], d["sw"], d["pad"]) == (L["strides"][0], L["strides"][1], tw.PAD[L["padding"]]), (i, d)
        if L["op"] not in ("reshape", "softmax"):
            assert d["act"] == tw.ACT[L.get("act")], (i, d)
        q = L.get("out_q") or q
        assert (d["out_scale"], d["out_zp"]) == (np.float32(q[0]), q[1]), (i, d)
        cur = tuple(L["out_shape"])
    assert tuple(m.output_shape) == cur


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_no_expected_tensor_in_front_of_a_softmax_is_saturated(O, case):
    """over the three random rows every such tensor takes at least 8 distinct values and has at most 75 % of its elements at the type's
    two ends.  A case that fails gets other scales or another seed (tests/composed.py), never a looser bound"""
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
