"""The models of tests/test_gpu_pd_quant.py (tests/pd_quant.py: person_detect's shapes under other activation quantisations), on
the CPU: the generator's default path is what it was, the library and the oracle read the new models alike, and -- judged on the
oracle's tensors alone -- the GPU comparisons are not vacuous: every tensor is spread, every clamp bound that is not the type's
limit is really held, and the clamps and zero points inside one launch really differ."""
import hashlib
import importlib
import itertools

import numpy as np
import pytest

from tests import pd_quant as P

tw = P.tw

# person_detect_like(quant=None, in_q=None): sha256 of the files the generator wrote before it had the two arguments, with
# tests/test_random_models.py's seeds (side * 7 + n_stage)
PINNED = [
    ((96, 1.0, 6, tw.INT8, False), "9c6ab5dcc9811d52297a830da3956cac13af9ddaf80bd0295b951fa270f00046"),
    ((96, 1.0, 2, tw.INT8, False), "0e9feac1ed7f0ed66bcf0afedcd4e221c25cbc9aa606c7c033619b64278a70b2"),
    ((64, 1.0, 5, tw.INT8, False), "548e7dbecf449fafccbc31fb711bf3c1f3d43ee0e49df385740eb8389d297b69"),
    ((72, 0.5, 5, tw.UINT8, True), "99c43fd366ab5d913b04c9502f85bb5ce6d2a311382b68e660d112710351c2ae"),
]


@pytest.mark.parametrize("case,digest", PINNED, ids=lambda v: "%dx%d-w%s-n%d" % (v[0], v[0], v[1], v[2]) if isinstance(v, tuple) else v[:8])
def test_default_path_writes_the_same_file(case, digest):
    side, width, nst, elem, wz = case
    blob = tw.person_detect_like(np.random.default_rng(side * 7 + nst), side, width, elem, wz, nst)
    assert hashlib.sha256(blob).hexdigest() == digest
    again = tw.person_detect_like(np.random.default_rng(side * 7 + nst), side, width, elem, wz, nst, quant=None, in_q=None)
    assert again == blob


def test_shipped_plan_draws_what_the_default_path_draws(O):
    """quant= consumes no random draw of its own: under the shipped quantisation as a plan, the weights and biases are the
    default path's (the scales are not: the stem's and the head's differ by design)"""
    lo, mid = -128, 0
    shipped = [("relu6", 0.0235294122, lo)] * 27 + [("none", 0.0125187514, mid - 1)]
    a = O.Model(tw.person_detect_like(np.random.default_rng(3), 96, 1.0))
    b = O.Model(tw.person_detect_like(np.random.default_rng(3), 96, 1.0, quant=shipped))
    assert a.num_ops == b.num_ops
    for i in range(1, 27):   # (between the stem and the head the constants themselves are equal: same scales, same draws)
        for x, y in zip(a.op_constants(i)[:3], b.op_constants(i)[:3]):
            assert np.array_equal(np.asarray(x).view(np.int32), np.asarray(y).view(np.int32)), i


@pytest.fixture(scope="module")
def layers(O):
    """per model: the oracle's tensors of every operator for the four non-constant images of the GPU file, concatenated"""
    cache = {}

    def get(name):
        if name not in cache:
            om = O.Model(P.blob(name))
            runs = [om.run_quantized(x, layers=True)[1] for x in P.inputs(name)[2:]]
            cache[name] = (om, [np.concatenate([r[i].reshape(-1) for r in runs]).astype(np.int64) for i in range(om.num_ops)])
        return cache[name]
    return get


@pytest.mark.parametrize("name", P.NAMES)
def test_parse_matches_oracle(O, name):
    mf = importlib.import_module("microflow_rs_amd")
    blob = P.blob(name)
    pm, om = mf.Model(blob), O.Model(blob)
    nst = P.MODELS[name][2]
    assert pm.dtype == om.dtype and pm.num_ops == om.num_ops == 2 * (8 + nst) + 5
    assert (pm.input_shape, pm.output_shape) == (om.in_shape, om.out_shape)
    for i in range(pm.num_ops):
        d, o = pm.op(i), om.ops[i]
        for k in ("kind", "in_shape", "out_shape", "KH", "KW", "sh", "sw", "pad", "act", "n_c0", "n_c1", "in_zp", "out_zp"):
            assert d[k] == o[k], (i, k, d[k], o[k])
        a, b = pm.op_constants(i), om.op_constants(i)
        for x, y in zip(a[:3], b[:3]):
            assert np.array_equal(np.asarray(x).view(np.int32), np.asarray(y).view(np.int32)), (i, d["name"])
        assert a[3] == b[3]
    # ... and the model is the plan: every conv-like layer's activation and output quantisation, each input's from the one before
    plan = P.plan(name)
    conv = P.conv_like(om.ops)
    assert len(conv) == len(plan)
    for (act, scale, zp), i in zip(plan, conv):
        o = om.ops[i]
        assert (o["act"], o["out_scale"], o["out_zp"]) == (tw.ACT[act], np.float32(scale), zp), i
        if i:
            assert (o["in_scale"], o["in_zp"]) == (om.ops[i - 1]["out_scale"], om.ops[i - 1]["out_zp"]), i
    if name == "shifted-i8":
        assert (om.in_scale, om.in_zp) == (np.float32(P.F32_IN_Q[0]), P.F32_IN_Q[1])


@pytest.mark.parametrize("name", P.NAMES)
def test_tensors_are_spread_and_every_bound_is_held(O, layers, name):
    """Conditions on the inputs, not tolerances.  Of every conv-like layer but the head (which has two bytes per image): at least
    64 distinct values, every clamp bound that is not the type's limit held by at least 2 % of the bytes, at least 20 % of the
    bytes strictly inside.  The head: at least 3 distinct values over the batch."""
    om, tensors = layers(name)
    elem = P.MODELS[name][1]
    lo, hi = P.limits(elem)
    conv = P.conv_like(om.ops)
    nontrivial = 0
    for i in conv[:-1]:
        t = tensors[i]
        cl, ch = P.clamp(O, om.ops[i], elem)
        assert lo <= cl <= t.min() and t.max() <= ch <= hi - 1, (i, cl, ch)
        assert len(np.unique(t)) >= 64, (i, len(np.unique(t)))
        if cl != lo:
            nontrivial += 1
            assert (t == cl).mean() >= 0.02, (i, "lower", cl, (t == cl).mean())
        if ch != hi - 1:
            nontrivial += 1
            assert (t == ch).mean() >= 0.02, (i, "upper", ch, (t == ch).mean())
        assert ((t > cl) & (t < ch)).mean() >= 0.20, (i, ((t > cl) & (t < ch)).mean())
    assert nontrivial >= 5, nontrivial   # (one_odd: five upper bounds and nothing else)
    assert len(np.unique(tensors[conv[-1]])) >= 3, tensors[conv[-1]]


def _members(O, om, elem, first, last):
    """(input zero point, clamp) of the conv-like operators first..last"""
    return {i: (om.ops[i]["in_zp"],) + P.clamp(O, om.ops[i], elem) for i in P.conv_like(om.ops) if first <= i <= last}


@pytest.mark.parametrize("name", ["varied-i8", "varied-u8"])
def test_varied_no_two_members_of_a_launch_agree(O, name):
    om = O.Model(P.blob(name))
    elem, nst = P.MODELS[name][1:3]
    for launch, (first, last) in P.launches(nst).items():
        mem = _members(O, om, elem, first, last)
        assert len(mem) >= 4, launch
        for a, b in itertools.combinations(mem, 2):
            assert mem[a] != mem[b], (launch, a, b, mem[a])
    # the 6x6x128 pairs read different zero points: what the stage builder has to refuse
    first, last = P.launches(nst)["stage"]
    assert len({om.ops[i]["in_zp"] for i in range(first, last, 2)}) > 1


@pytest.mark.parametrize("name", ["stage-i8", "stage-u8", "stage-n2-i8"])
def test_stage_pairs_share_the_zero_point_and_nothing_else(O, name):
    om = O.Model(P.blob(name))
    elem, nst = P.MODELS[name][1:3]
    lo, _ = P.limits(elem)
    first, last = P.launches(nst)["stage"]
    mem = _members(O, om, elem, first, last)
    assert {mem[i][0] for i in range(first, last + 1)} == {lo + 9}   # depthwise and 1x1 inputs alike
    pairs = [(mem[i][1:], mem[i + 1][1:]) for i in range(first, last, 2)]
    assert len(pairs) == nst
    for a, b in itertools.combinations(range(nst), 2):
        assert pairs[a][0] != pairs[b][0] or pairs[a][1] != pairs[b][1], (a, b)
    for a in range(nst - 1):   # neighbours differ in BOTH phases; every clamp of the run has a bound inside the type's range
        assert pairs[a][0] != pairs[a + 1][0] and pairs[a][1] != pairs[a + 1][1], a
    for dw, pw in pairs:
        assert dw[0] != lo and pw[0] != lo


def test_one_odd_changes_one_upper_bound_per_launch(O):
    om = O.Model(P.blob("one_odd-i8"))
    odd = {3, 7, 10, 17, 25}
    for launch, (first, last) in P.launches(5).items():
        mem = _members(O, om, tw.INT8, first, last)
        assert len(odd & set(mem)) == 1, launch
    for i in P.conv_like(om.ops)[:-1]:
        assert P.clamp(O, om.ops[i], tw.INT8) == ((-128, 72) if i in odd else (-128, 127)), i
        assert om.ops[i]["out_zp"] == -128
