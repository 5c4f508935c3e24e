"""ADD and skip connections without a GPU: residual models load and report every ADD's source, input position and constants; the
host's constants are the restatement's (tests/add_ref.py); every graph form outside the supported class is refused with the reference's
answer and the reason behind it; the writer's blobs without residuals are byte for byte what they were; and the restatement gives
hand-computed known answers."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

from tests.conftest import ROOT
from tests import add_ref as A

sys.path.insert(0, os.path.join(ROOT, "tools"))

I8, U8 = 9, 3
BLOCKS = [(64, 3, 1, 16), (64, 3, 1, 16), (96, 3, 2, 24), (96, 3, 1, 24)]


def _check_adds(m, in_q, layers):
    """every ADD of the loaded model against its layer dict"""
    from microflow_rs_amd import _lib
    import microflow_rs_amd as mf
    quants = [L.get("out_q") for L in layers]
    for i, L in enumerate(layers):
        if quants[i] is None:
            quants[i] = quants[i - 1]
    n_add = 0
    for i, L in enumerate(layers):
        d = m.op(i)
        if L["op"] != "add":
            assert d["kind"] != 0
            with pytest.raises(mf.MicroflowError) as ei:
                m.op_skip(i)
            assert ei.value.status == _lib.MF_ERR_INVALID_ARG
            continue
        n_add += 1
        assert d["kind"] == 0 == _lib.MF_OP_ADD and d["name"] == "add"
        assert d["in_shape"] == tuple(L["out_shape"]) == d["out_shape"] and d["out_elems"] == int(np.prod(L["out_shape"]))
        assert d["act"] == {"none": 0, "relu": 1, "relu6": 3}[L["act"]]
        assert m.op_skip(i) == (L["skip"], 1 if L["swap"] else 0)
        q_run, q_skip = quants[i - 1], in_q if L["skip"] < 0 else quants[L["skip"]]
        qa, qb = (q_skip, q_run) if L["swap"] else (q_run, q_skip)
        assert d["n_c0"] == 1 and d["n_c1"] == 1
        c0, c1, _, _ = m.op_constants(i)
        ca, cb = A.constants(qa[0], qb[0], L["out_q"][0])
        assert c0[0].tobytes() == ca.tobytes() and c1[0].tobytes() == cb.tobytes()
        assert (np.float32(d["out_scale"]), d["out_zp"]) == (np.float32(L["out_q"][0]), L["out_q"][1])
        assert (np.float32(d["in_scale"]), d["in_zp"]) == (np.float32(q_run[0]), q_run[1])   # the running operand's
    return n_add


def test_residual_models_load_and_report_their_adds():
    """the test that fails without the feature: `unsupported operator: 0`"""
    import microflow_rs_amd as mf
    import tflite_writer as tw
    for elem in (I8, U8):
        shape, in_q, layers = tw.inverted_residual_layers(np.random.default_rng(3), (8, 8, 16), BLOCKS, elem=elem, residual=True)
        blob = tw.build_model(shape, in_q, layers, elem)
        assert blob == tw.inverted_residual_net(np.random.default_rng(3), (8, 8, 16), BLOCKS, elem=elem, residual=True)
        m = mf.Model(blob)
        assert [o["kind"] for o in m.ops] == [3, 4, 3, 0, 3, 4, 3, 0, 3, 4, 3, 3, 4, 3, 0, 1, 22, 9, 25]
        assert _check_adds(m, in_q, layers) == 3
        # a skip from the model input, back-to-back adds (the second reads the first one's sum), a block without an add
        assert [m.op_skip(i)[0] for i in (3, 7, 14)] == [-1, 3, 10]
    shape, in_q, layers = tw.resnet_like_layers(np.random.default_rng(4), (8, 8, 16), 2, swap=(1,))
    m = mf.Model(tw.build_model(shape, in_q, layers, I8))
    assert [o["kind"] for o in m.ops] == [3, 3, 0, 3, 3, 0, 1, 22, 9, 25]
    assert _check_adds(m, in_q, layers) == 2
    assert m.op_skip(2) == (-1, 0) and m.op_skip(5) == (2, 1) and m.op(2)["act"] == 1


def test_preprocess_add_is_two_f32_divisions():
    from microflow_rs_amd import _lib
    rng = np.random.default_rng(11)
    L = _lib.lib()
    cases = [(0.05, 0.05, 0.1), (0.05, 0.031, 0.07), (0.1, 0.1, 0.02)] + [tuple(float(np.float32(v)) for v in 10.0 ** rng.uniform(-4, 1, 3)) for _ in range(200)]
    for sa, sb, so in cases:
        ca, cb = C.c_float(), C.c_float()
        assert L.mf_preprocess_add(sa, sb, so, C.byref(ca), C.byref(cb)) == _lib.MF_OK
        want = A.constants(sa, sb, so)
        assert (np.float32(ca.value).tobytes(), np.float32(cb.value).tobytes()) == (want[0].tobytes(), want[1].tobytes())
    assert L.mf_preprocess_add(1.0, 1.0, 1.0, None, C.byref(cb)) == _lib.MF_ERR_INVALID_ARG


def test_the_restatement_gives_hand_computed_answers():
    F = np.float32
    # halves: ca = cb = 0.5 exactly; (a - 3) + (b + 7) odd -> a tie, rounded away from zero on both sides of -5's neighbourhood
    qa, qb, qo = (0.05, 3), (0.05, -7), (0.1, -5)
    assert A.constants(0.05, 0.05, 0.1) == (F(0.5), F(0.5))
    a = np.array([3, 4, 3, 2, 127, -128, 10], np.int8)
    b = np.array([-7, -7, -6, -7, 127, -128, 17], np.int8)
    #   sums of the differences: 0, 1, 1, -1, 258, -252, 31 -> -5 + half of it: -5, -4.5, -4.5, -5.5, 124, -131, 10.5
    assert A.add(a, b, qa, qb, qo).tolist() == [-5, -5, -5, -6, 124, -128, 11]
    assert A.add(a, b, qa, qb, qo, "relu").tolist() == [-5, -5, -5, -5, 124, -5, 11]
    # relu6's upper bound: quantize(6.0, 0.1, -5) = 55
    assert A.add(a, b, qa, qb, qo, "relu6").tolist() == [-5, -5, -5, -5, 55, -5, 11]
    # equal quantisations: a + b - z, clipped
    q = (0.25, 10)
    a, b = np.array([0, 255, 200, 10], np.uint8), np.array([0, 255, 10, 10], np.uint8)
    assert A.add(a, b, q, q, q).tolist() == [0, 255, 200, 10]


def test_ties_round_away_from_zero_in_the_restatement():
    # -4.5 -> -5 and 10.5 -> 11 above; here the positive and negative ties around zero with zo = 0
    qa = qb = (0.05, 0)
    a = np.array([1, -1, 3, -3], np.int8)
    b = np.zeros(4, np.int8)
    assert A.add(a, b, qa, qb, (0.1, 0)).tolist() == [1, -1, 2, -2]


# ---- the graph forms that do not load -----------------------------------------------------------------------------------------------
def _conv(rng, shape, q, n=None, k=1, act="none"):
    import tflite_writer as tw
    return tw._conv_layer(rng, shape, q, False, n or shape[2], k, 1, "same", act)


def _refused_models():
    import tflite_writer as tw
    rng = np.random.default_rng(21)
    shp, S = (4, 4, 8), (1, 4, 4, 8)
    in_q, oq = (0.05, 3), (0.07, -5)

    def chain(n):
        layers, q = [], in_q
        for _ in range(n):
            layers.append(_conv(rng, shp, q))
            q = layers[-1]["out_q"]
        return layers

    def add(**kw):
        d = dict(op="add", skip=-1, swap=False, act="none", out_shape=S, out_q=oq)
        d.update(kw)
        return d

    const = dict(shape=S, q=(0.05, 0), data=np.zeros(S, np.int8))
    fresh = dict(shape=S, q=(0.05, 0))
    per_channel = dict(shape=S, q=(np.full(8, 0.05, np.float32), np.zeros(8, np.int64)))
    forms = {
        "a constant operand": chain(1) + [add(inputs=["cur", const])],
        "differing shapes": chain(1) + [_conv(rng, shp, (0.05, 0), n=4), add(skip=0, out_shape=(1, 4, 4, 4))],
        "neither input is the running value": chain(3) + [add(inputs=[0, 1])],
        "both inputs are the same tensor": chain(2) + [add(inputs=["cur", "cur"])],
        "two skip tensors alive at once": chain(4) + [add(skip=1), _conv(rng, shp, oq), add(skip=0)],     # nested: 0 .. 6 around 1 .. 4
        "two skip tensors alive at once ": chain(3) + [add(skip=0), _conv(rng, shp, oq), add(skip=1)],    # overlapping: 0 .. 3 and 1 .. 5
        "a fork tensor is used twice": chain(3) + [add(skip=0), _conv(rng, shp, oq), add(skip=0)],
        "mixed element types": chain(2) + [add(inputs=["cur", dict(shape=S, q=(0.05, 0), type=tw.UINT8)])],
        "mixed element types ": chain(2) + [add(skip=0, out_type=tw.UINT8), _conv(rng, shp, oq)],  # (the model's output stays i8)
        "per-channel quantisation": chain(2) + [add(inputs=["cur", per_channel])],
        "no earlier tensor of the chain": chain(2) + [add(inputs=["cur", fresh])],
    }
    return {k: tw.build_model(S, in_q, v, I8) for k, v in forms.items()}


REFUSED = ["a constant operand", "differing shapes", "neither input is the running value", "both inputs are the same tensor",
           "two skip tensors alive at once", "two skip tensors alive at once ", "a fork tensor is used twice", "mixed element types",
           "mixed element types ", "per-channel quantisation", "no earlier tensor of the chain"]


@pytest.mark.parametrize("form", REFUSED)
def test_every_other_form_of_add_is_refused_with_the_reason(form):
    import microflow_rs_amd as mf
    from microflow_rs_amd import _lib
    blob = _refused_models()[form]
    with pytest.raises(mf.MicroflowError) as ei:
        mf.Model(blob)
    assert ei.value.status == _lib.MF_ERR_UNSUPPORTED, str(ei.value)
    assert "unsupported operator: 0 (ADD:" in str(ei.value) and form.strip() in str(ei.value), str(ei.value)


def test_the_forms_beside_them_load():
    """the same writer calls in a supported arrangement: the refusals above are about the graph, not about the writer"""
    import microflow_rs_amd as mf
    import tflite_writer as tw
    rng = np.random.default_rng(22)
    shp, S, in_q, oq = (4, 4, 8), (1, 4, 4, 8), (0.05, 3), (0.07, -5)
    layers = [_conv(rng, shp, in_q), _conv(rng, shp, (0.05, 0)), dict(op="add", skip=0, swap=True, act="relu6", out_shape=S, out_q=oq),
              _conv(rng, shp, oq), dict(op="add", skip=2, swap=False, act="none", out_shape=S, out_q=oq)]
    m = mf.Model(tw.build_model(S, in_q, layers, I8))
    assert m.op_skip(2) == (0, 1) and m.op_skip(4) == (2, 0) and m.op(2)["act"] == 3


def test_bad_scales_are_refused():
    import microflow_rs_amd as mf
    import tflite_writer as tw
    from microflow_rs_amd import _lib
    rng = np.random.default_rng(23)
    shp, S, in_q = (4, 4, 8), (1, 4, 4, 8), (0.05, 3)
    L = _lib.lib()
    for bad in (0.0, -0.1, float("inf"), float("nan")):
        layers = [_conv(rng, shp, in_q), dict(op="add", skip=-1, swap=False, act="none", out_shape=S, out_q=(bad, 0))]
        with pytest.raises(mf.MicroflowError) as ei:
            mf.Model(tw.build_model(S, in_q, layers, I8))
        assert ei.value.status == _lib.MF_ERR_INVALID_MODEL, str(ei.value)
        # the operator: a bad argument whether or not there is a device to create it on
        for args in ((bad, 0, 0.05, 0, 0.05, 0), (0.05, 0, bad, 0, 0.05, 0), (0.05, 0, 0.05, 0, bad, 0)):
            h = C.c_void_p()
            for fn in (L.mf_add_create, L.mf_add_create_u8):
                assert fn(0, 16, *args, 0, 1.0, 1.0, C.byref(h)) == _lib.MF_ERR_INVALID_ARG and not h.value


# sha256 of the blob the writer gave before it knew ADD (recorded from the parent commit)
PARENT_BLOB = {"i8": (42872, "036c8532827eccf744b53bbfcbebe9fa063330b89f4360798f77d28443e50a5e"),
               "u8": (42872, "4787ee64cae5e1914bbe2b73f8c94b057832c889871573b2b085899596c363c8")}


def test_without_residuals_the_writer_gives_the_bytes_it_gave():
    import tflite_writer as tw
    for elem, key in ((I8, "i8"), (U8, "u8")):
        blob = tw.inverted_residual_net(np.random.default_rng(3), (8, 8, 16), BLOCKS, elem=elem, wzp_nonzero=elem == U8)
        assert (len(blob), hashlib.sha256(blob).hexdigest()) == PARENT_BLOB[key]
        assert blob == tw.inverted_residual_net(np.random.default_rng(3), (8, 8, 16), BLOCKS, elem=elem, wzp_nonzero=elem == U8, residual=False)
        # ... and the residual form without its ADD entries is a plain chain build_model writes as before (the same layers: the adds
        # draw their quantisation behind the block's)
        shape, in_q, layers = tw.inverted_residual_layers(np.random.default_rng(3), (8, 8, 16), BLOCKS, elem=elem, residual=True)
        plain = [L for L in layers if L["op"] != "add"]
        assert len(plain) == len(layers) - 3 and len(tw.build_model(shape, in_q, plain, elem)) > 0


# ---- the gated form -----------------------------------------------------------------------------------------------------------------
def _fma(c, u, k):
    """f32(c * u + k) with ONE rounding, for f32 c and k and bytes u: the product is exact in x87 extended precision (24 + 8 bits) and
    the sum is checked to be (Fast2Sum), so the conversion to f32 is the only rounding"""
    LD = np.longdouble
    assert np.finfo(LD).nmant >= 63
    prod = LD(c) * u.astype(LD)
    k = np.broadcast_to(np.asarray(k, np.float32).astype(LD), prod.shape)
    s = prod + k
    assert np.all((s - prod) == k) and np.all((s - k) == prod)
    return s.astype(np.float32)


def _forms_agree(ca, cb, za, zb, so, zo, act, dt):
    """brute force over all 65 536 pairs: the statement (tests/add_ref.add) against fma(cb, ub, fma(ca, ua, k1)) with the same tail"""
    from tests import maxpool_ref as R
    F = np.float32
    off = 0 if dt == np.uint8 else 128
    k1 = F(float(zo) - float(ca) * (off + za) - float(cb) * (off + zb))
    u = np.arange(256)
    ua, ub = np.repeat(u, 256), np.tile(u, 256)
    want = A.add((ua - off).astype(dt), (ub - off).astype(dt), (1.0, za), (1.0, zb), (so, zo), act, consts=(ca, cb))
    y = _fma(F(cb), ub, _fma(F(ca), ua, k1))
    got = R.activation(R.saturate(R.roundf(y), dt), act, so, zo, dt).astype(dt)
    return bool(np.array_equal(got, want)), k1


def test_the_gated_form_is_admitted_exactly_where_the_two_forms_agree():
    from microflow_rs_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(77)
    sets = [((0.05, 3), (0.05, 3), (0.05, 3)), ((0.05, 3), (0.05, -7), (0.1, -5)), ((0.05, 3), (0.031, -7), (0.07, -5)), ((0.1, 3), (0.1, -7), (0.02, -5))]
    for _ in range(10):
        sets.append(tuple((float(np.float32(rng.uniform(0.01, 0.2))), int(rng.integers(-60, 60))) for _ in range(3)))
    seen = set()
    for qa, qb, qo in sets:
        for dt in (np.int8, np.uint8):
            for act_name, act in (("none", 0), ("relu", 1), ("relu6", 3)):
                off = 128 if dt == np.uint8 else 0
                za, zb, zo = qa[1] + off, qb[1] + off, qo[1] + off
                ca, cb = A.constants(qa[0], qb[0], qo[0])
                agree, k1 = _forms_agree(ca, cb, za, zb, qo[0], zo, act_name, dt)
                k, ok = C.c_float(), C.c_int(-1)
                assert L.mf_add_fma_form(ca, cb, za, zb, qo[0], zo, act, int(dt == np.uint8), C.byref(k), C.byref(ok)) == _lib.MF_OK
                assert ok.value == int(agree), (qa, qb, qo, dt, act_name)
                if agree:
                    assert np.float32(k.value).tobytes() == k1.tobytes()
                seen.add(agree)
    # exact arithmetic (ca = cb = 1, and 0.5) is always admitted
    for qa, qb, qo in sets[:2]:
        ca, cb = A.constants(qa[0], qb[0], qo[0])
        assert _forms_agree(ca, cb, qa[1], qb[1], qo[0], qo[1], "none", np.int8)[0]
    assert L.mf_add_fma_form(float("inf"), 1.0, 0, 0, 1.0, 0, 0, 0, C.byref(k), C.byref(ok)) == _lib.MF_OK and ok.value == 0
    assert True in seen
