"""CONCATENATION without a GPU: fire modules (a squeeze 1x1, two expands that read it, their join) and SqueezeNet load in both element
types and both file orders of the expands, and report the join's skip and the side operator's source; an identity-skip
concat(x, conv(x)) loads; every refused form gives its status and reason, and the forms refused before keep their messages;
mf_preprocess_concatenation is the two f32 divisions; the writer's earlier blobs are byte for byte what they were; the host-side
routing facts (tests/cpp/concat_route.cpp against the built library: the parser, group_splits, side_join_candidate) say where the
side convolution and its join form one launch; and the numpy restatement of the contract (tests/concat_ref.py) agrees with a scalar
restatement on all 256 bytes."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import concat_ref as CR
from tests.conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

I8, U8 = 9, 3
CSRC = os.path.join(ROOT, "microflow_rs_amd", "csrc")
CONV, CAT, MAXPOOL = 3, 2, 17


def _check(m, layers):
    """every side operator and every join of the loaded model against the layer dicts -> (side operators, joins)"""
    import microflow_rs_amd as mf
    from microflow_rs_amd import _lib
    sides = joins = 0
    for i, L in enumerate(layers):
        if "side_of" in L:
            sides += 1
            assert m.op(i)["kind"] == CONV and m.op_source(i) == L["side_of"]
        else:
            with pytest.raises(mf.MicroflowError) as ei:
                m.op_source(i)
            assert ei.value.status == _lib.MF_ERR_INVALID_ARG
        if L["op"] == "concatenation":
            joins += 1
            d = m.op(i)
            assert d["kind"] == CAT and d["name"] == "concatenation" and d["out_shape"] == tuple(L["out_shape"])
            assert m.op_skip(i) == (L["skip"], 1 if L["swap"] else 0)
            assert (d["n_c0"], d["n_c1"]) == (1, 1)
        elif L["op"] != "add":
            with pytest.raises(mf.MicroflowError) as ei:
                m.op_skip(i)
            assert ei.value.status == _lib.MF_ERR_INVALID_ARG
    return sides, joins


@pytest.mark.parametrize("order", ["13", "31"])
@pytest.mark.parametrize("elem", [I8, U8], ids=["i8", "u8"])
def test_fire_models_and_squeezenet_load(elem, order):
    """fails without the feature: the parent refuses every such file at load (`unsupported operator: 2`, or, where the walk meets
    the expand on the skip edge first, `side operator: its output is never read`)"""
    import microflow_rs_amd as mf
    import tflite_writer as tw
    shape, in_q, layers = tw.squeezenet_layers(np.random.default_rng(1), 32, 10, elem, order=order)
    m = mf.Model(tw.squeezenet(np.random.default_rng(1), 32, 10, elem, order=order))
    fire = [CONV, CONV, CONV, CAT]
    assert [o["kind"] for o in m.ops] == [CONV, MAXPOOL] + fire * 2 + [MAXPOOL] + fire * 2 + [MAXPOOL] + fire * 4 + [CONV, 1, 22, 25]
    assert shape == (1, 32, 32, 3) and m.num_ops == len(layers) == 40 and m.output_shape == (1, 10)
    assert _check(m, layers) == (8, 8)
    # the first fire: squeeze 2, expands 3 and 4, join 5.  The first expand in the file is the side operator, the join reads [e1, e3]
    assert m.op_source(3) == 2 and m.op_skip(5) == (3, 1 if order == "13" else 0)
    k_side, k_main = (1, 3) if order == "13" else (3, 1)
    assert (m.op(3)["KH"], m.op(4)["KH"]) == (k_side, k_main)
    assert m.op(5)["out_shape"] == (1, 7, 7, 128) and m.op(35)["out_shape"] == (1, 1, 1, 512)
    ca, cb = m.op_constants(5)[:2]
    assert ca[0] == np.float32(1.0) and cb[0] == np.float32(1.0)          # converter-written: every slice is a copy
    # single fires: stride 2, the join written either way, slices that requantise
    for fire_, kw in (((16, 64, 64, 2, order), {}), ((16, 32, 48, 1, order), dict(e1_first=False)), ((32, 16, 16, 1, order), dict(identity=(False, True))),
                      ((16, 16, 80, 2, order), dict(identity=(False, False), e1_first=False))):
        rng = np.random.default_rng(7)
        ls, out_shape, _ = tw.fire_layers(rng, (4, 4, 32), (0.05, 3 if elem == I8 else 131), fire_, elem=elem, **kw)
        m = mf.Model(tw.build_model((1, 4, 4, 32), (0.05, 3 if elem == I8 else 131), ls, elem))
        assert _check(m, ls) == (1, 1) and m.output_shape == (1,) + tuple(out_shape)
        assert m.op_skip(3) == (1, 1 if ((order == "13") == kw.get("e1_first", True)) else 0)


def test_an_identity_skip_concat_loads():
    import microflow_rs_amd as mf
    import tflite_writer as tw
    for elem in (I8, U8):
        m = mf.Model(tw.dense_net(np.random.default_rng(2), (5, 5, 8), (8, 16), elem, swap=(1,), head=4))
        assert [o["kind"] for o in m.ops] == [CONV, CAT, CONV, CAT, 1, 22, 9, 25]
        # block 0 reads the model input beside the convolution, block 1 the first join's output; x is input a unless swapped
        assert m.op_skip(1) == (-1, 1) and m.op_skip(3) == (1, 0)
        assert m.op(1)["out_shape"] == (1, 5, 5, 16) and m.op(3)["out_shape"] == (1, 5, 5, 32)
    # rank 2, the axis given as 1 and as -1
    for axis in (1, -1):
        layers = [tw._fc_layer(np.random.default_rng(3), 8, 8, (0.05, 3)), dict(op="concatenation", skip=-1, swap=True, axis=axis, out_shape=(1, 16), out_q=(0.05, 3))]
        m = mf.Model(tw.build_model((1, 8), (0.05, 3), layers, I8))
        assert m.op_skip(1) == (-1, 1) and m.output_shape == (1, 16)


# ---- the forms that are refused ------------------------------------------------------------------------------------------------------
def _refused_models():
    import tflite_writer as tw
    rng = np.random.default_rng(51)
    S, in_q = (1, 4, 4, 16), (0.05, 3)
    c0 = tw._conv_layer(rng, (4, 4, 16), in_q, False, 16, 3, 1, "same", "none")
    q0 = c0["out_q"]

    def cat(**kw):
        return dict(dict(op="concatenation", skip=-1, swap=False, axis=-1, out_shape=(1, 4, 4, 32), out_q=q0), **kw)

    fresh = dict(shape=S, q=in_q)
    forms = {
        "it needs exactly two inputs": [c0, cat(inputs=["cur"], out_shape=S)],
        "it needs exactly two inputs ": [c0, cat(inputs=["cur", -1, dict(fresh)], out_shape=(1, 4, 4, 48))],
        "an axis other than the last": [c0, cat(axis=1, out_shape=(1, 8, 4, 16))],
        "an axis other than the last ": [c0, cat(axis=-2, out_shape=(1, 4, 8, 16))],
        "a constant operand": [c0, cat(inputs=["cur", dict(fresh, data=np.zeros(S, np.int8))])],
        "per-channel quantisation on an operand": [c0, cat(inputs=["cur", dict(shape=S, q=([0.05] * 16, [3] * 16))])],
        "a fused activation": [c0, cat(act="relu")],
        "mixed element types": [c0, cat(inputs=["cur", dict(fresh, type=tw.UINT8)])],
        "both inputs are the same tensor": [c0, cat(inputs=["cur", "cur"])],
        "neither input is the running value": [c0, cat(inputs=[-1, dict(fresh)])],
        "the other input is no earlier tensor of the chain": [c0, cat(inputs=["cur", dict(fresh)])],
        "the inputs differ in another dimension than the axis": [dict(c0, strides=(2, 2), out_shape=(1, 2, 2, 16)), cat(out_shape=(1, 2, 2, 32))],
    }
    return {k: tw.build_model(S, in_q, v, I8) for k, v in forms.items()}


REFUSED = ["it needs exactly two inputs", "it needs exactly two inputs ", "an axis other than the last", "an axis other than the last ", "a constant operand",
           "per-channel quantisation on an operand", "a fused activation", "mixed element types", "both inputs are the same tensor",
           "neither input is the running value", "the other input is no earlier tensor of the chain",
           "the inputs differ in another dimension than the axis"]


@pytest.mark.parametrize("form", REFUSED)
def test_every_refused_form_gives_its_reason(form):
    import microflow_rs_amd as mf
    from microflow_rs_amd import _lib
    blob = _refused_models()[form]
    with pytest.raises(mf.MicroflowError) as ei:
        mf.Model(blob)
    assert ei.value.status == _lib.MF_ERR_UNSUPPORTED, str(ei.value)
    assert "unsupported operator: 2 (CONCATENATION: " + form.strip() + ")" in str(ei.value), str(ei.value)


def test_an_output_shape_that_is_not_the_inputs_joined_is_an_invalid_model():
    import microflow_rs_amd as mf
    import tflite_writer as tw
    from microflow_rs_amd import _lib
    rng = np.random.default_rng(52)
    c0 = tw._conv_layer(rng, (4, 4, 16), (0.05, 3), False, 16, 3, 1, "same", "none")
    for shape in ((1, 4, 4, 16), (1, 4, 4, 33), (1, 4, 5, 32)):
        layers = [c0, dict(op="concatenation", skip=-1, swap=False, out_shape=shape, out_q=c0["out_q"])]
        with pytest.raises(mf.MicroflowError) as ei:
            mf.Model(tw.build_model((1, 4, 4, 16), (0.05, 3), layers, I8))
        assert ei.value.status == _lib.MF_ERR_INVALID_MODEL and "not the two inputs joined" in str(ei.value), str(ei.value)


def test_two_skips_alive_at_once_stay_refused():
    """SqueezeNet's bypass variant: an ADD around a fire module"""
    import microflow_rs_amd as mf
    import tflite_writer as tw
    from microflow_rs_amd import _lib
    rng = np.random.default_rng(53)
    ls, _, q = tw.fire_layers(rng, (4, 4, 32), (0.05, 3), (16, 16, 16))
    ls.append(dict(op="add", skip=-1, swap=False, act="none", out_shape=(1, 4, 4, 32), out_q=q))
    with pytest.raises(mf.MicroflowError) as ei:
        mf.Model(tw.build_model((1, 4, 4, 32), (0.05, 3), ls, I8))
    assert ei.value.status == _lib.MF_ERR_UNSUPPORTED and "two skip tensors alive at once" in str(ei.value), str(ei.value)


def test_the_forms_refused_before_keep_their_messages():
    """DESIGN 4.20's and 4.21's refusals, read by their own tests: the same status and text with CONCATENATION in the parser"""
    import microflow_rs_amd as mf
    import tflite_writer as tw
    from microflow_rs_amd import _lib
    from tests.test_shortcut_host import REFUSED as OLD, _refused_models as old_models
    blobs = old_models()
    for form in OLD:
        with pytest.raises(mf.MicroflowError) as ei:
            mf.Model(blobs[form])
        assert ei.value.status == _lib.MF_ERR_UNSUPPORTED
        assert "only linear operator chains are supported" in str(ei.value) and form.strip() in str(ei.value), str(ei.value)
    # a side convolution whose output a CONCATENATION and another operator read: the old text, whichever join reads it
    rng = np.random.default_rng(54)
    ls, _, q = tw.fire_layers(rng, (4, 4, 32), (0.05, 3), (16, 16, 16))
    ls.append(dict(op="add", skip=1, swap=False, act="none", out_shape=(1, 4, 4, 32), out_q=q))
    with pytest.raises(mf.MicroflowError) as ei:
        mf.Model(tw.build_model((1, 4, 4, 32), (0.05, 3), ls, I8))
    assert ei.value.status == _lib.MF_ERR_UNSUPPORTED
    assert "only linear operator chains are supported" in str(ei.value) and "its output is read by something other than one ADD" in str(ei.value), str(ei.value)
    # ADD's own refusals
    c0 = tw._conv_layer(rng, (4, 4, 16), (0.05, 3), False, 16, 3, 1, "same", "none")
    layers = [c0, dict(op="add", inputs=["cur", "cur"], act="none", out_shape=(1, 4, 4, 16), out_q=c0["out_q"])]
    with pytest.raises(mf.MicroflowError) as ei:
        mf.Model(tw.build_model((1, 4, 4, 16), (0.05, 3), layers, I8))
    assert "unsupported operator: 0 (ADD: both inputs are the same tensor)" in str(ei.value), str(ei.value)


def test_preprocess_concatenation_is_the_two_f32_divisions():
    from microflow_rs_amd import ops
    rng = np.random.default_rng(55)
    for _ in range(200):
        sa, sb, so = (np.float32(v) for v in rng.uniform(1e-3, 2.0, 3))
        ca, cb = ops.preprocess_concatenation(sa, sb, so)
        assert (ca, cb) == (np.float32(sa / so), np.float32(sb / so)) == CR.constants(sa, sb, so)
    assert ops.preprocess_concatenation(0.25, 0.25, 0.25) == (np.float32(1.0), np.float32(1.0))


def test_the_operator_api_refuses_bad_scales_without_a_device():
    import ctypes as C
    import microflow_rs_amd as mf
    from microflow_rs_amd import _lib
    L = _lib.lib()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        for pos in range(3):
            s = [0.1, 0.1, 0.1]
            s[pos] = bad
            h = C.c_void_p()
            st = L.mf_concatenation_create(0, 4, 16, 16, s[0], 0, s[1], 0, s[2], 0, 1.0, 1.0, C.byref(h))
            assert st == _lib.MF_ERR_INVALID_ARG, (bad, pos, st)
    assert mf is not None and L.mf_op_input2_elems(None) == 0


def test_every_existing_generator_writes_the_bytes_it_wrote():
    """tests/golden/writer_blobs.json and the pinned hash of tests/test_shortcut_host.py, through that file's own check"""
    from tests.test_shortcut_host import test_every_existing_generator_writes_the_bytes_it_wrote as check
    check()


# ---- the numpy form against a second restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
def test_the_numpy_form_equals_a_scalar_restatement_on_all_256_bytes(u8):
    dt = np.uint8 if u8 else np.int8
    x = np.arange(256).astype(np.uint8).view(dt) if not u8 else np.arange(256, dtype=np.uint8)
    off = 128 if u8 else 0
    inexact = np.float32(np.float32(0.0371) / np.float32(0.0523))
    ties = lo_hit = hi_hit = 0
    for c in (np.float32(1.0), np.float32(0.5), np.float32(1.5), inexact):
        for z, zo in ((0 + off, 0 + off), (-7 + off, 12 + off), (20 + off, -20 + off)):
            got = CR.requant(x, c, z, (1.0, zo))
            want = np.array([CR.requant_scalar(int(v), float(c), z, zo, u8) for v in x], np.int32)
            assert np.array_equal(got, want), (c, z, zo)
            if c == 1.0 and z == zo:
                assert np.array_equal(got, x.astype(np.int32))                 # the identity: y = x for every byte
            d = x.astype(np.int64) - z
            if c in (0.5, 1.5):
                ties += int(np.count_nonzero(d % 2))                           # c d ends in .5 for every odd d
            lo_hit += int(np.count_nonzero(got == (0 if u8 else -128)))
            hi_hit += int(np.count_nonzero(got == (255 if u8 else 127)))
    assert ties > 0 and lo_hit > 1 and hi_hit > 1
    # a tie of y = zo + c d is rounded away from zero: i8 with zo = 0 gives 1.5 -> 2 and -1.5 -> -2, u8 with zo = 128 gives
    # 129.5 -> 130 and 126.5 -> 127
    z = off
    three = np.array([3 + off, -3 + off]).astype(dt)
    assert list(CR.requant(three, np.float32(0.5), z, (1.0, z))) == ([130, 127] if u8 else [2, -2])
    # the join itself: rows of a followed by rows of b
    a = np.arange(2 * 3 * 4).reshape(2, 3, 4).astype(dt)
    b = (100 + np.arange(2 * 3 * 2)).reshape(2, 3, 2).astype(dt)
    y = CR.concat(a, b, (0.5, z), (0.5, z), (0.5, z))
    assert y.shape == (2, 3, 6) and np.array_equal(y[..., :4], a) and np.array_equal(y[..., 4:], b)


# ---- routing facts of the host ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def route(tmp_path_factory):
    lib = os.path.join(ROOT, "microflow_rs_amd", "libmicroflow_amd.so")
    cxx = shutil.which("g++") or shutil.which("c++")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    if not os.path.exists(lib) or not cxx or not os.path.exists(os.path.join(rocm_inc, "hip", "hip_runtime.h")):
        pytest.skip("no built library / host compiler / ROCm headers")
    tmp = tmp_path_factory.mktemp("concat_route")
    exe = str(tmp / "concat_route")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", rocm_inc, os.path.join(ROOT, "tests", "cpp", "concat_route.cpp"),
                           lib, "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])

    def run(blob):
        path = str(tmp / ("m%d.tflite" % len(os.listdir(str(tmp)))))
        with open(path, "wb") as f:
            f.write(blob)
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stdout + out.stderr
        facts = dict(side={}, join={}, span={})
        for l in out.stdout.splitlines():
            w = l.split()
            if w[0] == "side":
                facts["side"][int(w[1])] = int(w[2])
            elif w[0] == "join":
                facts["join"][int(w[1])] = tuple(int(v) for v in w[2:7])
            elif w[0] == "span":
                facts["span"][(int(w[1]), int(w[2]))] = w[3] == "1"
            elif w[0] == "forks":
                facts["forks"] = tuple(int(v) for v in w[1:4])
        return facts
    return run


@pytest.mark.parametrize("order", ["13", "31"])
def test_squeezenet_groups_every_1x1_side_expand_with_its_join(route, order):
    import tflite_writer as tw
    shape, in_q, layers = tw.squeezenet_layers(np.random.default_rng(1), 32, 10, I8, order=order)
    f = route(tw.build_model(shape, in_q, layers, I8))
    joins = [i for i, L in enumerate(layers) if L["op"] == "concatenation"]
    sides = [i for i, L in enumerate(layers) if "side_of" in L]
    assert f["side"] == {s: s - 1 for s in sides} and sorted(f["join"]) == joins
    for j in joins:   # (kind, skip_src, the operator whose tensor stays in memory -- the squeeze --, the grouped side operator, elements)
        kind, src, real, cand, elems = f["join"][j]
        assert (kind, src, real) == (CAT, j - 2, j - 3) and elems == int(np.prod(layers[j]["out_shape"]))
        assert cand == (j - 2 if order == "13" else -1)   # a 3x3 side convolution runs two launches
    # no group spans a join, a side operator's index or a tensor that has to stay in memory (the squeeze may end a group)
    for (a, b), refused in f["span"].items():
        if any(a <= s <= b for s in sides) or any(a <= j <= b for j in joins) or any(a <= j - 3 < b for j in joins):
            assert refused, (a, b)
    assert not f["span"][(0, 1)] and f["span"][(2, 3)] and not f["span"][(36, 39)] and not f["span"][(1, 2)]
    # the fork buffers hold T and S; the activation buffers the joined tensor
    fork, input_skip, max_elems = f["forks"]
    assert input_skip == 0
    assert fork == max(max(int(np.prod(layers[s]["out_shape"])) for s in sides), max(int(np.prod(layers[s - 1]["out_shape"])) for s in sides))
    assert max_elems >= max(f["join"][j][4] for j in joins)


FORMS = {"plain": ((16, 32, 48), {}, True), "s2": ((16, 32, 48, 2), {}, True), "e3-first": ((16, 32, 48), dict(e1_first=False), True),
         "requant": ((16, 32, 48), dict(identity=(False, False)), True), "u8": ((16, 32, 48), {}, True),
         "wzp": ((16, 32, 48), dict(side_wzp="conv"), False), "u8wzp": ((16, 32, 48), dict(side_wzp="conv"), False),
         "c24": ((24, 32, 48), {}, False), "cb24": ((16, 32, 24), {}, False), "n24": ((16, 24, 48), {}, False),
         "k3": ((16, 32, 48, 1, "31"), {}, False), "c272": ((272, 32, 48), {}, False)}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_the_group_forms_inside_the_class_only(route, form):
    import tflite_writer as tw
    fire, kw, grouped = FORMS[form]
    elem = U8 if form.startswith("u8") else I8
    ls, out_shape, _ = tw.fire_layers(np.random.default_rng(41), (4, 4, 32), (0.05, 3 if elem == I8 else 131), fire, elem=elem, **kw)
    f = route(tw.build_model((1, 4, 4, 32), (0.05, 3 if elem == I8 else 131), ls, elem))
    assert f["side"] == {1: 0}
    assert f["join"][3] == (CAT, 1, 0, 1 if grouped else -1, int(np.prod(out_shape)))
    t, s = int(np.prod(ls[0]["out_shape"])), int(np.prod(ls[1]["out_shape"]))
    assert f["forks"][:2] == (max(t, s), 0) and f["forks"][2] >= int(np.prod(out_shape))


def test_the_fork_buffers_cover_a_joined_tensor_that_is_the_next_skip(route):
    """concat(x1, g(x1)) with x1 = concat(x0, f(x0)): the first join's output stays in memory for the second"""
    import tflite_writer as tw
    f = route(tw.dense_net(np.random.default_rng(2), (5, 5, 8), (8, 16), I8, head=4))
    assert f["join"] == {1: (CAT, -1, -1, -1, 5 * 5 * 16), 3: (CAT, 1, 1, -1, 5 * 5 * 32)}
    assert f["forks"] == (5 * 5 * 16, 1, 5 * 5 * 32)
    assert f["span"][(0, 1)] and f["span"][(1, 2)] and not f["span"][(2, 2)] and not f["span"][(4, 7)]
