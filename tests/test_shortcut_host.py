"""Projection shortcuts without a GPU: models with a side operator (one Conv2D on a skip edge, read by one ADD) load -- ResNet-8 and
small blocks, both element types, the side convolution first and last in file order -- and report the side operator's source and the
ADD's skip; every form beside them is refused with the reference-style message and the reason; the writer's earlier blobs are byte for
byte what they were; and the host-side routing facts (tests/cpp/shortcut_route.cpp against the built library: the parser, group_splits,
side_join_candidate) say where the side convolution and its ADD form one launch and that no other group spans a side operator."""
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

I8, U8 = 9, 3
CSRC = os.path.join(ROOT, "microflow_rs_amd", "csrc")


def _check(m, layers):
    """every side operator and every ADD of the loaded model against the layer dicts"""
    import microflow_rs_amd as mf
    from microflow_rs_amd import _lib
    sides = 0
    for i, L in enumerate(layers):
        if "side_of" in L:
            sides += 1
            assert m.op(i)["kind"] == 3 and m.op_source(i) == L["side_of"]
        else:
            with pytest.raises(mf.MicroflowError) as ei:
                m.op_source(i)
            assert ei.value.status == _lib.MF_ERR_INVALID_ARG
        if L["op"] == "add":
            assert m.op_skip(i) == (L["skip"], 1 if L["swap"] else 0)
    return sides


@pytest.mark.parametrize("side", ["first", "last"])
@pytest.mark.parametrize("elem", [I8, U8], ids=["i8", "u8"])
def test_resnet8_and_small_projection_models_load(elem, side):
    """fails without the feature: the parent refuses every projection model at load"""
    import microflow_rs_amd as mf
    import tflite_writer as tw
    shape, in_q, layers = tw.resnet8_layers(np.random.default_rng(1), elem, side=side)
    assert shape == (1, 32, 32, 3) and [L["out_shape"][3] for L in layers[:12]] == [16] * 4 + [32] * 4 + [64] * 4
    m = mf.Model(tw.resnet8(np.random.default_rng(1), elem, side=side))
    assert m.num_ops == 16 and [o["kind"] for o in m.ops] == [3, 3, 3, 0, 3, 3, 3, 0, 3, 3, 3, 0, 1, 22, 9, 25]
    assert _check(m, layers) == 2
    s1, s2 = (4, 8) if side == "first" else (6, 10)
    assert (m.op_source(s1), m.op_source(s2)) == (3, 7) and (m.op_skip(7)[0], m.op_skip(11)[0]) == (s1, s2) and m.op_skip(3) == (0, 0)
    for s in (s1, s2):   # a 1x1 stride-2 convolution whose input quantisation is T's: the ADD's output in front of the block
        d, t = m.op(s), m.op(m.op_source(s))
        assert (d["KH"], d["KW"], d["sh"], d["sw"]) == (1, 1, 2, 2) and (d["in_scale"], d["in_zp"]) == (t["out_scale"], t["out_zp"])
    # small blocks: the model input as T, a stride-1 widening block, two projection blocks back to back, the ADD written either way
    for blocks, swap in (([(2, 32)], ()), ([(1, 32)], (0,)), ([(2, 32), (2, 64)], (1,)), ([(1, 16), (2, 32), (1, 32)], ())):
        shape, in_q, layers = tw.resnet_like_layers(np.random.default_rng(7), (8, 8, 16), blocks, elem, swap=swap, side=side)
        m = mf.Model(tw.build_model(shape, in_q, layers, elem))
        assert _check(m, layers) == sum(1 for L in layers if "side_of" in L) >= 1


def test_identity_models_still_load_and_report_as_before():
    import microflow_rs_amd as mf
    import tflite_writer as tw
    shape, in_q, layers = tw.resnet_like_layers(np.random.default_rng(4), (8, 8, 16), 2, swap=(1,))
    m = mf.Model(tw.build_model(shape, in_q, layers, I8))
    assert [o["kind"] for o in m.ops] == [3, 3, 0, 3, 3, 0, 1, 22, 9, 25]
    assert m.op_skip(2) == (-1, 0) and m.op_skip(5) == (2, 1) and _check(m, layers) == 0
    blocks = [(64, 3, 1, 16), (64, 3, 1, 16), (96, 3, 2, 24), (96, 3, 1, 24)]
    m = mf.Model(tw.inverted_residual_net(np.random.default_rng(3), (8, 8, 16), blocks, residual=True))
    assert [m.op_skip(i)[0] for i in (3, 7, 14)] == [-1, 3, 10]


# ---- the forms that stay refused ----------------------------------------------------------------------------------------------------
def _refused_models():
    import tflite_writer as tw
    rng = np.random.default_rng(31)
    shp, S, S2 = (4, 4, 16), (1, 4, 4, 16), (1, 2, 2, 32)
    in_q, oq = (0.05, 3), (0.07, -5)

    def conv(q, n=16, k=3, s=1, shape=shp, **kw):
        return dict(tw._conv_layer(rng, shape, q, False, n, k, s, "same", "none"), **kw)

    def add(skip, **kw):
        return dict(dict(op="add", skip=skip, swap=False, act="none", out_shape=S2, out_q=oq), **kw)

    def main(q):   # the block's main chain: 4x4x16 -> 2x2x32
        a = conv(q, 32, 3, 2)
        return [a, conv(a["out_q"], 32, 3, 1, (2, 2, 32))]

    side = lambda q, of, **kw: conv(q, 32, 1, 2, side_of=of, **kw)
    c0 = conv(in_q)
    q0 = c0["out_q"]
    pool = dict(op="average_pool_2d", filter=(2, 2), padding="valid", strides=(2, 2), act="none", out_shape=(1, 2, 2, 16), out_q=q0, side_of=0)
    dw = dict(tw._conv_layer(rng, shp, q0, True, 16, 3, 2, "same", "none"), side_of=0)
    s_a = side(q0, 0)
    after = conv(s_a["out_q"], 32, 1, 1, (2, 2, 32))
    forms = {
        "a side operator that is not a Conv2D": [c0, pool] + main(q0) + [add(1, out_shape=(1, 2, 2, 16))],
        "a side operator that is not a Conv2D ": [c0, dw] + main(q0) + [add(1, out_shape=(1, 2, 2, 16))],
        # (the second operator on the edge reads the first one's output: written through the writer's side_of)
        "two or more operators on the skip edge": [c0, s_a, dict(after, side_of=1)] + main(q0) + [add(2)],
        "its output is read by something other than one ADD": [c0, s_a] + main(q0) + [add(1), conv(oq, 32, 3, 1, (2, 2, 32)), add(1)],
        "its output is never read": [c0, s_a] + main(q0),
        "its input is no tensor of the chain": [c0, dict(conv(q0, 32, 1, 2), detach_input=(1, 6, 6, 16))] + main(q0),
        "a side operator while another skip is alive": [c0, s_a, side(q0, 0)] + main(q0) + [add(1), add(2)],
    }
    return {k: tw.build_model(S, in_q, v, I8) for k, v in forms.items()}


REFUSED = ["a side operator that is not a Conv2D", "a side operator that is not a Conv2D ", "two or more operators on the skip edge",
           "its output is read by something other than one ADD", "its output is never read", "its input is no tensor of the chain",
           "a side operator while another skip is alive"]


@pytest.mark.parametrize("form", REFUSED)
def test_every_other_form_is_refused_with_the_reason(form):
    import microflow_rs_amd as mf
    from microflow_rs_amd import _lib
    blob = _refused_models()[form]
    with pytest.raises(mf.MicroflowError) as ei:
        mf.Model(blob)
    assert ei.value.status == _lib.MF_ERR_UNSUPPORTED, str(ei.value)
    assert "only linear operator chains are supported" in str(ei.value) and form.strip() in str(ei.value), str(ei.value)


def test_mixed_element_types_on_the_skip_edge_are_refused():
    """the side convolution's output (and so the ADD's operand) in the other element type"""
    import microflow_rs_amd as mf
    import tflite_writer as tw
    from microflow_rs_amd import _lib
    shape, in_q, layers = tw.resnet_like_layers(np.random.default_rng(32), (4, 4, 16), [(2, 32)], I8, head=0)
    assert "side_of" in layers[0]
    layers[0] = dict(layers[0], out_type=tw.UINT8)
    with pytest.raises(mf.MicroflowError) as ei:
        mf.Model(tw.build_model(shape, in_q, layers, I8))
    assert ei.value.status == _lib.MF_ERR_UNSUPPORTED, str(ei.value)
    assert "only linear operator chains are supported" in str(ei.value) and "mixed element types" in str(ei.value), str(ei.value)


def test_every_existing_generator_writes_the_bytes_it_wrote():
    """tests/golden/writer_blobs.json, untouched: the writer's new keys and arguments change nothing that was written before"""
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
    assert got == want, sorted(k for k in got if got.get(k) != want.get(k))
    # identity blocks by count: the layer dicts of the form with a block list
    a = tw.resnet_like(rng(4), (8, 8, 16), 2, swap=(1,))
    assert a == tw.resnet_like(rng(4), (8, 8, 16), [(1, 16), (1, 16)], swap=(1,))
    assert hashlib.sha256(a).hexdigest() == RESNET_LIKE_PARENT


# sha256 of resnet_like(rng(4), (8, 8, 16), 2, swap=(1,)) as the parent commit's writer gives it
RESNET_LIKE_PARENT = "7ec1445a30522b9b1c17dd20520c8da439b129385935b44d433ce924260fb2a1"


# ---- routing facts of the host ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def route(tmp_path_factory):
    lib = os.path.join(ROOT, "microflow_rs_amd", "libmicroflow_amd.so")
    cxx = shutil.which("g++") or shutil.which("c++")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    if not os.path.exists(lib) or not cxx or not os.path.exists(os.path.join(rocm_inc, "hip", "hip_runtime.h")):
        pytest.skip("no built library / host compiler / ROCm headers")
    tmp = tmp_path_factory.mktemp("shortcut_route")
    exe = str(tmp / "shortcut_route")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", rocm_inc, os.path.join(ROOT, "tests", "cpp", "shortcut_route.cpp"),
                           lib, "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])

    def run(blob):
        path = str(tmp / ("m%d.tflite" % len(os.listdir(str(tmp)))))
        with open(path, "wb") as f:
            f.write(blob)
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stdout + out.stderr
        facts = dict(side={}, add={}, span={})
        for l in out.stdout.splitlines():
            w = l.split()
            if w[0] == "side":
                facts["side"][int(w[1])] = int(w[2])
            elif w[0] == "add":
                facts["add"][int(w[1])] = tuple(int(v) for v in w[2:5])
            elif w[0] == "span":
                facts["span"][(int(w[1]), int(w[2]))] = w[3] == "1"
            elif w[0] == "forks":
                facts["forks"] = (int(w[1]), int(w[2]))
        return facts
    return run


@pytest.mark.parametrize("side", ["first", "last"])
def test_the_side_convolution_and_its_add_form_one_group_where_the_class_is_taken(route, side):
    import tflite_writer as tw
    f = route(tw.resnet8(np.random.default_rng(1), I8, side=side))
    s1, s2 = (4, 8) if side == "first" else (6, 10)
    assert f["side"] == {s1: 3, s2: 7}
    # (skip_src, the operator whose tensor stays in memory, the side operator grouped with the ADD)
    assert f["add"] == {3: (0, 0, -1), 7: (s1, 3, s1), 11: (s2, 7, s2)}
    # the fork buffers hold T (32x32x16 at most) and S, and the model input is no skip here
    assert f["forks"] == (32 * 32 * 16, 0)
    # no group spans a side operator's index, an ADD, or a tensor that has to stay in memory
    for (a, b), refused in f["span"].items():
        if any(a <= s <= b for s in (s1, s2)) or any(a <= k <= b for k in (3, 7, 11)):
            assert refused, (a, b)
    # T's producer may end a group, never stand inside one (operator 0: the identity block's T); spans clear of all of them are free
    assert f["span"][(0, 1)] and not f["span"][(0, 0)] and not f["span"][(1, 2)] and not f["span"][(12, 15)]


@pytest.mark.parametrize("form,grouped", [("plain", True), ("s1", True), ("wzp", False), ("c24", False), ("k3", False), ("u8", True), ("u8wzp", False)])
def test_the_group_forms_inside_the_class_only(route, form, grouped):
    import tflite_writer as tw
    rng = np.random.default_rng(41)
    elem = U8 if form.startswith("u8") else I8
    C = 24 if form == "c24" else 16
    blocks = [(1, 32)] if form == "s1" else [(2, 32)]
    shape, in_q, layers = tw.resnet_like_layers(rng, (8, 8, C), blocks, elem, head=0, side_wzp="conv" if form.endswith("wzp") else "none")
    s = [i for i, L in enumerate(layers) if "side_of" in L][0]
    if form == "k3":   # a 3x3 convolution on the skip edge loads, and runs two launches
        layers[s] = dict(tw._conv_layer(rng, (8, 8, C), in_q, False, 32, 3, 2, "same", "none", elem), side_of=-1)
    f = route(tw.build_model(shape, in_q, layers, elem))
    add = len(layers) - 1
    assert f["side"] == {s: -1} and f["add"][add] == (s, -1, s if grouped else -1)
    assert f["forks"] == (int(np.prod(layers[s]["out_shape"])), 1)   # S lives in a fork buffer; T is the model input
