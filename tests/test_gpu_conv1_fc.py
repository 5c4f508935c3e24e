"""A one-channel convolution -> Reshape -> FullyConnected (-> Softmax) as one conv1_fc_rt launch (k_conv1_fc.hip): routing, launch
count, bit-exactness against the CPU oracle every way the model can be run, the bytes around the output, graph replay, predict, and
the models that must keep today's launches (speech.tflite's geometry among them).  The cases: tests/conv1_fc_cases.py."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests.conftest import ROOT, ROUTING_SWITCHED, model_path
from tests.conv1_fc_cases import CASES, build, out_hw

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))

FUSED = "(fused"
BATCHES = (1, 15, 16, 17, 77)          # one image; one short of a step, a step, one more; four steps and a ragged fifth
LABEL = "conv1_fc_rt<"


class Kws:
    """one case: the model, its oracle, BATCHES[-1] random images (image 0 all-minimum, image 1 all-maximum) and the oracle's outputs
    for images 0, 1, the middle one and the last, computed once"""

    def __init__(self, O, name):
        import microflow_rs_amd as mf
        self.name = name
        self.shape, self.stem, self.classes, self.u8, _, self.softmax, _ = CASES[name]
        self.blob = build(name)
        self.m = mf.Model(self.blob)
        self.m.prepare(1)
        self.om = O.Model(self.blob)
        self.lo, self.hi = (0, 256) if self.m.dtype == np.uint8 else (-128, 128)
        n = BATCHES[-1]
        rng = np.random.default_rng(17 + ord(name))
        self.x = rng.integers(self.lo, self.hi, (n, self.m.input_elems), dtype=np.int16).astype(self.m.dtype)
        self.x[0], self.x[1] = self.lo, self.hi - 1
        self.picks = [0, 1, n // 2, n - 1]
        self.want = self.om.run_quantized_batch(self.x[self.picks]).reshape(len(self.picks), -1)
        self.N = self.want.shape[1]
        self.conv = [i for i in range(self.m.num_ops) if self.m.op(i)["kernel"] != ""][0]  # (no Reshape in front: operator 0)

    def layerwise(self, x):
        """fusion off: every operator's own launch"""
        self.m.set_fusion(False)
        try:
            return self.m.run_quantized(x).reshape(len(x), -1)
        finally:
            self.m.set_fusion(True)


_models = {}


@pytest.fixture(params=sorted(CASES))
def kws(request, O):
    if request.param not in _models:
        _models[request.param] = Kws(O, request.param)
    return _models[request.param]


def test_the_model_is_one_conv1_fc_rt_launch(kws):
    """the convolution reports the group, every operator behind it "fused"; one run_quantized of an int8 model enqueues one launch;
    fusion off shows the operators' own kernels"""
    import torch
    m = kws.m
    if not ROUTING_SWITCHED:
        names = [m.op(i)["kernel"] for i in range(m.num_ops)]
        kind, N, KH, KW, _, _ = kws.stem
        want0 = "%s%s,%dx%d,%d>%s" % (LABEL, kind, KH, KW, N, "+sm" if kws.softmax else "")
        assert names[kws.conv] == want0, names
        assert all(n == "" or n.startswith(FUSED) for n in names[kws.conv + 1:]), names
        assert m.op_epilogue_mode(kws.conv) in (0, 1, 2)
        if not kws.u8:
            x = torch.as_tensor(kws.x[:17]).cuda()
            out = torch.empty((17, kws.N), dtype=torch.int8, device="cuda")
            m.run_quantized(x, out=out)
            before = m.device_ops()
            m.run_quantized(x, out=out)
            assert m.device_ops() - before == 1
        m.set_fusion(False)
        try:
            off = [m.op(i)["kernel"] for i in range(m.num_ops)]
            assert not any(n.startswith(LABEL) or n.startswith(FUSED) for n in off), off
        finally:
            m.set_fusion(True)


def test_every_image_equals_layerwise_and_generic_and_the_oracle(kws):
    m = kws.m
    full = kws.layerwise(kws.x)
    assert np.array_equal(full[kws.picks], kws.want), kws.name
    m.set_generic(True)
    try:
        assert np.array_equal(m.run_quantized(kws.x).reshape(len(kws.x), -1), full)
    finally:
        m.set_generic(False)
    for n in BATCHES:
        got = m.run_quantized(kws.x[:n]).reshape(n, -1)
        bad = np.flatnonzero((got != full[:n]).any(axis=1))
        assert bad.size == 0, (kws.name, n, bad[:8], got[bad[:2]], full[bad[:2]])
    got = m.run_quantized(kws.x).reshape(len(kws.x), -1)
    assert np.array_equal(got[kws.picks], kws.want)


def test_run_until_the_convolution_equals_the_oracles_layer(kws):
    """a run that ends inside the group uses the operators' own launches"""
    m = kws.m
    for k in (0, 1, 5):
        _, layers = kws.om.run_quantized(kws.x[k], layers=True)
        for i in range(m.num_ops):
            got = np.asarray(m.run_until(kws.x[k:k + 1], i)).reshape(-1)
            assert np.array_equal(got, layers[i].reshape(-1)), (kws.name, k, i)


@pytest.mark.parametrize("name,n", [("a", 8209), ("a", 4089), ("e", 8209)])
def test_many_steps_per_workgroup_and_a_ragged_last_step(O, name, n):
    """8209 images: more steps than workgroups, and nine images in the last one.  Case e takes any batch in one launch; case a, whose
    FullyConnected has a launch of its own, takes up to 4096 in one launch (4089: 256 steps, nine images in the last) and the
    operators' launches beyond: the same bytes either way"""
    if name not in _models:
        _models[name] = Kws(O, name)
    k = _models[name]
    x = np.random.default_rng(3).integers(-128, 128, (n, k.m.input_elems)).astype(np.int8)
    got = k.m.run_quantized(x).reshape(n, -1)
    want = k.layerwise(x)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:8])
    assert np.array_equal(got[:3], k.om.run_quantized_batch(x[:3]).reshape(3, -1))


def test_bytes_around_the_output_stay(kws):
    """the output inside a larger device buffer filled with a sentinel, at a 16-byte-aligned offset and at an odd one: exactly
    batch x N bytes change"""
    import torch
    m = kws.m
    dt = torch.uint8 if m.dtype == np.uint8 else torch.int8
    for n in (17, 77):
        x = torch.as_tensor(kws.x[:n]).cuda()
        want = kws.layerwise(kws.x[:n])
        for off in (32, 3):
            buf = torch.full((off + n * kws.N + 4096,), 0x5A, dtype=dt, device="cuda")
            m.run_quantized(x, out=buf[off:off + n * kws.N])
            b = buf.cpu().numpy()
            assert (b[:off] == 0x5A).all() and (b[off + n * kws.N:] == 0x5A).all(), (kws.name, n, off)
            assert np.array_equal(b[off:off + n * kws.N].reshape(n, -1), want), (kws.name, n, off)


def test_input_view_offset_by_one_byte(kws):
    """a device input that is not 16-byte aligned: same bytes (conv1_fc_rt loads 16-byte words and is not given such a pointer)"""
    import torch
    m = kws.m
    n = 17
    flat = kws.x[:n].reshape(-1)
    buf = torch.zeros(flat.size + 64, dtype=torch.uint8 if m.dtype == np.uint8 else torch.int8, device="cuda")
    view = buf[1:1 + flat.size]
    view.copy_(torch.as_tensor(flat))
    assert view.data_ptr() % 16 == 1
    got = m.run_quantized(view).cpu().numpy().reshape(n, -1)
    assert np.array_equal(got, kws.layerwise(kws.x[:n]))


def test_graph_replays_give_the_same_bytes(kws):
    import torch
    m = kws.m
    x = torch.as_tensor(kws.x).cuda()
    ref = m.run_quantized(x).clone()
    assert np.array_equal(ref.cpu().numpy().reshape(len(kws.x), -1)[kws.picks], kws.want)
    m.set_graph(True)
    try:
        out = torch.empty_like(ref)
        before = m.graph_launches
        for it in range(4):                            # eager, captured + replayed, replayed, replayed
            out.zero_()
            m.run_quantized(x, out=out)
            assert torch.equal(out, ref), it
        assert m.graph_launches >= before + 2
    finally:
        m.set_graph(False)


def test_predict_gives_the_oracles_floats(kws):
    """the f32 boundaries stay outside this launch: M::predict's floats, bit for bit, on five images"""
    m = kws.m
    rng = np.random.default_rng(23)
    q = rng.integers(kws.lo, kws.hi, (5, m.input_elems)).astype(np.float32)
    x = ((q - np.float32(m.input_zero_point)) * np.float32(m.input_scale) + rng.uniform(-0.4, 0.4, q.shape).astype(np.float32) * np.float32(m.input_scale)).astype(np.float32)
    want = np.stack([kws.om.predict(x[i].reshape(m.input_shape)).reshape(-1) for i in range(5)]).astype(np.float32)
    got = np.asarray(m.predict(x.reshape((5,) + tuple(m.input_shape)))).reshape(5, -1).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), kws.name


# ---- what must not move ------------------------------------------------------------------------------------------------------
def _kept(name):
    """a model outside the group, by the reason conv1_fc_plan (or the peephole) refuses it"""
    import tflite_writer as tw
    rng = np.random.default_rng(31)
    dw = lambda n, kh, kw, s=(1, 1), p="same": ("dw", n, kh, kw, s, p)  # noqa: E731
    return {
        "speech_like": lambda: tw.speech_like(rng),
        "speech_like-u8-wzp": lambda: tw.speech_like(rng, elem=tw.UINT8, fc_wzp=9),
        "W-not-whole-dwords": lambda: tw.kws_like(rng, (12, 10), dw(8, 3, 3), 6),
        "six-filters": lambda: tw.kws_like(rng, (12, 8), ("conv", 6, 3, 3, (1, 1), "same"), 6),
        "filter-17-wide": lambda: tw.kws_like(rng, (6, 20), ("conv", 4, 2, 17, (1, 1), "same"), 6),
        "65-classes": lambda: tw.kws_like(rng, (8, 8), dw(8, 3, 3), 65),
        "tiles-exceed-lds": lambda: tw.kws_like(rng, (200, 64), ("conv", 4, 3, 3, (2, 2), "same"), 6),
        "filter-zero-points": lambda: tw.kws_like(rng, (10, 8), ("conv", 8, 3, 3, (1, 1), "same"), 6, stem_wzp=True),
    }[name]()


@pytest.mark.parametrize("name", ["speech_like", "speech_like-u8-wzp", "W-not-whole-dwords", "six-filters", "filter-17-wide", "65-classes",
                                  "tiles-exceed-lds", "filter-zero-points"])
def test_models_outside_the_group_keep_their_launches(O, name):
    import microflow_rs_amd as mf
    blob = _kept(name)
    m = mf.Model(blob)
    m.prepare(1)
    names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    if not ROUTING_SWITCHED:
        assert not any(n.startswith(LABEL) for n in names), names
        if name.startswith("speech_like"):
            assert names[1].startswith("dwc1_fc_softmax") and all(n.startswith(FUSED) for n in names[2:]), names
    lo, hi = (0, 256) if m.dtype == np.uint8 else (-128, 128)
    n = 19 if name == "tiles-exceed-lds" else 77
    x = np.random.default_rng(8).integers(lo, hi, (n, m.input_elems), dtype=np.int16).astype(m.dtype)
    x[0], x[1] = lo, hi - 1
    assert np.array_equal(m.run_quantized(x).reshape(n, -1), O.Model(blob).run_quantized_batch(x).reshape(n, -1))


def test_speech_keeps_its_kernel():
    import microflow_rs_amd as mf
    if ROUTING_SWITCHED:
        return
    sp = mf.Model(model_path("speech"))
    sp.prepare(1)
    names = [sp.op(i)["kernel"] for i in range(sp.num_ops)]
    assert names[1].startswith("dwc1_fc_softmax") and all(n.startswith(FUSED) for n in names[2:]), names


def test_no_conv1_fc_switch_goes_back_to_todays_launches():
    """MF_DEV=1 MF_NO_CONV1_FC=1 (a child process: the switches are read once per process): the operators' own launches and the
    FullyConnected + Softmax groups as before this kernel, with the same bytes as conv1_fc_rt in the other child; and speech_like
    under MF_NO_DWFC keeps dw_c1_lds + fc_rowwave_softmax<4> whatever this switch says"""
    code = r'''
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import microflow_rs_amd as mf
import tflite_writer as tw
from tests.conv1_fc_cases import build
outs = []
for name in ("a", "c"):
    m = mf.Model(build(name))
    m.prepare(1)
    x = np.random.default_rng(6).integers(-128, 128, (77, m.input_elems)).astype(np.int8)
    print("KERNELS", name, "|".join(m.op(i)["kernel"] for i in range(m.num_ops)))
    outs.append(m.run_quantized(x).reshape(-1))
sp = mf.Model(tw.speech_like(np.random.default_rng(2)))
sp.prepare(1)
print("KERNELS", "speech_like", "|".join(sp.op(i)["kernel"] for i in range(sp.num_ops)))
np.save(sys.argv[1], np.concatenate(outs))
''' % (ROOT, os.path.join(ROOT, "tools"))
    outs, kernels = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for sw in ({}, dict(MF_DEV="1", MF_NO_CONV1_FC="1"), dict(MF_DEV="1", MF_NO_DWFC="1")):
            env = dict(os.environ)
            for k in [k for k in env if k.startswith("MF_")]:
                del env[k]
            env.update(sw)
            path = os.path.join(tmp, "out%d.npy" % len(outs))
            r = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
            assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
            kernels.append({l.split()[1]: l.split(" ", 2)[2].split("|") for l in r.stdout.splitlines() if l.startswith("KERNELS")})
            outs.append(np.load(path))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    on, off, nodwfc = kernels
    assert on["a"][0] == "conv1_fc_rt<dw,3x3,8>+sm" and on["c"][0] == "conv1_fc_rt<conv,5x2,12>+sm", on
    assert off["a"][0].endswith("_lds") and "fc_rowwave_softmax<4>" in off["a"] and off["a"][-1].startswith(FUSED), off
    assert off["c"][0].endswith("_lds") and off["c"][1:] == ["", "fc_rt", "softmax_table"], off
    assert on["speech_like"][1].startswith("dwc1_fc_softmax") and off["speech_like"] == on["speech_like"], (on, off)
    assert "dw_c1_lds" in nodwfc["speech_like"] and "fc_rowwave_softmax<4>" in nodwfc["speech_like"], nodwfc
    assert nodwfc["a"] == on["a"], nodwfc
