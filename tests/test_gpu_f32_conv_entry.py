"""M::predict on models whose first operator is a Conv2D (or a one-channel DepthwiseConv2D) on a 1- to 4-channel image.  Where
conv_rows_lds walks one image per step the boundary quantisation runs inside conv_rows_lds_f32, the model's first launch; with several
small images per step, and on conv_gemm_rt, the separate pass measured faster and stays: those models are here with their
unchanged launch counts.  The floats of the CPU oracle's
predict bit for bit -- at half-way points, zeros, denormals, saturation, infinities and NaN --, the same floats with fusion off and on
the shape-generic kernels, the number of launches (mf_model_device_ops), an input that is not 16-byte aligned, the floats around the
output, overlapping buffers, graph replay, the host-fed path and the dev switch that brings the separate pass back.

The shapes are the smallest at which each staging path can go wrong; the images per step (G) that the batches are ragged against
are checked against conv_rows_plan in tests/test_f32_conv_entry_host.py."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests.conftest import ROOT, ROUTING_SWITCHED

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))


def _stem_head(rng, shape, stem, head=10, elem=None):
    """one stem layer given in full (what conv_net cannot express: VALID padding, a depth multiplier, a non-square filter), a 1x1
    Conv2D to 16 channels and conv_net's head: AveragePool over the whole image, FullyConnected(head), Softmax"""
    import tflite_writer as tw
    elem = tw.INT8 if elem is None else elem
    lo, hi = (0, 256) if elem == tw.UINT8 else (-128, 128)
    mid = (lo + hi) // 2
    H, W, C = shape
    in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, hi - 20)))
    dw, n, kh, kw, s, pad = stem
    oh, ow = (-(-H // s), -(-W // s)) if pad == "same" else ((H - kh) // s + 1, (W - kw) // s + 1)
    sc = rng.uniform(0.002, 0.01, n).astype(np.float32)
    taps = kh * kw * (1 if dw else C)
    q = (float(np.float32(in_q[0] * float(sc.mean()) * 60.0 * np.sqrt(taps))), lo)
    d = dict(op="depthwise_conv_2d" if dw else "conv_2d", fscale=sc, fzp=np.full(n, mid), bias=rng.integers(-500, 500, n),
             bscale=(sc * np.float32(in_q[0])).astype(np.float32), bzp=np.zeros(n, np.int64), padding=pad, strides=(s, s), act="relu6",
             out_shape=(1, oh, ow, n), out_q=q)
    if dw:
        d["weights"], d["depth_multiplier"] = rng.integers(lo, hi, (1, kh, kw, n)), n // C
    else:
        d["filters"] = rng.integers(lo, hi, (n, kh, kw, C))
    # a 1x1 Conv2D to 16 channels: the width from which the head is one launch that stores the floats (pool_fc_chain)
    sc1 = rng.uniform(0.002, 0.01, 16).astype(np.float32)
    q1 = (float(np.float32(q[0] * float(sc1.mean()) * 60.0 * np.sqrt(n))), lo)
    pw = dict(op="conv_2d", filters=rng.integers(lo, hi, (16, 1, 1, n)), fscale=sc1, fzp=np.full(16, mid), bias=rng.integers(-500, 500, 16),
              bscale=(sc1 * np.float32(q[0])).astype(np.float32), bzp=np.zeros(16, np.int64), padding="same", strides=(1, 1), act="relu6",
              out_shape=(1, oh, ow, 16), out_q=q1)
    q, n = q1, 16
    layers = [d, pw, dict(op="average_pool_2d", filter=(oh, ow), padding="valid", strides=(oh, ow), act="none", out_shape=(1, 1, 1, n), out_q=q),
              dict(op="reshape", out_shape=(1, n), out_q=q)]
    wsc = np.float32(rng.uniform(0.002, 0.02))
    osc = float(np.float32(q[0] * wsc * 60.0 * np.sqrt(n)))
    layers.append(dict(op="fully_connected", weights=rng.integers(lo, hi, (head, n)), wscale=[wsc], wzp=[mid], bias=rng.integers(-2000, 2000, head),
                       bscale=[np.float32(q[0]) * wsc], bzp=[0], act="none", out_shape=(1, head), out_q=(osc, int(rng.integers(lo + 20, hi - 20)))))
    layers.append(dict(op="softmax", out_shape=(1, head), out_q=(1.0 / 256.0, lo)))
    return tw.build_model((1, H, W, C), in_q, layers, elem)


# name -> (builder, kernel of operator 0, batches)
def _models():
    import tflite_writer as tw
    r = lambda: np.random.default_rng(73)  # noqa: E731
    return {
        # conv_rows_lds (G images per step from conv_rows_plan: 8, 6, 1, 8)
        "rows-12x12x3-s2-16": (lambda: tw.conv_net(r(), (12, 12, 3), [("conv", 16, 3, 2)], head=10), "conv_rows_lds", (1, 77)),  # 36-byte rows
        "rows-40x40x3-s1-8": (lambda: tw.conv_net(r(), (40, 40, 3), [("conv", 8, 3, 1), ("conv", 16, 1, 1)], head=10), "conv_rows_lds", (1, 77)),
        "rows-80x80x3-s2-16": (lambda: tw.conv_net(r(), (80, 80, 3), [("conv", 16, 3, 2)], head=10), "conv_rows_lds", (1, 77, 2053)),
        "rows-28x28x1-5x5valid-6": (lambda: _stem_head(r(), (28, 28, 1), (False, 6, 5, 5, 1, "valid")), "conv_rows_lds", (1, 77)),  # shy = 0
        "rows-10x10x2-12-u8-wzp": (lambda: tw.conv_net(r(), (10, 10, 2), [("conv", 12, 3, 1), ("conv", 16, 1, 1)], elem=tw.UINT8, wzp_nonzero=True, head=10),
                                   "conv_rows_lds<wzp>", (1, 77)),                                                       # N % 8 != 0 byte stores
        "dwrows-20x12x1-4x3-12": (lambda: _stem_head(r(), (20, 12, 1), (True, 12, 4, 3, 1, "same")), "dw_rows_lds", (1, 77)),
        # ... and with one image per step (4 097 .. 8 192 dwords of image), where the first launch takes the floats: the u8 element type
        # with filter zero points off the middle, 228-byte rows and N % 8 != 0 byte stores; the one-channel depthwise with a depth
        # multiplier; VALID padding (shy = 0) with N % 8 != 0
        "rows-76x76x3-12-u8-wzp-g1": (lambda: tw.conv_net(r(), (76, 76, 3), [("conv", 12, 3, 1), ("conv", 16, 1, 1)], elem=tw.UINT8, wzp_nonzero=True, head=10),
                                      "conv_rows_lds<wzp>", (1, 77)),
        "dwrows-136x128x1-4x3-12-g1": (lambda: _stem_head(r(), (136, 128, 1), (True, 12, 4, 3, 1, "same")), "dw_rows_lds", (1, 77)),
        "rows-144x128x1-5x5valid-6-g1": (lambda: _stem_head(r(), (144, 128, 1), (False, 6, 5, 5, 1, "valid")), "conv_rows_lds", (1, 77)),
        # conv_gemm_rt
        "gemm-16x16x3-80": (lambda: tw.conv_net(r(), (16, 16, 3), [("conv", 80, 3, 1)], head=10), "conv_gemm_rt", (1, 77)),  # AL 1; 48-byte rows
        "gemm-10x10x2-72": (lambda: tw.conv_net(r(), (10, 10, 2), [("conv", 72, 3, 1), ("conv", 16, 1, 1)], head=10), "conv_gemm_rt", (1, 77)),        # 20-byte rows
        "gemm-16x16x4-96": (lambda: tw.conv_net(r(), (16, 16, 4), [("conv", 96, 3, 1)], head=10), "conv_gemm_rt", (1, 77)),        # AL 4
        "gemm-128x128x3-s2-16": (lambda: tw.conv_net(r(), (128, 128, 3), [("conv", 16, 3, 2)], head=10), "conv_gemm_rt", (1, 77)),  # past conv_rows_plan
        "gemm-128x128x3-s1-16": (lambda: tw.conv_net(r(), (128, 128, 3), [("conv", 16, 3, 1)], head=10), "conv_gemm_rt", (1, 5)),   # row bands
        "gemm-10x10x2-72-u8-wzp": (lambda: tw.conv_net(r(), (10, 10, 2), [("conv", 72, 3, 1), ("conv", 16, 1, 1)], elem=tw.UINT8, wzp_nonzero=True, head=10),
                                   "conv_gemm_rt<wzp>", (1, 77)),
        # 40 column tiles of 4 k steps: three weight slices
        "gemm-8x8x4-7x7-640-sliced": (lambda: tw.conv_net(r(), (8, 8, 4), [("conv", 640, 7, 1)], head=10), "conv_gemm_rt", (1, 77)),
    }


MODELS = ["rows-12x12x3-s2-16", "rows-40x40x3-s1-8", "rows-80x80x3-s2-16", "rows-28x28x1-5x5valid-6", "rows-10x10x2-12-u8-wzp", "dwrows-20x12x1-4x3-12",
          "rows-76x76x3-12-u8-wzp-g1", "dwrows-136x128x1-4x3-12-g1", "rows-144x128x1-5x5valid-6-g1",
          "gemm-16x16x3-80", "gemm-10x10x2-72", "gemm-16x16x4-96", "gemm-128x128x3-s2-16", "gemm-128x128x3-s1-16", "gemm-10x10x2-72-u8-wzp",
          "gemm-8x8x4-7x7-640-sliced"]
U8 = ["rows-10x10x2-12-u8-wzp", "gemm-10x10x2-72-u8-wzp", "rows-76x76x3-12-u8-wzp-g1"]
# conv_rows_lds with G = 1: the floats are the first launch's input
ENTRY = ["rows-80x80x3-s2-16", "rows-76x76x3-12-u8-wzp-g1", "dwrows-136x128x1-4x3-12-g1", "rows-144x128x1-5x5valid-6-g1"]


def _inputs(om, n, seed):
    """tests/test_gpu_f32_boundary.py's generator: n f32 images (q - zp) * scale over random q of the element type, with the hard values
    planted in every image: half-way points (k + 0.5 - zp) * scale incl. the two that decide saturation, +-0, denormals, values far
    beyond both ends, +-inf, NaN"""
    rng = np.random.default_rng(seed)
    lo, hi = (0, 256) if om.dtype == np.uint8 else (-128, 128)
    sc, zp, E = np.float32(om.in_scale), om.in_zp, om.in_elems
    q = rng.integers(lo, hi, (n, E))
    x = ((q - zp).astype(np.float32) * sc).astype(np.float32)
    ks = np.array([lo - 1, lo, lo + 1, zp - 1, zp, hi - 2, hi - 1] + list(rng.integers(lo, hi, 9)), np.float64)
    half = ((ks + 0.5 - zp).astype(np.float32) * sc).astype(np.float32)
    big = np.float32(1e30)
    special = np.concatenate([half, -half, np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, big, -big, 3.4e38, -3.4e38, (hi + 1000 - zp) * sc,
                                                     (lo - 1000 - zp) * sc, np.inf, -np.inf, np.nan, -np.nan], np.float32)]).astype(np.float32)
    ns = special.size
    for b in range(n):
        if E >= 2 * ns:
            x[b, rng.choice(E, ns, replace=False)] = special
        elif b % 2:
            k = min(E, ns)
            x[b, :k] = special[(b // 2 * k + np.arange(k)) % ns]
    return x


class Case:
    """one model: the device model, the oracle, the f32 batch and the oracle's predict for the images checked, computed once"""

    def __init__(self, O, name):
        import microflow_rs_amd as mf
        import torch
        build, self.kernel, self.batches = _models()[name]
        self.name = name
        self.blob = build()
        self.m = mf.Model(self.blob)
        self.m.prepare(1)
        self.om = O.Model(self.blob)
        self.n = max(self.batches)
        self.x = _inputs(self.om, self.n, 1900 + MODELS.index(name))
        self.N = self.om.out_elems
        # every image of the small batches; on the large one the first 77, the last 21 and 40 random ones
        small = 77 if self.n > 2000 else self.n
        picks = set(range(small))
        if self.n > small:
            picks = set(range(8)) | set(range(self.n - 21, self.n)) | set(np.random.default_rng(5).integers(0, self.n, 40).tolist()) | picks
        self.picks = np.array(sorted(picks))
        self.want = np.stack([self.om.predict(self.x[i]).reshape(-1) for i in self.picks]).astype(np.float32)
        self.xd = torch.as_tensor(self.x).cuda()
        lo, hi = (0, 256) if self.m.dtype == np.uint8 else (-128, 128)
        nq = min(self.n, 77)
        self.xq = torch.as_tensor(np.random.default_rng(6).integers(lo, hi, (nq, self.om.in_elems)).astype(self.m.dtype)).cuda()

    def check(self, got, n, what):
        got = np.asarray(got, np.float32).reshape(n, -1)
        keep = self.picks < n
        sel = self.picks[keep]
        a, b = got[sel].view(np.uint32), self.want[keep].view(np.uint32)
        bad = np.flatnonzero((a != b).any(axis=1))
        assert not bad.size, (self.name, what, n, "images", sel[bad][:8].tolist(), got[sel[bad[0]]], self.want[keep][bad[0]])


_cases = {}


def _case(O, name):
    if name not in _cases:
        _cases[name] = Case(O, name)
    return _cases[name]


@pytest.fixture(params=MODELS)
def case(request, O):
    return _case(O, request.param)


def _bits(t):
    return t.detach().cpu().numpy().reshape(-1).view(np.uint32)


def test_operator_zero_runs_the_kernel_the_case_is_about(case):
    if ROUTING_SWITCHED:
        pytest.skip("the kernel names describe the default routing, not %s" % ", ".join(ROUTING_SWITCHED))
    assert case.m.op(0)["kernel"] == case.kernel, (case.name, case.m.op(0)["kernel"])


def test_predict_is_the_oracles_floats_fused_layerwise_and_generic(case):
    m = case.m
    for n in case.batches:
        x = case.xd[:n]
        got = m.predict(x).cpu().numpy()
        case.check(got, n, "default")
        m.set_fusion(False)
        try:
            off = m.predict(x).cpu().numpy()
        finally:
            m.set_fusion(True)
        assert np.array_equal(off.view(np.uint32), got.view(np.uint32)), (case.name, n, "fusion off")   # (every image)
        if n > 2000:
            continue
        m.set_generic(True)
        try:
            gen = m.predict(x).cpu().numpy()
        finally:
            m.set_generic(False)
        assert np.array_equal(gen.view(np.uint32), got.view(np.uint32)), (case.name, n, "generic")


def _deltas(m, x, xq, of, oq):
    """device_ops() added by one predict and by one run_quantized (after one of each: scratch buffers are sized by then)"""
    m.predict(x, out=of), m.run_quantized(xq, out=oq)
    a = m.device_ops()
    m.predict(x, out=of)
    b = m.device_ops()
    m.run_quantized(xq, out=oq)
    return b - a, m.device_ops() - b


def _outs(c, n):
    import torch
    return (torch.empty((n, c.N), dtype=torch.float32, device="cuda"), torch.empty((n, c.N), dtype=c.m._tdtype(), device="cuda"))


@pytest.mark.parametrize("name", MODELS)
def test_predict_adds_no_launch(O, name):
    """the test the separate quantise pass fails: with it predict is one launch more than run_quantized on an i8 model whose last
    launch stores the floats, and that is what the models outside ENTRY keep.  A u8 model's run_quantized moves its bytes to the
    internal domain and back (two passes); its predict's last launch stores the floats (one fewer), and with the entry inside the
    first launch it needs neither pass: two fewer."""
    if ROUTING_SWITCHED:
        pytest.skip("the launch counts describe the default routing, not %s" % ", ".join(ROUTING_SWITCHED))
    c = _case(O, name)
    m, n = c.m, 77 if 77 in c.batches else c.batches[-1]
    x, xq = c.xd[:n], c.xq[:n]
    assert x.data_ptr() % 16 == 0 and xq.data_ptr() % 16 == 0
    of, oq = _outs(c, n)
    dp, dq = _deltas(m, x, xq, of, oq)
    print(name, "predict", dp, "run_quantized", dq)
    assert dq >= 1
    assert dp == (dq if name in ENTRY else dq + 1) - (2 if name in U8 else 0), (name, dp, dq)
    c.check(of.cpu().numpy(), n, "out=")


@pytest.mark.parametrize("name", ENTRY)
def test_input_view_offset_by_four_bytes_is_one_launch_more(O, name):
    """an f32 input that is not 16-byte aligned keeps the quantise pass (the staging loads 16 bytes): exactly one launch more, same floats"""
    import torch
    c = _case(O, name)
    m, n = c.m, 77
    buf = torch.zeros(n * c.om.in_elems + 8, dtype=torch.float32, device="cuda")
    view = buf[1:1 + n * c.om.in_elems]
    view.copy_(c.xd[:n].reshape(-1))
    assert view.data_ptr() % 16 == 4
    of, oq = _outs(c, n)
    dp, _ = _deltas(m, c.xd[:n], c.xq[:n], of, oq)
    ref = of.clone()
    dpo, _ = _deltas(m, view.reshape(n, -1), c.xq[:n], of, oq)
    assert np.array_equal(_bits(of), _bits(ref))
    if not ROUTING_SWITCHED:
        assert dpo == dp + 1, (name, dp, dpo)


def test_floats_around_the_output_stay(case):
    """the f32 output inside a larger buffer filled with a pattern, at a 16-byte aligned offset and at an odd float: exactly
    batch x output_elems floats change"""
    import torch
    m, N, n = case.m, case.N, min(case.batches[-1], 77)
    pat = np.float32(-1234.5)
    for off in (64, 3):
        buf = torch.full((off + n * N + 1024,), float(pat), dtype=torch.float32, device="cuda")
        out = buf[off:off + n * N]
        m.predict(case.xd[:n], out=out)
        b1 = buf.cpu().numpy()
        assert (b1[:off] == pat).all() and (b1[off + n * N:] == pat).all(), (case.name, n, off)
        case.check(b1[off:off + n * N], n, "guarded, offset %d" % off)


@pytest.mark.parametrize("name", ["rows-80x80x3-s2-16", "rows-76x76x3-12-u8-wzp-g1", "gemm-16x16x3-80"])
def test_overlapping_input_and_output_give_the_oracles_floats(O, name):
    import torch
    c = _case(O, name)
    m, n = c.m, 77
    E, N = c.om.in_elems, c.N
    for shift in (0, 4):                                       # the output at the input's start, and a few floats into it
        buf = torch.zeros(shift + n * max(E, N) + 64, dtype=torch.float32, device="cuda")
        xin = buf[:n * E]
        xin.copy_(c.xd[:n].reshape(-1))
        out = buf[shift:shift + n * N]
        m.predict(xin.reshape(n, -1), out=out)
        c.check(out.cpu().numpy(), n, "overlap, shift %d" % shift)


@pytest.mark.parametrize("name", ["rows-80x80x3-s2-16", "dwrows-136x128x1-4x3-12-g1", "gemm-10x10x2-72"])
def test_graph_replays_give_the_same_floats(O, name):
    import torch
    c = _case(O, name)
    m, n = c.m, 77
    x = c.xd[:n].clone()
    ref = m.predict(x).clone()
    c.check(ref.cpu().numpy(), n, "eager")
    m.set_graph(True)
    try:
        out = torch.empty_like(ref)
        before, ops = m.graph_launches, []
        for it in range(4):                                    # eager, captured + replayed, replayed, replayed
            out.zero_()
            a = m.device_ops()
            m.predict(x, out=out)
            ops.append(m.device_ops() - a)
            assert np.array_equal(_bits(out), _bits(ref)), (name, it)
        assert m.graph_launches >= before + 2
        assert ops[1:] == [1, 1, 1], ops                       # (a replay counts as one)
    finally:
        m.set_graph(False)


@pytest.mark.parametrize("name", ["rows-80x80x3-s2-16", "rows-144x128x1-5x5valid-6-g1", "rows-28x28x1-5x5valid-6"])
def test_host_fed_predict_equals_the_device_fed_one(O, name):
    c = _case(O, name)
    got = c.m.predict(c.x[:77])
    c.check(got, 77, "host-fed")
    assert np.array_equal(np.asarray(got).reshape(-1).view(np.uint32), _bits(c.m.predict(c.xd[:77])))


def test_dev_switch_brings_the_separate_pass_back():
    """MF_DEV=1 MF_NO_F32_BOUNDARY=1 (a child process: the switches are read once per process): predict is two launches more than
    run_quantized again (quantise and dequantise), and the floats are the same as the default child's"""
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import microflow_rs_amd as mf
import tflite_writer as tw
for k, shape, n in ((0, (80, 80, 3), 16), (1, (96, 96, 3), 8)):
    m = mf.Model(tw.conv_net(np.random.default_rng(73), shape, [("conv", n, 3, 2), ("conv", 16, 1, 1)][:1 + k], head=10))
    m.prepare(1)
    rng = np.random.default_rng(6)
    E = shape[0] * shape[1] * shape[2]
    x = torch.as_tensor(rng.normal(0, 2, (77, E)).astype(np.float32)).cuda()
    xq = torch.as_tensor(rng.integers(-128, 128, (77, E)).astype(np.int8)).cuda()
    of = torch.empty((77, 10), dtype=torch.float32, device="cuda")
    oq = torch.empty((77, 10), dtype=torch.int8, device="cuda")
    m.predict(x, out=of), m.run_quantized(xq, out=oq)
    a = m.device_ops(); m.predict(x, out=of); b = m.device_ops(); m.run_quantized(xq, out=oq); c = m.device_ops()
    print("OPS", b - a, c - b)
    np.save(sys.argv[1] + str(k) + ".npy", of.cpu().numpy())
''' % (ROOT, os.path.join(ROOT, "tools"))
    outs, ops = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for sw in (None, "1"):
            env = dict(os.environ)
            for k in [k for k in env if k.startswith("MF_")]:
                del env[k]
            if sw:
                env.update(MF_DEV="1", MF_NO_F32_BOUNDARY="1")
            path = os.path.join(tmp, "out%d_" % len(outs))
            r = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
            assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
            ops.append([[int(v) for v in l.split()[1:]] for l in r.stdout.splitlines() if l.startswith("OPS")])
            outs.append([np.load(path + "%d.npy" % k) for k in (0, 1)])
    for k in (0, 1):
        assert np.array_equal(outs[0][k].view(np.uint32), outs[1][k].view(np.uint32)), k
        assert ops[0][k][0] == ops[0][k][1], ops
        assert ops[1][k][0] == ops[1][k][1] + 2, ops
