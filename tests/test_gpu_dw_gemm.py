"""DepthwiseConv2D of any channel count and filter zero point on the int8 matrix pipe (k_dw_gemm.hip: dw_gemm_rt; one-channel
depthwise layers through conv_gemm_rt): routing, bit-exactness against the CPU oracle and against dwconv_generic over a sampled
shape grid, large images in row bands, the bytes around the output, the limits, generated inverted-residual models and the
MF_NO_DW_GEMM switch."""
import os

import numpy as np
import pytest

from tests.conftest import ROOT, ROUTING_SWITCHED

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def mf():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import microflow_rs_amd as m
    assert m.lib().mf_device_count() > 0
    return m


def _out_hw(H, W, KH, KW, sh, sw, same):
    if same:
        return -(-H // sh), -(-W // sw)
    return (H - KH) // sh + 1, (W - KW) // sw + 1


def on_generic_today(H, W, C, KH, KW, sh, sw, same, wz):
    """the DepthwiseConv2D routing of the parent commit (ops.hip route_*) for the shapes sampled here: C == N >= 2, finite constants, images
    small enough for every planner's budget.  The 3x3 SAME stride-1 / 2 family runs the tables or dw3x3_rt (dw_rt_plan: C % 4 == 0,
    W C % 16 == 0), with or without filter zero points; dw_mm_rt takes C % 16 == 0 without them; everything else ran dwconv_generic."""
    if KH == 3 and KW == 3 and same and sh == sw and sh in (1, 2) and C % 4 == 0 and (W * C) % 16 == 0:
        return False
    if C % 16 == 0 and not wz and KH <= 7 and KW <= 7:
        return False
    return True


def expected_kernel(H, W, C, KH, KW, sh, sw, same, wz):
    """None: not a shape this change moves (the old kernel, whatever it is, keeps it)"""
    if not on_generic_today(H, W, C, KH, KW, sh, sw, same, wz):
        return None
    if (W * C) % 4 == 0 and KH <= 7 and KW <= 7:
        return "dw_gemm_rt<%dx%d%s>" % (KH, KW, ",wzp" if wz else "")
    return "dwconv_generic"


def check_route(op, want):
    if ROUTING_SWITCHED:
        return
    if want is None:
        assert op.kernel != "dwconv_generic" and not op.kernel.startswith(("dw_gemm_rt", "conv_gemm_rt")), op.kernel
    else:
        assert op.kernel == want, (op.kernel, want)


def _consts(rng, n, taps):
    c0 = rng.uniform(-30, 30, n).astype(f32)
    return c0, (rng.uniform(0.5, 1.5, n) * 40.0 / (5476.0 * np.sqrt(taps))).astype(f32)


def make_dw(mf, O, rng, H, W, C, KH, KW, sh, sw, same, wz, act, u8, N=None, izp=None, consts=None):
    """a DepthwiseConv2D with N outputs (N = C by default); wz: per-channel filter zero points off the middle, the i8-domain extremes
    -128 and 127 among them"""
    N = C if N is None else N
    dt = np.uint8 if u8 else np.int8
    lo, hi = (0, 256) if u8 else (-128, 128)
    OH, OW = _out_hw(H, W, KH, KW, sh, sw, same)
    w = rng.integers(lo, hi, (KH, KW, N)).astype(dt)
    if wz:
        z = rng.integers(-128, 128, N)
        z[0], z[-1] = -128, 127
        z[z == 0] = 3
        zp = (z + (128 if u8 else 0)).astype(dt)
    else:
        zp = np.full(N, 128 if u8 else 0, dt)
    izp = int(rng.integers(lo, hi)) if izp is None else izp
    oscale, ozp = 0.0235294122, int(rng.integers(lo, lo + 100))
    c0, c1 = _consts(rng, N, KH * KW) if consts is None else consts
    pad = 0 if same else 1
    opts = mf.ops.DepthwiseConv2DOptions(mf.FusedActivation(act), mf.TensorViewPadding(pad), (sh, sw))
    op = mf.ops.prepare_depthwise_conv_2d((H, W, C), w, zp, izp, oscale, ozp, opts, (c0, c1), (OH, OW))
    ref = lambda x: O.depthwise_conv_2d(x, w, zp, izp, oscale, ozp, act, pad, (sh, sw), (OH, OW), c0, c1)  # noqa: E731
    return op, ref


def check(op, ref, x, pick=None):
    """the fast path against dwconv_generic over the whole output, and against the oracle on the picked images (all by default)"""
    import torch
    xd = torch.as_tensor(x).cuda()
    got = op(xd).cpu().numpy()
    op.set_generic(True)
    gen = op(xd).cpu().numpy()
    op.set_generic(False)
    assert np.array_equal(got, gen), int((got != gen).sum())
    for i in (range(len(x)) if pick is None else pick):
        assert np.array_equal(got[i], ref(x[i])), i
    return got


def _inputs(rng, batch, H, W, C, u8):
    lo, hi = (0, 256) if u8 else (-128, 128)
    x = rng.integers(lo, hi, (batch, H, W, C)).astype(np.uint8 if u8 else np.int8)
    x[0] = hi - 1
    x[-1, : H // 2] = lo
    return x


FILTERS = [(1, 1, 1, 1, True), (2, 3, 1, 1, False), (3, 3, 1, 1, True), (3, 3, 2, 2, True), (3, 3, 1, 1, False), (5, 5, 1, 1, True),
           (5, 5, 2, 2, True), (7, 7, 1, 1, True), (7, 7, 2, 2, False), (3, 3, 1, 2, True), (5, 3, 2, 1, False), (1, 5, 3, 3, True),
           (3, 3, 3, 3, True), (4, 2, 2, 3, False), (2, 4, 1, 1, True)]


def _grid():
    """C sampled, a filter / image / batch / wzp / izp / activation / element type per case; mostly shapes that ran dwconv_generic
    before this kernel, plus a few the older kernels keep (their labels must not change)"""
    rng = np.random.default_rng(11)
    cases = []
    for C, wz_only in [(c, False) for c in (2, 3, 4, 6, 8, 12, 20, 24, 36, 40, 72, 120)] + [(c, True) for c in (16, 48, 144)]:
        for _ in range(3):
            KH, KW, sh, sw, same = FILTERS[int(rng.integers(len(FILTERS)))]
            H = int(rng.integers(max(KH, 4), 13 if C < 72 else 9))
            W = int(rng.integers(max(KW, 4), 13 if C < 72 else 9))
            while (W * C) % 4:
                W += 1
            wz = True if wz_only else bool(rng.integers(0, 2))
            cases.append((H, W, C, KH, KW, sh, sw, same, wz, int(rng.choice((0, 1, 3))), bool(rng.integers(0, 2)),
                          int(rng.choice((1, 5, 37))), int(rng.integers(0, 3))))
    cases.append((9, 10, 6, 3, 3, 1, 1, True, True, 1, True, 4099, 0))        # a ragged last step above 4096 images
    cases.append((12, 12, 16, 3, 3, 1, 1, True, False, 3, False, 5, 0))       # dw3x3_rt keeps its shape
    cases.append((10, 10, 32, 5, 5, 1, 1, True, False, 3, True, 5, 1))        # dw_mm_rt keeps its shape
    return cases


def _id(c):
    return "%dx%dx%d-%dx%ds%d%d%s%s-act%d-%s-b%d-z%d" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6], "S" if c[7] else "V",
                                                        "-wzp" if c[8] else "", c[9], "u8" if c[10] else "i8", c[11], c[12])


@pytest.mark.parametrize("case", _grid(), ids=_id)
def test_dw_gemm_vs_oracle_and_generic(mf, O, case):
    H, W, C, KH, KW, sh, sw, same, wz, act, u8, batch, zsel = case
    rng = np.random.default_rng(abs(hash(case)) % (2 ** 32))
    lo, hi = (0, 256) if u8 else (-128, 128)
    izp = (lo, hi - 1, None)[zsel]                                             # the input zero point at both extremes, or random
    op, ref = make_dw(mf, O, rng, H, W, C, KH, KW, sh, sw, same, wz, act, u8, izp=izp)
    check_route(op, expected_kernel(H, W, C, KH, KW, sh, sw, same, wz))
    x = _inputs(rng, batch, H, W, C, u8)
    check(op, ref, x, None if batch < 100 else [0, 1, 2047, 4095, batch - 2, batch - 1])


@pytest.mark.parametrize("H,W,C,KH,KW,s,same,wz,batch", [(112, 112, 24, 5, 5, 1, True, False, 2), (112, 112, 24, 5, 5, 2, True, True, 3),
                                                         (224, 224, 8, 3, 3, 1, False, False, 2), (1, 1, 4, 3, 3, 1, True, True, 7),
                                                         (2, 3, 4, 2, 3, 1, False, True, 5), (2, 3, 12, 3, 3, 2, True, False, 9)])
@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
def test_dw_gemm_size_extremes(mf, O, H, W, C, KH, KW, s, same, wz, batch, u8):
    """images far beyond one tile (row bands with the zero-point halo above and below) and tiny ones (1x1, 2x3)"""
    rng = np.random.default_rng(H * W + C + KH + int(u8))
    op, ref = make_dw(mf, O, rng, H, W, C, KH, KW, s, s, same, wz, 3, u8)
    check_route(op, expected_kernel(H, W, C, KH, KW, s, s, same, wz))
    check(op, ref, _inputs(rng, batch, H, W, C, u8))


@pytest.mark.parametrize("H,W,C,K,s,wz,batch", [(7, 8, 6, 3, 1, True, 37), (9, 9, 20, 5, 2, False, 1001), (8, 8, 12, 3, 3, True, 4099),
                                                 (6, 8, 3, 7, 1, True, 5)])
def test_dw_gemm_leaves_the_bytes_around_the_output(mf, O, H, W, C, K, s, wz, batch):
    """the output handed over inside a larger buffer pre-filled with a pattern: C % 4 != 0, partial last channel groups, a ragged last
    step write exactly batch x OH x OW x C bytes; nothing in front of the output, nothing behind it"""
    import torch
    from microflow_rs_amd import _lib
    rng = np.random.default_rng(H * W * C + K)
    op, ref = make_dw(mf, O, rng, H, W, C, K, K, s, s, True, wz, 0, False)
    assert ROUTING_SWITCHED or op.kernel.startswith("dw_gemm_rt"), op.kernel
    OH, OW = _out_hw(H, W, K, K, s, s, True)
    xn = _inputs(rng, batch, H, W, C, False)
    x = torch.as_tensor(xn).cuda()
    want = op(x).cpu().numpy().reshape(-1)
    n = batch * OH * OW * C
    for off in (16, 48):
        buf = torch.full((off + n + 4096,), 0x5A, dtype=torch.int8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().mf_op_run(op._h, x.data_ptr(), batch, buf.data_ptr() + off, stream))
        b = buf.cpu().numpy()
        assert (b[:off] == 0x5A).all() and (b[off + n:] == 0x5A).all(), off
        assert np.array_equal(b[off:off + n], want)
    for i in (0, batch - 1):
        assert np.array_equal(want.reshape(batch, OH, OW, C)[i], ref(xn[i]))


def test_dw_gemm_limits_stay_on_the_generic_kernel(mf, O):
    """W C % 4 != 0, a 9x9 filter, 1 < C != N (the reference's channel-0 quirk), non-finite constants and a one-channel layer
    conv_gemm_rt cannot take (W % 4 != 0): dwconv_generic, with correct bytes"""
    rng = np.random.default_rng(99)
    shapes = [dict(H=7, W=7, C=3, KH=5, KW=5), dict(H=12, W=12, C=8, KH=9, KW=9), dict(H=8, W=8, C=4, KH=3, KW=5, N=8),
              dict(H=31, W=31, C=1, KH=5, KW=5, N=80)]
    for sh in shapes:
        op, ref = make_dw(mf, O, rng, sh["H"], sh["W"], sh["C"], sh["KH"], sh["KW"], 1, 1, True, True, 1, False, N=sh.get("N"))
        assert ROUTING_SWITCHED or op.kernel == "dwconv_generic", (sh, op.kernel)
        x = _inputs(rng, 3, sh["H"], sh["W"], sh["C"], False)
        assert np.array_equal(op(x), np.stack([ref(v) for v in x])), sh
    c0, c1 = _consts(rng, 24, 25)
    c0[3], c1[5] = np.nan, np.inf
    op, ref = make_dw(mf, O, rng, 8, 8, 24, 5, 5, 1, 1, True, False, 0, False, consts=(c0, c1))
    assert ROUTING_SWITCHED or op.kernel == "dwconv_generic", op.kernel
    x = _inputs(rng, 3, 8, 8, 24, False)
    assert np.array_equal(op(x), np.stack([ref(v) for v in x]))


@pytest.mark.parametrize("wz", [False, True], ids=["nowzp", "wzp"])
@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
def test_one_channel_depthwise_runs_conv_gemm(mf, O, u8, wz):
    """224x224x1 -> 16 5x5 stride 2 (a grayscale stem beyond dw_c1_lds, dw3x3_stem_rt and conv_rows_lds): conv_gemm_rt as the Conv2D
    with C = 1 that the reference's channel-0 read makes it"""
    rng = np.random.default_rng(224 + 2 * int(u8) + int(wz))
    op, ref = make_dw(mf, O, rng, 224, 224, 1, 5, 5, 2, 2, True, wz, 3, u8, N=16)
    assert ROUTING_SWITCHED or op.kernel == ("conv_gemm_rt<dw,wzp>" if wz else "conv_gemm_rt<dw>"), op.kernel
    check(op, ref, _inputs(rng, 3, 224, 224, 1, u8))


# ---- generated models (tools/tflite_writer.inverted_residual_net) -------------------------------------------------------------
BLOCKS = [(24, 5, 1, 8), (72, 5, 2, 24), (120, 5, 1, 40), (24, 7, 1, 24), (36, 3, 1, 16)]
MODELS = [("i8", False), ("i8", True), ("u8", True)]


def _model(elem, wz, seed):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import tflite_writer as tw
    return tw.inverted_residual_net(np.random.default_rng(seed), (28, 28, 8), BLOCKS, elem=3 if elem == "u8" else 9, wzp_nonzero=wz,
                                    head=20)


@pytest.mark.parametrize("elem,wz", MODELS, ids=["%s%s" % (e, "-wzp" if w else "") for e, w in MODELS])
def test_inverted_residual_models_have_no_generic_operator(O, elem, wz):
    """no operator of a MobileNetV3-style stack of 5x5 / 7x7 / 3x3 inverted-residual blocks runs a *_generic kernel; sampled
    images equal the oracle, also at several layers; the whole batch equals fusion off, all-generic and hipGraph replay"""
    import torch
    import microflow_rs_amd as mf
    blob = _model(elem, wz, 17 + int(wz) + (2 if elem == "u8" else 0))
    m = mf.Model(blob)
    m.prepare(1)
    names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    if not ROUTING_SWITCHED:
        assert not any(n.endswith("_generic") for n in names), names
        assert sum(n.startswith("dw_gemm_rt") for n in names) >= 4, names
    om = O.Model(blob)
    rng = np.random.default_rng(5)
    lo, hi = (0, 256) if m.dtype == np.uint8 else (-128, 128)
    n = 40
    xq = rng.integers(lo, hi, (n, m.input_elems)).astype(m.dtype)
    xq[0] = lo
    got = m.run_quantized(xq).reshape(n, -1)
    for i in (0, 1, n - 1):
        assert np.array_equal(got[i], om.run_quantized_batch(xq[i:i + 1]).reshape(-1)), (i, names)
    _, layers = om.run_quantized(xq[3], layers=True)
    for i in (1, 4, 7, 10, 13, len(layers) - 1):
        assert np.array_equal(np.asarray(m.run_until(xq[3:4], i)).reshape(-1), layers[i].reshape(-1)), (i, names[i])
    m.set_fusion(False)
    assert np.array_equal(m.run_quantized(xq).reshape(n, -1), got)
    m.set_fusion(True)
    m.set_generic(True)
    assert np.array_equal(m.run_quantized(xq).reshape(n, -1), got)
    m.set_generic(False)
    x = torch.as_tensor(xq).cuda()
    m.set_graph(True)
    out = torch.empty_like(torch.as_tensor(got)).cuda()
    for it in range(2):
        out.zero_()
        m.run_quantized(x, out=out)
        assert np.array_equal(out.cpu().numpy().reshape(n, -1), got), it
    m.set_graph(False)


def test_no_dw_gemm_switch_goes_back_to_generic():
    """MF_DEV=1 MF_NO_DW_GEMM=1 (a child process: the switches are read once per process): the same operators run dwconv_generic
    with the same bytes as dw_gemm_rt / conv_gemm_rt<dw> in this process"""
    import subprocess
    import sys as _sys
    import tempfile
    code = r'''
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import microflow_rs_amd as mf
import tflite_writer as tw
rng = np.random.default_rng(3)
m = mf.Model(tw.inverted_residual_net(np.random.default_rng(19), (28, 28, 8), %r, wzp_nonzero=True, head=20))
m.prepare(1)
x = rng.integers(-128, 128, (8, m.input_elems)).astype(np.int8)
w = rng.integers(-128, 128, (5, 5, 16)).astype(np.int8)
opts = mf.ops.DepthwiseConv2DOptions(mf.FusedActivation(3), mf.TensorViewPadding.SAME, (2, 2))
c0, c1 = rng.uniform(-30, 30, 16).astype(np.float32), np.full(16, 0.002, np.float32)
op = mf.ops.prepare_depthwise_conv_2d((224, 224, 1), w, rng.integers(-20, 20, 16).astype(np.int8), -5, 0.0235, 3, opts, (c0, c1), (112, 112))
xs = rng.integers(-128, 128, (2, 224, 224, 1)).astype(np.int8)
print("KERNELS", "|".join([m.op(i)["kernel"] for i in range(m.num_ops)] + [op.kernel]))
np.save(sys.argv[1], np.concatenate([np.asarray(m.run_quantized(x)).reshape(-1), np.asarray(op(xs)).reshape(-1)]))
''' % (ROOT, os.path.join(ROOT, "tools"), BLOCKS)
    outs, kernels = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for sw in (None, "1"):
            env = dict(os.environ)
            for k in [k for k in env if k.startswith("MF_")]:
                del env[k]
            if sw:
                env.update(MF_DEV="1", MF_NO_DW_GEMM="1")
            path = os.path.join(tmp, "out%d.npy" % len(outs))
            r = subprocess.run([_sys.executable, "-c", code, path], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
            assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
            kernels.append([l for l in r.stdout.splitlines() if l.startswith("KERNELS")][0].split(" ", 1)[1].split("|"))
            outs.append(np.load(path))
    assert np.array_equal(outs[0], outs[1])
    on, off = kernels
    moved = [i for i, (a, b) in enumerate(zip(on, off)) if a != b]
    assert moved and on[-1] == "conv_gemm_rt<dw,wzp>", (on, off)
    assert all(on[i].startswith(("dw_gemm_rt", "conv_gemm_rt<dw")) and off[i] == "dwconv_generic" for i in moved), (on, off)
