"""Conv2D of any channel count and width on the int8 matrix pipe (k_conv_gemm.hip: conv_gemm_rt): routing, bit-exactness against
the CPU oracle and against conv2d_generic over a sampled shape grid, large images in row bands, accumulators beyond 2^25, the bytes
around the output, the limits, generated models and the MF_NO_CONV_GEMM switch."""
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


def _rows_ok(H, W, C, N, KH, KW, sh, sw, OH, OW, same):
    """k_rt.hip conv_rows_plan"""
    RWB = KW * C
    if RWB > 64 or KH > 16 or N > 64 or (W * C) % 4 or C >= 16:
        return False
    KG, NP = (RWB + 3) // 4, (N + 7) & ~7
    padl, padt = ((KW - 1) // 2, (KH - 1) // 2) if same else (0, 0)
    XO = (padl * C + 3) & ~3
    need = XO - padl * C + (OW - 1) * sw * C + 4 * (KG + 1)
    TWP = (max(need, XO + W * C) + 7) & ~3
    TILE = (max((OH - 1) * sh + KH, padt + H) * TWP + 4 + 15) & ~15
    g = min(8, 8192 // max(H * (W * C // 4), 1))
    while g > 1 and g * TILE > 65536:
        g -= 1
    if g < 1 or TILE > 65536:
        return False
    return g * TILE + KH * KG * NP * 4 + ((KG * 4 + 15) & ~15) + NP * 16 + 64 <= 96 * 1024


def _mm_ok(W, C, N, KH, KW, wz):
    """k_rt.hip conv_mm_plan (its weight budget; the image geometry always fits at the sizes sampled here)"""
    if C % 16 or N % 4 or KH > 7 or KW > 7 or (W * C) % 16:
        return False
    KS, NT = (KH * KW * C + 63) // 64, (N + 15) // 16
    TB = min(NT, 4)
    return -(-NT // TB) * TB * KS * 1024 + (KS * 1024 if wz else 0) <= 96 * 1024


def on_generic_today(H, W, C, N, KH, KW, sh, sw, same, wz):
    """the Conv2D routing of the parent commit (ops.hip route_*) for the shapes sampled here: no 1x1 stride-1 filters (pw_rt,
    conv1x1_rowwave, the tables), finite constants"""
    assert not (KH == 1 and KW == 1 and sh == 1 and sw == 1)
    OH, OW = _out_hw(H, W, KH, KW, sh, sw, same)
    return not _rows_ok(H, W, C, N, KH, KW, sh, sw, OH, OW, same) and not _mm_ok(W, C, N, KH, KW, wz)


def expected_kernel(H, W, C, N, KH, KW, sh, sw, same, wz):
    if not on_generic_today(H, W, C, N, KH, KW, sh, sw, same, wz):
        return None
    if (W * C) % 4 == 0 and KH * ((KW * C + 15) // 16 * 16) <= 8192:  # conv_gemm_plan: whole-dword rows, K' <= 8192
        return "conv_gemm_rt<wzp>" if wz else "conv_gemm_rt"
    return "conv2d_generic"


def _consts(rng, n, taps):
    c0 = rng.uniform(-30, 30, n).astype(f32)
    return c0, (rng.uniform(0.5, 1.5, n) * 40.0 / (5476.0 * np.sqrt(taps))).astype(f32)


def make_conv(mf, O, rng, H, W, C, N, KH, KW, sh, sw, same, wz, act, u8, f=None, izp=None):
    dt = np.uint8 if u8 else np.int8
    lo, hi = (0, 256) if u8 else (-128, 128)
    OH, OW = _out_hw(H, W, KH, KW, sh, sw, same)
    if f is None:
        f = rng.integers(lo, hi, (N, KH, KW, C)).astype(dt)
    zp = (rng.integers(-25, 25, N) + (128 if u8 else 0)).astype(dt) if wz else np.full(N, 128 if u8 else 0, dt)
    izp = int(rng.integers(lo, hi)) if izp is None else izp
    oscale, ozp = 0.0235294122, int(rng.integers(lo, lo + 100))
    c0, c1 = _consts(rng, N, KH * KW * C)
    pad = 0 if same else 1
    opts = mf.ops.Conv2DOptions(mf.FusedActivation(act), mf.TensorViewPadding(pad), (sh, sw))
    op = mf.ops.prepare_conv_2d((H, W, C), f, zp, izp, oscale, ozp, opts, (c0, c1), (OH, OW))
    ref = lambda x: O.conv_2d(x, f, zp, izp, oscale, ozp, act, pad, (sh, sw), (OH, OW), c0, c1)  # noqa: E731
    return op, ref


def check(op, ref, x, pick=None):
    """the fast path against conv2d_generic over the whole output, and against the oracle on the picked images (all by default)"""
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


FILTERS = [(1, 1, 2, 2, True), (2, 3, 1, 1, False), (3, 3, 1, 1, True), (3, 3, 2, 2, True), (5, 5, 1, 1, True), (7, 7, 2, 2, True),
           (3, 3, 1, 2, True), (3, 1, 2, 1, False), (5, 3, 2, 1, False)]


def _grid():
    """C x N sampled, a filter / image / batch / wzp / activation / element type per case; only shapes that ran conv2d_generic
    before this kernel and have whole-dword rows"""
    Cs = (1, 2, 3, 4, 8, 12, 20, 24, 40, 64, 96, 128, 256, 512)
    Ns = (1, 3, 10, 16, 24, 64, 96, 100, 128, 256, 512)
    rng = np.random.default_rng(7)
    cases = []
    for C in Cs:
        picks = rng.choice(Ns, 4, replace=False) if C < 256 else rng.choice(Ns, 2, replace=False)
        for N in picks:
            for _ in range(8):
                KH, KW, sh, sw, same = FILTERS[int(rng.integers(len(FILTERS)))]
                H = int(rng.integers(max(KH, 4), 11 if C < 256 else 6))
                W = int(rng.integers(max(KW, 4), 11 if C < 256 else 6))
                while (W * C) % 4:
                    W += 1
                wz = bool(rng.integers(0, 2))
                if on_generic_today(H, W, C, int(N), KH, KW, sh, sw, same, wz):
                    cases.append((H, W, C, int(N), KH, KW, sh, sw, same, wz, int(rng.choice((0, 1, 3))), bool(rng.integers(0, 2)),
                                  int(rng.choice((1, 3, 37)))))
                    break
    cases.append((8, 8, 24, 24, 1, 1, 2, 2, True, True, 3, False, 37))    # 1x1 stride 2, C = 24
    cases.append((6, 8, 3, 96, 3, 3, 1, 1, True, False, 1, False, 4100))   # ragged batch above 4096 on a small shape
    return cases


def _id(c):
    return "%dx%dx%d-N%d-%dx%ds%d%d%s%s-act%d-%s-b%d" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], "S" if c[8] else "V",
                                                     "-wzp" if c[9] else "", c[10], "u8" if c[11] else "i8", c[12])


@pytest.mark.parametrize("case", _grid(), ids=_id)
def test_conv_gemm_vs_oracle_and_generic(mf, O, case):
    H, W, C, N, KH, KW, sh, sw, same, wz, act, u8, batch = case
    rng = np.random.default_rng(abs(hash(case)) % (2 ** 32))
    op, ref = make_conv(mf, O, rng, H, W, C, N, KH, KW, sh, sw, same, wz, act, u8)
    assert ROUTING_SWITCHED or op.kernel == expected_kernel(H, W, C, N, KH, KW, sh, sw, same, wz), (op.kernel, case)
    x = _inputs(rng, batch, H, W, C, u8)
    check(op, ref, x, None if batch < 100 else [0, 1, 2047, batch - 2, batch - 1])


@pytest.mark.parametrize("H,W,C,N,K,s,batch", [(224, 224, 3, 32, 3, 2, 3), (224, 224, 3, 64, 7, 2, 2), (128, 128, 3, 16, 3, 1, 3)])
@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
def test_conv_gemm_large_images(mf, O, H, W, C, N, K, s, batch, u8):
    """few-channel images far beyond one tile: row bands with the zero-point halo above and below"""
    rng = np.random.default_rng(H + N + K + int(u8))
    wz = u8
    op, ref = make_conv(mf, O, rng, H, W, C, N, K, K, s, s, True, wz, 3, u8)
    assert ROUTING_SWITCHED or op.kernel == expected_kernel(H, W, C, N, K, K, s, s, True, wz), op.kernel
    check(op, ref, _inputs(rng, batch, H, W, C, u8))


@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
def test_conv_gemm_accumulators_beyond_2_25(mf, O, u8):
    """3x3x512 -> 512 (K' = 4608, one resident tile per workgroup, 32 slices) with extreme operands: |acc| up to 4608 x 255 x 128"""
    H, W, C, N = 4, 4, 512, 512
    rng = np.random.default_rng(512 + int(u8))
    lo, hi = (0, 256) if u8 else (-128, 128)
    dt = np.uint8 if u8 else np.int8
    f = rng.integers(lo, hi, (N, 3, 3, C)).astype(dt)
    f[0], f[1] = lo, hi - 1
    f[2, :, :, ::2], f[2, :, :, 1::2] = lo, hi - 1
    op, ref = make_conv(mf, O, rng, H, W, C, N, 3, 3, 1, 1, True, False, 0, u8, f=f, izp=lo)
    assert ROUTING_SWITCHED or op.kernel == "conv_gemm_rt", op.kernel
    x = _inputs(rng, 5, H, W, C, u8)
    x[1] = lo
    check(op, ref, x)


@pytest.mark.parametrize("H,W,C,N,K,s,batch", [(7, 8, 20, 10, 3, 1, 37), (5, 4, 3, 100, 3, 2, 1001), (4, 4, 128, 130, 3, 1, 9),
                                                 (6, 6, 512, 30, 3, 1, 5)])
def test_conv_gemm_leaves_the_bytes_around_the_output(mf, O, H, W, C, N, K, s, batch):
    """the output handed over inside a larger buffer pre-filled with a pattern: N % 4 != 0, a ragged last step, the sliced-weight
    shapes write exactly batch x OH x OW x N bytes; nothing in front of the output, nothing behind it"""
    import torch
    from microflow_rs_amd import _lib
    rng = np.random.default_rng(H * W * C + N)
    op, ref = make_conv(mf, O, rng, H, W, C, N, K, K, s, s, True, bool(N % 2), 0, False)
    assert ROUTING_SWITCHED or op.kernel.startswith("conv_gemm_rt"), op.kernel
    OH, OW = _out_hw(H, W, K, K, s, s, True)
    xn = _inputs(rng, batch, H, W, C, False)
    x = torch.as_tensor(xn).cuda()
    want = op(x).cpu().numpy().reshape(-1)
    n = batch * OH * OW * N
    for off in (16, 48):                               # 16-byte-aligned offsets keep the fast path
        buf = torch.full((off + n + 4096,), 0x5A, dtype=torch.int8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().mf_op_run(op._h, x.data_ptr(), batch, buf.data_ptr() + off, stream))
        b = buf.cpu().numpy()
        assert (b[:off] == 0x5A).all() and (b[off + n:] == 0x5A).all(), off
        assert np.array_equal(b[off:off + n], want)
    for i in (0, batch - 1):
        assert np.array_equal(want.reshape(batch, OH, OW, N)[i], ref(xn[i]))


def test_conv_gemm_limits_stay_on_the_generic_kernel(mf, O):
    """K' = 3 x 3 x 1024 > 8192, non-finite constants, and 21-byte image rows: conv2d_generic, with correct bytes"""
    rng = np.random.default_rng(1024)
    op, ref = make_conv(mf, O, rng, 3, 3, 1024, 16, 3, 3, 1, 1, True, False, 1, False)
    assert ROUTING_SWITCHED or op.kernel == "conv2d_generic", op.kernel
    x = _inputs(rng, 3, 3, 3, 1024, False)
    assert np.array_equal(op(x), np.stack([ref(v) for v in x]))
    op, ref = make_conv(mf, O, rng, 7, 7, 3, 100, 3, 3, 1, 1, True, False, 0, False)       # (W C) % 4 != 0
    assert ROUTING_SWITCHED or op.kernel == "conv2d_generic", op.kernel
    x = _inputs(rng, 3, 7, 7, 3, False)
    assert np.array_equal(op(x), np.stack([ref(v) for v in x]))
    # non-finite constants on a shape conv_gemm_rt would take
    H, W, C, N = 6, 6, 24, 24
    f = rng.integers(-128, 128, (N, 3, 3, C)).astype(np.int8)
    c0, c1 = _consts(rng, N, 9 * C)
    c0[3], c1[5] = np.nan, np.inf
    opts = mf.ops.Conv2DOptions(mf.FusedActivation(0), mf.TensorViewPadding.SAME, (1, 1))
    zp = np.zeros(N, np.int8)
    op = mf.ops.prepare_conv_2d((H, W, C), f, zp, -3, 0.0235294122, 5, opts, (c0, c1), (H, W))
    assert ROUTING_SWITCHED or op.kernel == "conv2d_generic", op.kernel
    x = _inputs(rng, 3, H, W, C, False)
    want = np.stack([O.conv_2d(v, f, zp, -3, 0.0235294122, 5, 0, 0, (1, 1), (H, W), c0, c1) for v in x])
    assert np.array_equal(op(x), want)


# ---- generated models (tools/tflite_writer.conv_net) ----------------------------------------------------------------------
CIFAR = [("conv", 32, 3, 1), ("conv", 64, 3, 2), ("conv", 128, 3, 1), ("conv", 128, 3, 2), ("conv", 256, 3, 1)]
MOBILENET_FRONT = [("conv", 32, 3, 2), ("dw", 0, 3, 1), ("conv", 64, 1, 1), ("dw", 0, 3, 2), ("conv", 128, 1, 1), ("dw", 0, 3, 1),
                   ("conv", 128, 1, 1)]
MODELS = [("cifar", (32, 32, 3), CIFAR, 10, "i8", False), ("cifar", (32, 32, 3), CIFAR, 10, "i8", True),
          ("cifar", (32, 32, 3), CIFAR, 10, "u8", False), ("cifar", (32, 32, 3), CIFAR, 10, "u8", True),
          ("mobilenet_front", (224, 224, 3), MOBILENET_FRONT, None, "i8", False)]


def _model(shape, convs, head, elem, wz, seed):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import tflite_writer as tw
    return tw.conv_net(np.random.default_rng(seed), shape, convs, elem=elem, wzp_nonzero=wz, head=head)


@pytest.mark.parametrize("name,shape,convs,head,elem,wz", MODELS, ids=["%s-%s%s" % (m[0], m[4], "-wzp" if m[5] else "") for m in MODELS])
def test_conv_models_have_no_generic_operator(O, name, shape, convs, head, elem, wz):
    """no operator of a plain CIFAR-style CNN or of a 224x224 MobileNet-v1 front runs a *_generic kernel; sampled images equal
    the oracle; the whole batch equals all-generic, fusion off and hipGraph replay"""
    import torch
    import microflow_rs_amd as mf
    elem_code = 3 if elem == "u8" else 9
    blob = _model(shape, convs, head, elem_code, wz, sum(map(ord, name + elem)) + int(wz))
    m = mf.Model(blob)
    m.prepare(1)
    names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    if not ROUTING_SWITCHED:
        assert not any(n.endswith("_generic") for n in names), names
    om = O.Model(blob)
    rng = np.random.default_rng(5)
    lo, hi = (0, 256) if m.dtype == np.uint8 else (-128, 128)
    n = 64 if name == "cifar" else 6
    xq = rng.integers(lo, hi, (n, m.input_elems)).astype(m.dtype)
    xq[0] = lo
    got = m.run_quantized(xq).reshape(n, -1)
    for i in (0, 1, n - 1):
        assert np.array_equal(got[i], om.run_quantized_batch(xq[i:i + 1]).reshape(-1)), (i, names)
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


def test_no_conv_gemm_switch_goes_back_to_generic():
    """MF_DEV=1 MF_NO_CONV_GEMM=1 (a child process: the switches are read once per process): the same operators run
    conv2d_generic with the same bytes as conv_gemm_rt in this process"""
    import subprocess
    import sys as _sys
    code = r'''
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import microflow_rs_amd as mf
import tflite_writer as tw
rng = np.random.default_rng(3)
x = rng.integers(-128, 128, (8, 32 * 32 * 3)).astype(np.int8)
m = mf.Model(tw.conv_net(np.random.default_rng(11), (32, 32, 3), %r, head=10))
m.prepare(1)
print("KERNELS", "|".join(m.op(i)["kernel"] for i in range(m.num_ops)))
np.save(sys.argv[1], m.run_quantized(x).reshape(8, -1))
''' % (ROOT, os.path.join(ROOT, "tools"), CIFAR)
    import tempfile
    outs, kernels = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for sw in (None, "1"):
            env = dict(os.environ)
            for k in [k for k in env if k.startswith("MF_")]:
                del env[k]
            if sw:
                env.update(MF_DEV="1", MF_NO_CONV_GEMM="1")
            path = os.path.join(tmp, "out%d.npy" % len(outs))
            r = subprocess.run([_sys.executable, "-c", code, path], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
            assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
            kernels.append([l for l in r.stdout.splitlines() if l.startswith("KERNELS")][0].split(" ", 1)[1].split("|"))
            outs.append(np.load(path))
    assert np.array_equal(outs[0], outs[1])
    on, off = kernels
    moved = [i for i, (a, b) in enumerate(zip(on, off)) if a != b]
    assert moved and all(on[i].startswith("conv_gemm_rt") and off[i] == "conv2d_generic" for i in moved), (on, off)
