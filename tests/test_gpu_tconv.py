"""TRANSPOSE_CONV (k_tconv.hip): tconv_phase_rt and tconv_generic, each byte for byte against the contract restated in
tests/tconv_ref.py, through ops.transpose_conv's prepared operator.  Every case names what it can break.

Inputs are uniform over the whole byte range, weights uniform in +-127; c1 puts the standard deviation of c1 * acc near 190 output
steps around a zero point near the middle of the range, so that about half the outputs lie strictly inside the clamp (asserted on
the reference's result, which needs no GPU).  Seeds are fixed per case."""
import zlib

import numpy as np
import pytest

from tests import tconv_ref as T

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def mf():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import microflow_rs_amd as m
    assert m.lib().mf_device_count() > 0
    return m


#        H   W   C    N  KH KW sh sw same batch
SHAPES = {
    1:  (4,  4,  16,  16, 3, 3, 2, 2, True, 2),    # phases of 4 / 2 / 2 / 1 taps, top / left halo
    2:  (5,  3,  16,  8,  4, 4, 2, 2, True, 2),    # padt = 1, a base row beyond H - 1 (bottom / right halo), N < 16
    3:  (3,  4,  16,  24, 3, 3, 2, 2, False, 2),   # odd output 7 x 9: phases with unequal pixel counts, masked stores
    4:  (3,  5,  32,  20, 2, 2, 2, 2, False, 2),   # one tap per phase, N % 16 != 0
    5:  (3,  3,  16,  16, 2, 2, 3, 3, False, 2),   # phases with NO tap (acc = 0)
    6:  (5,  5,  16,  16, 3, 3, 1, 1, True, 2),    # a single phase, the flipped filter
    7:  (4,  6,  16,  16, 5, 3, 1, 2, True, 2),    # unequal strides and filter sides, Ty = 5
    8:  (4,  4,  4,   12, 3, 3, 2, 2, True, 2),    # AL = 4 operand
    9:  (4,  4,  20,  10, 3, 3, 2, 2, True, 2),    # AL = 4 operand, byte stores (N % 4 != 0)
    10: (32, 32, 64,  16, 3, 3, 2, 2, True, 3),    # the tile exceeds the whole-image budget: row bands, halo rows between bands
    11: (4,  4,  128, 128, 3, 3, 2, 2, True, 2),   # weights beyond the resident budget: N slices
    12: (4,  4,  16,  16, 3, 3, 2, 2, True, 5),    # case 1, a ragged last step when G > 1
    17: (4,  4,  18,  16, 3, 3, 2, 2, True, 2),    # case 1 with C = 18: routes to tconv_generic, still exact
}
FAST, GENERIC = "tconv_phase_rt", "tconv_generic"
#        id                 shape  variation                      kernel
CASES = [(str(i), i, {}, GENERIC if i == 17 else FAST) for i in SHAPES] + [
    ("13-worst", 1, dict(worst=True), FAST),       # input all -128, weights all 127, unit scales: the accumulator bound, saturation
    ("14-u8-1", 1, dict(u8=True), FAST),
    ("14-u8-2", 2, dict(u8=True), FAST),
    ("15-relu", 1, dict(act=1), FAST),
    ("15-relu6", 1, dict(act=3), FAST),
    ("15-nobias", 1, dict(bias=False), FAST),
    ("16-wzp", 1, dict(wz=True), GENERIC),         # per-channel non-zero filter zero points: tconv_generic, still exact
]


def build(name, shape, u8=False, act=0, bias=True, wz=False, worst=False, batch=None):
    """-> (prepare(mf) giving the operator, x, the contract's output)"""
    H, W, C, N, KH, KW, sh, sw, same, batch = SHAPES[shape][:9] + (batch or SHAPES[shape][9],)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    dt, off = (np.uint8, 128) if u8 else (np.int8, 0)
    OH, OW = T.out_hw(H, W, KH, KW, sh, sw, same)
    x = (rng.integers(-128, 128, (batch, H, W, C)) + off).astype(dt)
    w = (rng.integers(-127, 128, (N, KH, KW, C)) + off).astype(dt)
    wzp = (np.where(rng.integers(0, 2, N) > 0, 1, -1) * rng.integers(1, 25, N) if wz else np.zeros(N, np.int64)) + off
    izp, ozp = int(rng.integers(-20, 21)) + off, int(rng.integers(-20, 21)) + off
    oscale = f32(0.0235294122)
    c0 = rng.uniform(-30, 30, N).astype(f32) if bias else np.zeros(N, f32)
    c1 = (rng.uniform(0.8, 1.25, N) * 190.0 / (74.0 * 73.3 * np.sqrt(KH * KW * C / (sh * sw)))).astype(f32)
    if worst:
        x[:], w[:], izp, c0, c1 = -128, 127, 0, np.zeros(N, f32), np.ones(N, f32)
    want = T.transpose_conv(x, w, izp, wzp, (sh, sw), (OH, OW), c0, c1, ozp, oscale, act)

    def prepare(mf):
        opts = mf.ops.TransposeConvOptions(mf.FusedActivation(act), mf.TensorViewPadding(0 if same else 1), (sh, sw))
        return mf.ops.prepare_transpose_conv((H, W, C), w, wzp.astype(dt), izp, oscale, ozp, opts, (c0, c1), (OH, OW))
    return prepare, x, want


@pytest.mark.parametrize("name,shape,var,kernel", CASES, ids=[c[0] for c in CASES])
def test_transpose_conv_is_the_contract(mf, name, shape, var, kernel):
    prepare, x, want = build(name, shape, **var)
    if not var.get("worst") and not var.get("act"):
        lo, hi = (0, 255) if want.dtype == np.uint8 else (-128, 127)
        inside = float(np.mean((want > lo) & (want < hi)))
        assert 0.35 <= inside <= 0.65, inside       # (a property of the test's constants, from the reference alone)
    op = prepare(mf)
    assert op.kernel.startswith(kernel), op.kernel
    got = op(x)
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    op.set_generic(True)
    assert op.kernel.startswith(GENERIC), op.kernel
    gen = op(x)
    assert np.array_equal(gen, want), int((gen != want).sum())


@pytest.mark.parametrize("shape,batch,unique", [(1, 70003, 61), (10, 803, 3)], ids=["whole-images", "bands"])
def test_a_workgroup_walks_many_steps(mf, shape, batch, unique):
    """More steps than the launch can have workgroups (at most 8 of 256 threads per CU on 256 CUs: 2048; three per CU beside case 10's
    46 KiB of LDS), so every workgroup stages over a tile it has read: 4376 steps of G = 16 whole images with a ragged last one, and
    1606 bands whose out-of-image halo row is refilled.  `unique` different images repeated, and the reference's output repeated alike."""
    import torch
    prepare, x, want = build("steps-%d" % shape, shape, batch=unique)
    idx = torch.arange(batch) % unique
    op = prepare(mf)
    assert op.kernel.startswith(FAST)
    got = op(torch.as_tensor(x)[idx].cuda())
    bad = (got != torch.as_tensor(want)[idx].cuda()).flatten(1).any(1).nonzero().flatten()
    assert bad.numel() == 0, bad[:8].tolist()


def test_the_existing_corpus_routes_as_on_the_parent(mf):
    """scripts/routing_dump.py's fixed corpus, prepared in this process, gets the launches tests/golden/routing_corpus.txt recorded on
    the commit before TRANSPOSE_CONV: the parser's choice of the operand that continues the chain, create_conv's kind argument and
    op_epilogue_mode moved no existing model"""
    import os
    import sys
    from tests.conftest import ROOT, ROUTING_SWITCHED
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import routing_dump
    lines = []
    for name, make in routing_dump.corpus_all():
        m = mf.Model(make(), autotune=False)
        m.prepare(64)
        lines.append("# " + name)
        lines += ["%d %s %d" % (i, m.op(i)["kernel"], m.op_epilogue_mode(i)) for i in range(m.num_ops)]
    with open(os.path.join(ROOT, "tests", "golden", "routing_corpus.txt")) as f:
        assert ROUTING_SWITCHED or lines == f.read().splitlines()   # (an MF_* routing switch in the environment moves launches on purpose)


@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
def test_conv_autoencoder_runs_as_the_composed_operators(mf, u8):
    """conv_autoencoder((16, 16, 4), (16, 32)), batch 7: the Conv2D runs through the CPU oracle (one model per run of reference
    operators), the TRANSPOSE_CONVs through tests/tconv_ref.py; predict is the same composition behind quantize and in front of
    dequantize (src/tensor.rs: roundf(x / s + zp) saturating; s * f32(q - zp))"""
    import os
    import sys
    from tests import maxpool_ref as R
    from tests.conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import tflite_writer as tw
    from oracle import oracle as O
    elem, dt = (tw.UINT8, np.uint8) if u8 else (tw.INT8, np.int8)
    in_q, layers = tw.conv_autoencoder_layers(np.random.default_rng(67), (16, 16, 4), (16, 32), elem=elem)
    m = mf.model(tw.build_model((1, 16, 16, 4), in_q, layers, elem))
    assert [o["kind"] for o in m.ops] == [3, 3, 67, 67, 3]

    def composed(xq):
        t, shape, q = xq, (1, 16, 16, 4), in_q
        for L in layers:
            if L["op"] == "transpose_conv":
                mid = 128 if u8 else 0
                c0 = (F32(L["bscale"]) / F32(L["out_q"][0])) * (np.asarray(L["bias"], np.int32) - np.asarray(L["bzp"], np.int32)).astype(F32)
                c1 = (F32(q[0]) * F32(L["fscale"])) / F32(L["out_q"][0])
                t = T.transpose_conv(t.reshape((len(t),) + shape[1:]), np.asarray(L["filters"], dt), q[1], np.full(1, mid), L["strides"],
                                     L["out_shape"][1:3], c0, c1, L["out_q"][1], L["out_q"][0], L["act"])
            else:
                t = O.Model(tw.build_model(shape, q, [L], elem)).run_quantized_batch(t.reshape(len(t), -1))
            shape, q = tuple(L["out_shape"]), L["out_q"]
        return np.asarray(t).reshape(len(xq), -1), q
    rng = np.random.default_rng(3)
    xq = (rng.integers(-128, 128, (7, 16, 16, 4)) + (128 if u8 else 0)).astype(dt)
    want, out_q = composed(xq)
    assert np.array_equal(m.run_quantized(xq).reshape(7, -1), want)
    names = [m.op(i)["kernel"] for i in range(m.num_ops)]   # (the launches exist once the model is prepared)
    assert all(n.startswith(FAST) for n in names[2:4]), names
    xf = rng.uniform(-4, 4, (7, 16, 16, 4)).astype(F32)
    xq = R.saturate(R.roundf(xf / F32(in_q[0]) + F32(in_q[1])), dt).astype(dt)
    want = F32(out_q[0]) * (composed(xq)[0].astype(np.int32) - int(out_q[1])).astype(F32)
    assert np.array_equal(m.predict(xf).reshape(7, -1), want)


F32 = np.float32
