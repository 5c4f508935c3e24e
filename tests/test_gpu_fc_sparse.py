"""FullyConnected with 2:4-sparse weights on the sparse int8 matrix instruction (k_fc_sparse.hip, fc_sparse24): routing, bit-exact
parity against the CPU oracle and against the shape-generic kernel, the bytes around the output, repeatability, graph replay and
generated models."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT, ROUTING_SWITCHED

pytestmark = pytest.mark.gpu

f32 = np.float32
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def mf():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import microflow_rs_amd as m
    assert m.lib().mf_device_count() > 0
    return m


def sparse_weights(rng, N, K, extremes=False):
    """i8 weights with 0, 1 or 2 non-zero bytes in every aligned group of four along K, at every index pair; with `extremes` the
    non-zero bytes are mostly +-127 / -128; a few whole rows are zero"""
    pats = [()] + [(p,) for p in range(4)] + [(a, b) for a in range(4) for b in range(a + 1, 4)]
    sel = rng.integers(0, len(pats), N * K // 4)
    w = np.zeros((N * K // 4, 4), np.int8)
    for i, pat in enumerate(pats):
        rows = np.nonzero(sel == i)[0]
        for q in pat:
            v = rng.integers(1, 128, len(rows)) * rng.choice((-1, 1), len(rows))
            if extremes:
                v = rng.choice((-128, 127, -127), len(rows))
            w[rows, q] = v
    w = w.reshape(N, K)
    w[rng.integers(0, N, 2)] = 0
    return w


def make_fc(mf, O, rng, K, N, wzp, act, u8, w=None):
    """an operator with the reference's own constants (preprocess_fully_connected); w in the i8 domain"""
    if w is None:
        w = sparse_weights(rng, N, K)
    lo, hi = (0, 256) if u8 else (-128, 128)
    if u8:
        w = (w.astype(np.int16) + 128).astype(np.uint8)
    bias = rng.integers(-3000, 3000, N).astype(np.int32)
    izp = (lo + hi) // 2                          # centred inputs: the weight zero point term does not saturate the outputs
    iscale, wscale = 0.05, 0.01
    oscale, ozp = f32(0.05 * 0.01 * 110 * np.sqrt(K)), int(rng.integers(lo + 20, hi - 20))
    c = O.preprocess_fully_connected(iscale, izp, K, w, wscale, wzp, bias, iscale * wscale, 0, oscale)
    op = mf.ops.prepare_fully_connected(1, w, wzp, oscale, ozp, mf.ops.FullyConnectedOptions(mf.FusedActivation(act)), c)
    ref = lambda x: O.fully_connected(x, w, wzp, oscale, ozp, act, *c)  # noqa: E731  x [rows][K]
    return op, ref, w


def run_both(op, x):
    """(fast path, fc_generic) on the same device input"""
    import torch
    xd = torch.as_tensor(x).cuda()
    got = op(xd).cpu().numpy()
    op.set_generic(True)
    gen = op(xd).cpu().numpy()
    op.set_generic(False)
    return got, gen


def wzp_of(u8, nonzero, rng):
    return (int(rng.integers(1, 100)) * (1 if u8 else -1) + (128 if u8 else 0)) if nonzero else (128 if u8 else 0)


# ---- routing ----------------------------------------------------------------------------------------------------------------
def test_sparse_weights_route_to_fc_sparse24(mf, O):
    """2:4 weights on fc_mfma's shapes take fc_sparse24 (fc_sparse24<wzp> with a weight zero point); one group of three non-zero
    bytes keeps fc_mfma; N or K off a multiple of 128 keeps today's kernel; non-finite constants stay on fc_generic"""
    if ROUTING_SWITCHED:
        pytest.skip("routing switched")
    rng = np.random.default_rng(1)
    for u8 in (False, True):
        for wz in (0, 1):
            op, _, _ = make_fc(mf, O, rng, 256, 128, wzp_of(u8, wz, rng), 0, u8)
            assert op.kernel == ("fc_sparse24<wzp>" if wz else "fc_sparse24"), (u8, wz, op.kernel)
    w = sparse_weights(rng, 128, 256)
    w[77, 128:132] = (5, -3, 0, 9)
    op, _, _ = make_fc(mf, O, rng, 256, 128, 0, 0, False, w=w)
    assert op.kernel == "fc_mfma"
    for K, N, kern in ((256, 192, "fc_rt"), (200, 128, "fc_rt"), (4096, 8, "fc_rowwave<8>")):
        op, _, _ = make_fc(mf, O, rng, K, N, 0, 0, False, w=sparse_weights(rng, N, K))
        assert op.kernel == kern, (K, N, op.kernel)
    w = sparse_weights(rng, 128, 256)
    c0 = rng.uniform(-3, 3, 128).astype(f32)
    c0[3] = np.inf
    op = mf.ops.prepare_fully_connected(1, w, 0, 0.05, 3, mf.ops.FullyConnectedOptions(), (c0, f32(1e-3), np.zeros(128, np.int32), 0))
    assert op.kernel == "fc_generic"


_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import microflow_rs_amd as mf
from tests.test_gpu_fc_sparse import sparse_weights
rng = np.random.default_rng(8)
w = sparse_weights(rng, 256, 512)
c0 = rng.uniform(-3, 3, 256).astype(np.float32)
op = mf.ops.prepare_fully_connected(1, w, -5, 0.05, 3, mf.ops.FullyConnectedOptions(), (c0, np.float32(2e-4), np.zeros(256, np.int32), 0))
x = torch.as_tensor(rng.integers(-128, 128, (1000, 512)).astype(np.int8)).cuda()
np.save(sys.argv[2], op(x).cpu().numpy())
print(op.kernel)
"""


def test_switch_sends_sparse_weights_back_to_fc_mfma(tmp_path):
    """MF_DEV=1 MF_NO_FC_SPARSE=1 (a child process: the switches are read once) runs fc_mfma on the same weights, same bytes"""
    outs = {}
    for name, extra in (("sparse", {}), ("dense", {"MF_DEV": "1", "MF_NO_FC_SPARSE": "1"})):
        env = {k: v for k, v in os.environ.items() if not k.startswith("MF_")}
        env.update(extra)
        path = str(tmp_path / (name + ".npy"))
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[name] = (r.stdout.strip().split("\n")[-1], np.load(path))
    assert outs["sparse"][0] == "fc_sparse24<wzp>" and outs["dense"][0] == "fc_mfma", outs
    assert np.array_equal(outs["sparse"][1], outs["dense"][1])


# ---- parity -----------------------------------------------------------------------------------------------------------------
SHAPES = [(128, 128, 128), (256, 512, 384), (384, 128, 256), (5000, 384, 4096), (8192, 256, 8192)]
CASES = [(M, K, N, wz, act, u8) for (M, K, N) in SHAPES for wz in (0, 1) for act, u8 in ((0, False), (1, True), (3, False), (0, True))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "M%d-K%d-N%d-wzp%d-act%d-%s" % (c[:5] + ("u8" if c[5] else "i8",)))
def test_fc_sparse24_vs_oracle_and_generic(mf, O, case):
    M, K, N, wz, act, u8 = case
    rng = np.random.default_rng(M + 7 * K + 13 * N + wz)
    op, ref, _ = make_fc(mf, O, rng, K, N, wzp_of(u8, wz, rng), act, u8)
    assert ROUTING_SWITCHED or op.kernel == ("fc_sparse24<wzp>" if wz else "fc_sparse24"), op.kernel
    lo, hi = (0, 256) if u8 else (-128, 128)
    x = rng.integers(lo, hi, (M, K)).astype(np.uint8 if u8 else np.int8)
    x[0], x[-1] = lo, hi - 1
    got, gen = run_both(op, x)
    assert np.array_equal(got, gen), int((got != gen).sum())
    pick = np.arange(M) if M * K * N <= 2 ** 31 else np.unique(np.r_[0, 1, 63, 64, 255, 256, rng.integers(0, M, 120), M - 2, M - 1])
    assert np.array_equal(got.reshape(M, N)[pick], ref(x[pick])), case
    assert len(np.unique(got)) > 20 or act != 0  # (relu / relu6 clamp most outputs)


def test_fc_sparse24_extremes_and_accumulators_beyond_2_24(mf, O):
    """+-127 / -128 weights against constant extreme inputs: |acc| up to 2048 * 128 * 128 = 2^25, converted to f32 with rounding
    exactly as fc_generic's (float)acc"""
    K, N, M = 4096, 256, 512
    rng = np.random.default_rng(44)
    w = sparse_weights(rng, N, K, extremes=True)
    w[5] = 0
    w[6] = 0
    w[6].reshape(-1, 4)[:, :2] = -128           # two -128 of every four: acc = 2^25 on a constant -128 row
    x = np.where(rng.random((M, K)) < 0.98, -128, 127).astype(np.int8)
    x[0], x[1], x[2] = -128, 127, rng.integers(-128, 128, K)
    x[3:40] = -128
    for i in range(3, 40):                       # accumulators one step apart around 2^25
        x[i, :i] = rng.integers(-128, 128, i)
    c0 = rng.uniform(-2, 2, N).astype(f32)
    c1 = f32(1.0 / 524287.0)                     # not a power of two: the product's rounding matters
    c2 = np.zeros(N, np.int32)
    op = mf.ops.prepare_fully_connected(1, w, 0, 0.05, 0, mf.ops.FullyConnectedOptions(), (c0, c1, c2, 0))
    assert ROUTING_SWITCHED or op.kernel == "fc_sparse24", op.kernel
    acc = x.astype(np.int64) @ w.astype(np.int64).T
    assert np.abs(acc).max() >= 2 ** 25
    got, gen = run_both(op, x)
    want = O.fully_connected(x, w, 0, 0.05, 0, 0, c0, c1, c2, 0)
    assert np.array_equal(gen.reshape(M, N), want)
    assert np.array_equal(got.reshape(M, N), want), int((got.reshape(M, N) != want).sum())
    assert len(np.unique(want)) > 5


@pytest.mark.parametrize("wz", [0, 1])
def test_fc_sparse24_4096_cubed(mf, O, wz):
    """4096^3 (the 256^2-tile instance): every row against fc_generic, sampled rows against the oracle"""
    rng = np.random.default_rng(4096 + wz)
    op, ref, _ = make_fc(mf, O, rng, 4096, 4096, wzp_of(False, wz, rng), 0, False)
    x = rng.integers(-128, 128, (4096, 4096)).astype(np.int8)
    got, gen = run_both(op, x)
    assert np.array_equal(got, gen), int((got != gen).sum())
    pick = [0, 1, 255, 256, 2047, 4095]
    assert np.array_equal(got.reshape(4096, 4096)[pick], ref(x[pick]))


# ---- robustness -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [64, 333, 4096 + 77])
def test_fc_sparse24_leaves_the_bytes_around_the_output(mf, O, rows):
    """a ragged last row tile writes exactly rows x N bytes: nothing in front of the output, nothing behind it; five repeated
    launches give the same bytes"""
    import torch
    from microflow_rs_amd import _lib
    K, N = 512, 256
    rng = np.random.default_rng(rows)
    op, ref, _ = make_fc(mf, O, rng, K, N, -7, 0, False)
    x = torch.as_tensor(rng.integers(-128, 128, (rows, K)).astype(np.int8)).cuda()
    want = op(x).cpu().numpy().reshape(-1)
    assert np.array_equal(want.reshape(rows, N), ref(x.cpu().numpy()))
    stream = torch.cuda.current_stream().cuda_stream
    for off in (16, 48):
        buf = torch.full((off + rows * N + 4096,), 0x5A, dtype=torch.int8, device="cuda")
        for _ in range(5):
            _lib.check(_lib.lib().mf_op_run(op._h, x.data_ptr(), rows, buf.data_ptr() + off, stream))
            b = buf.cpu().numpy()
            assert (b[:off] == 0x5A).all() and (b[off + rows * N:] == 0x5A).all(), (rows, off)
            assert np.array_equal(b[off:off + rows * N], want)


def test_fewer_than_64_rows_fall_to_fc_generic(mf, O):
    rng = np.random.default_rng(63)
    op, ref, _ = make_fc(mf, O, rng, 256, 128, 0, 0, False)
    x = rng.integers(-128, 128, (63, 256)).astype(np.int8)
    got, gen = run_both(op, x)
    assert np.array_equal(got, gen) and np.array_equal(got.reshape(63, 128), ref(x))


@pytest.mark.parametrize("u8,wzp", [(False, 0), (False, -3), (True, 131)])
def test_generated_sparse_model(O, u8, wzp):
    """make_fc_model.py --sparse24 through predict, predict_quantized and run_quantized equals the oracle; hipGraph replay of one
    batch size equals eager"""
    import torch
    import microflow_rs_amd as mf
    from make_fc_model import synthetic_fc
    M, K, N = 256, 512, 256
    blob = synthetic_fc(M, K, N, wzp=wzp, seed=9, u8=u8, sparse24=True)
    m = mf.Model(blob)
    m.prepare(1)
    assert ROUTING_SWITCHED or m.op(0)["kernel"] == ("fc_sparse24<wzp>" if wzp not in (0, 128) else "fc_sparse24"), m.op(0)["kernel"]
    om = O.Model(blob)
    rng = np.random.default_rng(5)
    lo, hi = (0, 256) if u8 else (-128, 128)
    xq = rng.integers(lo, hi, (2, m.input_elems)).astype(m.dtype)
    want = om.run_quantized_batch(xq).reshape(2, -1)
    assert np.array_equal(m.run_quantized(xq).reshape(2, -1), want)
    got = np.asarray(m.predict_quantized(xq)).reshape(2, -1)
    assert all(np.array_equal(got[i], om.predict_quantized(xq[i]).reshape(-1)) for i in range(2))
    xf = rng.uniform(-1, 1, (2, m.input_elems)).astype(f32)
    got = np.asarray(m.predict(xf)).reshape(2, -1)
    assert all(np.array_equal(got[i], om.predict(xf[i]).reshape(-1)) for i in range(2))
    x = torch.as_tensor(xq[:1]).cuda()
    ref = m.run_quantized(x).clone()
    m.set_graph(True)
    out = torch.empty_like(ref)
    for it in range(3):
        out.zero_()
        m.run_quantized(x, out=out)
        assert torch.equal(out, ref), it
    m.set_graph(False)


def test_mlp_with_sparse_layers_keeps_its_chain(O):
    """256 -> 512 -> 256 -> 64 -> 10 with the two big layers 2:4: the fc_chain of the small layers and every fc_rt label stay as
    they are with dense weights; only the stand-alone fc_mfma layers become fc_sparse24; results equal the oracle"""
    import microflow_rs_amd as mf
    import tflite_writer as tw
    sizes = (256, 512, 256, 64, 10)
    names = {}
    for sp in ((), (0, 1)):
        blob = tw.mlp(np.random.default_rng(31), sizes, sparse24=sp)
        m = mf.Model(blob)
        m.prepare(1)
        names[sp] = [m.op(i)["kernel"] for i in range(m.num_ops)]
        m.set_fusion(False)
        names[sp] += [m.op(i)["kernel"] for i in range(m.num_ops)]
        m.set_fusion(True)
    if not ROUTING_SWITCHED:
        assert "fc_mfma" in names[()], names
        assert names[(0, 1)] == [n.replace("fc_mfma", "fc_sparse24") for n in names[()]], names
    om = O.Model(blob)
    xq = np.random.default_rng(2).integers(-128, 128, (3000, m.input_elems)).astype(m.dtype)
    assert np.array_equal(m.run_quantized(xq).reshape(3000, -1), om.run_quantized_batch(xq).reshape(3000, -1))
