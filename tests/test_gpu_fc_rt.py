"""FullyConnected of any K and N on the int8 matrix pipe (k_fc_rt.hip): bit-exact against the CPU oracle and against the
shape-generic kernel, routing, the bytes around the output, and accumulators beyond 2^24."""
import numpy as np
import pytest

from tests.conftest import ROUTING_SWITCHED

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def mf():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import microflow_rs_amd as m
    assert m.lib().mf_device_count() > 0
    return m


def expected_kernel(K, N, wzp_i8):
    if K % 16 == 0 and K >= 256 and N in (1, 2, 4, 8):
        return "fc_rowwave<%d>" % N
    if N % 128 == 0 and K % 128 == 0:
        return "fc_mfma"
    if K * N <= 256:                 # one 16 x 16 weight tile of work per row at most: the byte-wise kernel is as fast
        return "fc_generic"
    return "fc_rt<wzp>" if wzp_i8 else "fc_rt"


def make_fc(mf, O, rng, M, K, N, wzp, act, u8):
    """an operator with the reference's own constants (preprocess_fully_connected) and spread-out outputs"""
    dt = np.uint8 if u8 else np.int8
    lo, hi = (0, 256) if u8 else (-128, 128)
    w = rng.integers(lo, hi, (N, K)).astype(dt)
    bias = rng.integers(-3000, 3000, N).astype(np.int32)
    izp = int(rng.integers(lo, hi))
    iscale, wscale = 0.05, 0.01
    oscale, ozp = f32(0.05 * 0.01 * 160 * np.sqrt(K)), int(rng.integers(lo + 20, hi - 20))
    c = O.preprocess_fully_connected(iscale, izp, K, w, wscale, wzp, bias, iscale * wscale, 0, oscale)
    op = mf.ops.prepare_fully_connected(M, w, wzp, oscale, ozp, mf.ops.FullyConnectedOptions(mf.FusedActivation(act)), c)
    ref = lambda x: O.fully_connected(x, w, wzp, oscale, ozp, act, *c)  # noqa: E731  x [rows][K]
    return op, ref


def run_both(op, x):
    """(fast path, fc_generic) on the same device input"""
    import torch
    xd = torch.as_tensor(x).cuda()
    got = op(xd).cpu().numpy()
    op.set_generic(True)
    gen = op(xd).cpu().numpy()
    op.set_generic(False)
    return got, gen


def _grid():
    """a sample of M x K x N x wzp x act x element type, every K and every N present, a few ragged batches each"""
    Ks = (1, 3, 16, 17, 63, 64, 65, 100, 513, 784, 4000)
    Ns = (1, 2, 3, 10, 12, 16, 17, 64, 100, 130)
    rng = np.random.default_rng(2024)
    cases = set()
    for i, K in enumerate(Ks):
        for N in rng.choice(Ns, 4, replace=False):
            cases.add((int(rng.choice((1, 3))), K, int(N), int(rng.integers(0, 2)), int(rng.choice((0, 1, 3))), bool(rng.integers(0, 2))))
    for j, N in enumerate(Ns):
        cases.add((3 if j % 2 else 1, Ks[(3 * j + 1) % len(Ks)], N, j % 2, (0, 1, 3)[j % 3], j % 3 == 0))
    return sorted(cases)


@pytest.mark.parametrize("case", _grid(), ids=lambda c: "M%d-K%d-N%d-wzp%d-act%d-%s" % (c[:5] + ("u8" if c[5] else "i8",)))
def test_fc_rt_vs_oracle_and_generic(mf, O, case):
    M, K, N, wz, act, u8 = case
    rng = np.random.default_rng(K * 1000 + N * 7 + M)
    wzp = (int(rng.integers(1, 100)) * (1 if u8 else -1) + (128 if u8 else 0)) if wz else (128 if u8 else 0)
    op, ref = make_fc(mf, O, rng, M, K, N, wzp, act, u8)
    wzp_i8 = wzp - 128 if u8 else wzp
    assert ROUTING_SWITCHED or op.kernel == expected_kernel(K, N, wzp_i8), (op.kernel, case)
    dt = np.uint8 if u8 else np.int8
    lo, hi = (0, 256) if u8 else (-128, 128)
    for rows in (1, 7, 4099):
        batch = max(1, rows // M)
        x = rng.integers(lo, hi, (batch, M, K)).astype(dt)
        x[0, 0, :] = lo                               # constant extremes in the first and the last row
        x[-1, -1, :] = hi - 1
        got, gen = run_both(op, x)
        assert np.array_equal(got, gen), (case, rows, int((got != gen).sum()))
        pick = sorted({0, batch // 2, batch - 1})
        want = ref(x[pick].reshape(-1, K)).reshape(len(pick), M, N)
        assert np.array_equal(got[pick], want), (case, rows)


@pytest.mark.parametrize("K,N,wzp", [(784, 10, 0), (1024, 64, -9), (2048, 1000, 0)])
def test_fc_rt_whole_output_equals_generic(mf, O, K, N, wzp):
    """every byte of a 65 536-row run against fc_generic, rows spread over the batch against the oracle"""
    rows = 65536
    rng = np.random.default_rng(K + N)
    op, ref = make_fc(mf, O, rng, 1, K, N, wzp, 0, False)
    assert ROUTING_SWITCHED or op.kernel == expected_kernel(K, N, wzp), op.kernel
    x = rng.integers(-128, 128, (rows, 1, K)).astype(np.int8)
    got, gen = run_both(op, x)
    assert np.array_equal(got, gen), int((got != gen).sum())
    pick = [0, 1, 15, 16, 4095, 33333, rows - 2, rows - 1]
    assert np.array_equal(got[pick].reshape(-1, N), ref(x[pick].reshape(-1, K)))


@pytest.mark.parametrize("K,N,rows", [(100, 10, 4099), (17, 31, 1001), (65, 17, 77), (3, 100, 1025), (4000, 130, 35), (2048, 1000, 21)])
def test_fc_rt_leaves_the_bytes_around_the_output(mf, O, K, N, rows):
    """the output handed over inside a larger buffer pre-filled with a pattern: a ragged last row tile (and, for the sliced
    shapes, every slice) writes exactly rows x N bytes; nothing in front of the output, nothing behind it"""
    import torch
    from microflow_rs_amd import _lib
    rng = np.random.default_rng(K * 3 + rows)
    op, ref = make_fc(mf, O, rng, 1, K, N, 0, 0, False)
    assert ROUTING_SWITCHED or op.kernel == "fc_rt", op.kernel
    x = torch.as_tensor(rng.integers(-128, 128, (rows, K)).astype(np.int8)).cuda()
    want = op(x).cpu().numpy().reshape(-1)
    for off in (16, 48):                               # 16-byte-aligned offsets keep the fast path
        buf = torch.full((off + rows * N + 4096,), 0x5A, dtype=torch.int8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().mf_op_run(op._h, x.data_ptr(), rows, buf.data_ptr() + off, stream))
        b = buf.cpu().numpy()
        assert (b[:off] == 0x5A).all() and (b[off + rows * N:] == 0x5A).all(), (K, N, rows, off)
        assert np.array_equal(b[off:off + rows * N], want)
    pick = [0, rows // 2, rows - 1]
    assert np.array_equal(want.reshape(rows, N)[pick], ref(x.cpu().numpy()[pick]))


def test_fc_rt_accumulators_beyond_2_24(mf, O):
    """K = 4000 with extreme operands: |acc| up to 4000 * 128 * 128 > 2^25, converted to f32 with rounding exactly as
    fc_generic's (float)acc -- epilogue mode 0 (the bit-pattern modes need |acc| < 2^22 and are not chosen)"""
    K, N, rows = 4000, 3, 600
    rng = np.random.default_rng(44)
    w = np.where(rng.random((N, K)) < 0.97, -128, 127).astype(np.int8)
    w[1] = 127
    w[2, ::2], w[2, 1::2] = -128, 127
    x = np.where(rng.random((rows, K)) < 0.98, -128, 127).astype(np.int8)
    x[0], x[1], x[2] = -128, 127, rng.integers(-128, 128, K)
    x[3:40] = -128
    for i in range(3, 40):                         # accumulators one step apart around 2^25 + odd values
        x[i, :i] = rng.integers(-128, 128, i)
    c0 = np.array([0.25, -3.5, 1.0], f32)
    c1 = f32(1.0 / 524287.0)                       # not a power of two: the product's rounding matters
    c2 = np.zeros(N, np.int32)
    op = mf.ops.prepare_fully_connected(1, w, 0, 0.05, 0, mf.ops.FullyConnectedOptions(), (c0, c1, c2, 0))
    assert ROUTING_SWITCHED or op.kernel == "fc_rt", op.kernel
    acc = x.astype(np.int64) @ w.astype(np.int64).T
    assert np.abs(acc).max() > 2 ** 25
    got, gen = run_both(op, x.reshape(rows, 1, K))
    want = O.fully_connected(x, w, 0, 0.05, 0, 0, c0, c1, c2, 0)
    assert np.array_equal(gen.reshape(rows, N), want)
    assert np.array_equal(got.reshape(rows, N), want), int((got.reshape(rows, N) != want).sum())
    assert len(np.unique(want)) > 5                   # the outputs are spread, not saturated


def test_fc_rt_k_limit(mf, O):
    """the documented limit: one 16-column weight slice (16 x pad64(K) bytes) and one 16-row buffer must fit the LDS
    budget -- K = 5056 runs fc_rt, K = 5057 stays on fc_generic; both bit-exact"""
    rng = np.random.default_rng(3)
    for K, kern in ((5056, "fc_rt"), (5057, "fc_generic")):
        op, ref = make_fc(mf, O, rng, 1, K, 3, 0, 0, False)
        assert ROUTING_SWITCHED or op.kernel == kern, (K, op.kernel)
        x = rng.integers(-128, 128, (37, 1, K)).astype(np.int8)
        got, gen = run_both(op, x)
        assert np.array_equal(got, gen) and np.array_equal(got.reshape(37, 3), ref(x.reshape(37, K)))


def test_fc_rt_unaligned_pointers_and_non_finite_constants(mf, O):
    """an output pointer that is not 16-byte aligned takes the byte-wise kernel (same bytes); non-finite constants stay on
    fc_generic (Rust's NaN -> 0 cast)"""
    import torch
    from microflow_rs_amd import _lib
    rng = np.random.default_rng(5)
    op, ref = make_fc(mf, O, rng, 1, 100, 10, 0, 1, False)
    x = torch.as_tensor(rng.integers(-128, 128, (300, 100)).astype(np.int8)).cuda()
    want = op(x).cpu().numpy().reshape(-1)
    buf = torch.zeros(300 * 10 + 64, dtype=torch.int8, device="cuda")
    _lib.check(_lib.lib().mf_op_run(op._h, x.data_ptr(), 300, buf.data_ptr() + 3, torch.cuda.current_stream().cuda_stream))
    assert np.array_equal(buf.cpu().numpy()[3:3 + 3000], want)
    w = rng.integers(-128, 128, (10, 100)).astype(np.int8)
    c0 = rng.uniform(-3, 3, 10).astype(f32)
    c0[4] = np.nan
    op = mf.ops.prepare_fully_connected(1, w, 0, 0.05, 3, mf.ops.FullyConnectedOptions(), (c0, f32(1e-3), np.zeros(10, np.int32), 0))
    assert ROUTING_SWITCHED or op.kernel == "fc_generic"


# ---- FullyConnected-only models (tools/tflite_writer.mlp): fc_chain -------------------------------------------------------
MLPS = [((1, 16, 16, 1), {}, 1), ((3, 100, 16, 1), {}, 7), ((64, 64, 64, 10), dict(act="relu6"), 3), ((100, 12, 3), dict(elem=3), 4),
        ((65, 17, 10), dict(wzp_nonzero=True), 5), ((63, 100, 130, 17), dict(wzp_nonzero=True), 6), ((64, 100, 10), dict(softmax=True), 8),
        ((100, 64, 12), dict(softmax=True, elem=3), 9)]


def _mlp(sizes, kw, seed):
    import os
    import sys
    from tests.conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import tflite_writer as tw
    return tw.mlp(np.random.default_rng(seed), sizes, **kw)


def _check_model(O, m, blob, seed, ns=(1, 17, 3000)):
    """fused == oracle == layer-wise == all fc_generic; run_until at every layer; hipGraph replay == eager"""
    import torch
    om = O.Model(blob)
    rng = np.random.default_rng(seed)
    lo, hi = (0, 256) if m.dtype == np.uint8 else (-128, 128)
    for n in ns:
        xq = rng.integers(lo, hi, (n, m.input_elems)).astype(m.dtype)
        xq[0] = lo
        want = om.run_quantized_batch(xq).reshape(n, -1)
        got = m.run_quantized(xq).reshape(n, -1)
        assert np.array_equal(got, want), n
        m.set_fusion(False)
        assert np.array_equal(m.run_quantized(xq).reshape(n, -1), got), n
        m.set_fusion(True)
        m.set_generic(True)
        assert np.array_equal(m.run_quantized(xq).reshape(n, -1), got), n
        m.set_generic(False)
    _, layers = om.run_quantized(xq[min(5, len(xq) - 1)], layers=True)
    k = min(5, len(xq) - 1)
    for i in range(len(layers)):                  # run_until inside a chain runs unfused up to that operator
        assert np.array_equal(np.asarray(m.run_until(xq[k:k + 1], i)).reshape(-1), layers[i].reshape(-1)), (i, m.op(i)["kernel"])
    x = torch.as_tensor(xq[:64]).cuda()
    ref = m.run_quantized(x).clone()
    m.set_graph(True)
    out = torch.empty_like(ref)
    for it in range(3):
        out.zero_()
        m.run_quantized(x, out=out)
        assert torch.equal(out, ref), it
    m.set_graph(False)


@pytest.mark.parametrize("sizes,kw,seed", MLPS, ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else None)
def test_mlp_models_run_as_one_fc_chain(O, sizes, kw, seed):
    """a generated MLP is ONE fc_chain launch: operator 0 reports the chain, every other operator "fused"; layer-wise (fusion
    off) its layers run fc_rt / fc_generic as alone; results equal the oracle every way they are run"""
    import microflow_rs_amd as mf
    blob = _mlp(sizes, kw, seed)
    m = mf.Model(blob)
    m.prepare(1)
    nfc = len(sizes) - 1
    if not ROUTING_SWITCHED:
        names = [m.op(i)["kernel"] for i in range(m.num_ops)]
        want0 = "fc_chain<%d>%s" % (nfc, "+sm" if kw.get("softmax") else "")
        assert names[0] == want0 and all(n == "(fused into the previous operator)" for n in names[1:]), names
        m.set_fusion(False)
        wz = kw.get("wzp_nonzero", False)
        assert [m.op(i)["kernel"] for i in range(nfc)] == [expected_kernel(sizes[i], sizes[i + 1], wz) for i in range(nfc)]
        m.set_fusion(True)
    _check_model(O, m, blob, seed)


@pytest.mark.parametrize("seed", [2, 12])
def test_mlp_784_128_10_keeps_its_layer_launches(O, seed):
    """784 -> 128 -> 10 + Softmax: the 104 KiB first-layer image leaves LDS room for only 16 rows per step of a chain, fewer than
    the layers' own launches keep in flight (the chain was 2x slower), so no chain is formed: fc_rt, fc_rt, softmax"""
    import microflow_rs_amd as mf
    blob = _mlp((784, 128, 10), dict(softmax=True), seed)
    m = mf.Model(blob)
    m.prepare(1)
    if not ROUTING_SWITCHED:
        assert [m.op(i)["kernel"] for i in range(m.num_ops)] == ["fc_rt", "fc_rt", "softmax_table"]
    _check_model(O, m, blob, seed)


def test_sine_is_one_launch(O):
    """models/sine.tflite (1 -> 16 -> 16 -> 1) runs as one fc_chain launch, and the reference's 500 recorded outputs still match"""
    import csv
    import os
    import microflow_rs_amd as mf
    from tests.conftest import GOLDEN, model_path
    m = mf.model(model_path("sine"))
    m.prepare(1)
    if not ROUTING_SWITCHED:
        names = [m.op(i)["kernel"] for i in range(m.num_ops)]
        assert names[0] == "fc_chain<3>" and all(n == "(fused into the previous operator)" for n in names[1:]), names
    rows = list(csv.reader(open(os.path.join(GOLDEN, "sine_microflow.csv"))))[1:]
    x = np.array([f32(r[0]) for r in rows], f32).reshape(-1, 1, 1)
    y = np.array([f32(r[1]) for r in rows], f32)
    assert np.array_equal(m.predict(x).reshape(-1), y)
    _check_model(O, m, open(model_path("sine"), "rb").read(), 9, ns=(1, 500, 65536))


def test_chain_beyond_the_lds_budget_is_cut(O):
    """1024 -> 64 -> 64 -> 1024 -> 16 -> 10: the five layers' images (~150 KiB) plus their tiles do not fit one launch's LDS; the
    run is cut greedily into shorter chains, each still bit-exact"""
    import microflow_rs_amd as mf
    sizes = (1024, 64, 64, 1024, 16, 10)
    blob = _mlp(sizes, {}, 21)
    m = mf.Model(blob)
    m.prepare(1)
    if not ROUTING_SWITCHED:
        names = [m.op(i)["kernel"] for i in range(m.num_ops)]
        launches = [n for n in names if n != "(fused into the previous operator)"]
        assert names[0].startswith("fc_chain<") and names[0] != "fc_chain<5>", names
        assert 2 <= len(launches) < 5 and all(n.startswith("fc_chain<") or n.startswith("fc_rt") for n in launches), names
    _check_model(O, m, blob, 21, ns=(1, 333, 4099))
