#!/usr/bin/env python3
"""GPU box: FullyConnected shapes outside fc_rowwave / fc_mfma -- fc_generic (set_generic) against the run-time-shape
matrix-pipe kernel fc_rt (k_fc_rt.hip), and FullyConnected-only models (tools/tflite_writer.mlp, models/sine.tflite).

    python scripts/time_fc_rt.py [--rows 65536,262144] [--reps 20]

One line per case: the median of --reps launches, each timed with HIP events, back to back after warm-up; hbm_frac is
rows x (K + N) bytes (the least a launch must move) over time against 8.0 TB/s, mfma_frac is 2 rows K N operations over
time against 5.0 POP/s (dense int8 MFMA; both MI355X spec figures).  Outputs of the two paths are compared too."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import microflow_rs_amd as mf  # noqa: E402
import tflite_writer as tw  # noqa: E402
from microflow_rs_amd import _lib  # noqa: E402

HBM, MFMA_I8 = 8.0e12, 5.0e15
FC_SHAPES = [(784, 10), (1024, 64), (256, 12), (100, 3), (2048, 1000)]
MLPS = [("mlp 784-128-10+softmax", (784, 128, 10), dict(softmax=True)), ("mlp 64-64-64-10", (64, 64, 64, 10), dict(act="relu6"))]


def median_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def fc_case(K, N, rows, reps):
    rng = np.random.default_rng(K * 7 + N)
    w = rng.integers(-128, 128, (N, K)).astype(np.int8)
    c0 = rng.uniform(-3, 3, N).astype(np.float32)
    c1 = np.float32(1.0 / (300.0 * np.sqrt(K)))
    op = mf.ops.prepare_fully_connected(1, w, 0, 0.05, 3, mf.ops.FullyConnectedOptions(), (c0, c1, np.zeros(N, np.int32), 0))
    x = torch.randint(-128, 128, (rows, K), dtype=torch.int8, device="cuda")
    y = torch.empty(rows * N, dtype=torch.int8, device="cuda")
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    run = lambda: _lib.check(L.mf_op_run(op._h, x.data_ptr(), rows, y.data_ptr(), st))  # noqa: E731
    kern = op.kernel
    t_new = median_ms(run, reps)
    y_new = y.clone()
    op.set_generic(True)
    t_gen = median_ms(run, reps)
    same = bool(torch.equal(y, y_new))
    op.set_generic(False)
    hb, ops = rows * (K + N), 2.0 * rows * K * N
    print("fc %5d -> %4d rows %6d  %-10s %8.4f ms  fc_generic %9.4f ms  x%6.1f  hbm_frac %.3f  mfma_frac %.3f  same=%s" % (
        K, N, rows, kern, t_new, t_gen, t_gen / t_new, hb / (t_new * 1e-3) / HBM, ops / (t_new * 1e-3) / MFMA_I8, same), flush=True)


def model_case(name, blob, rows, reps):
    m = mf.Model(blob)
    m.prepare(rows)
    x = torch.randint(-128 if m.dtype == np.int8 else 0, 128 if m.dtype == np.int8 else 256, (rows, m.input_elems),
                      dtype=torch.int8 if m.dtype == np.int8 else torch.uint8, device="cuda")
    out = m.run_quantized(x).clone()
    ref = out.clone()
    kernels = sorted({m.op(i)["kernel"] for i in range(m.num_ops)})
    t = {}
    for label, setup in (("fused", lambda: (m.set_fusion(True), m.set_generic(False))),
                         ("layer-wise", lambda: (m.set_fusion(False), m.set_generic(False))),
                         ("generic", lambda: (m.set_fusion(True), m.set_generic(True)))):
        setup()
        t[label] = median_ms(lambda: m.run_quantized(x, out=out), reps)
        assert torch.equal(out, ref), (name, label)
    m.set_generic(False)
    print("%-24s rows %6d  fused %8.4f ms  layer-wise %8.4f ms  all fc_generic %8.4f ms  x%5.1f  kernels %s" % (
        name, rows, t["fused"], t["layer-wise"], t["generic"], t["generic"] / t["fused"], ",".join(kernels)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="65536,262144")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    for rows in [int(r) for r in a.rows.split(",")]:
        for K, N in FC_SHAPES:
            fc_case(K, N, rows, a.reps)
        for name, sizes, kw in MLPS:
            model_case(name, tw.mlp(np.random.default_rng(1), sizes, **kw), rows, a.reps)
        model_case("sine.tflite", open(os.path.join(ROOT, "models", "sine.tflite"), "rb").read(), rows, a.reps)


if __name__ == "__main__":
    main()
