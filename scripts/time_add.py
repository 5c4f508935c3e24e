#!/usr/bin/env python3
"""GPU box: the ADD operator's launch (k_add.hip: add_c16) at the tensor sizes of the layer-wise tables, against two yardsticks timed
in the same process on buffers of the same size:

    torch.add(a, b, out=c) on int8 tensors   the same 3 bytes per element, a wrapping integer add
    c.copy_(a)                                a plain device copy, 2 bytes per element, scaled to 3

    python scripts/time_add.py [--reps 20] [--only 3] [--model]

Two lines per size -- an operator whose constants keep the statement's own form (add_c16) and one the host admits the gated form for
(add_c16<fma>) -- each the median of --reps runs of each, each timed with HIP events after warm-up, in three repeats of the whole
measurement -- the median of the three medians and their spread ((max - min) / median) -- the ratios, hbm_frac = 3 bytes per element
over add_c16's time against 8.0 TB/s (the MI355X spec figure; a plain copy reaches 5.3 - 5.6 TB/s, profiles/r03/hbm_copy_ceiling.txt),
and parity: add_c16's bytes against add_generic's on the same operator.

--model times tools/tflite_writer.inverted_residual_net(residual=True) against the same blocks without the adds: the cost of the adds
in a whole model (the two models draw different quantisations behind the first block; the launches are the same).

Every case runs in a child process of its own under a time limit; the first that fails or runs into its limit ends the run."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM = 8.0e12
BATCH = 65536
SIZES = [(96, 96, 8), (48, 48, 16), (24, 24, 32), (12, 12, 64), (6, 6, 128)]  # per image
MODEL_BLOCKS = [(96, 3, 1, 16), (96, 3, 1, 16), (144, 3, 2, 24), (144, 3, 1, 24), (144, 3, 1, 24)]
MODEL_SHAPE, MODEL_BATCH = (28, 28, 16), 4096
STEP_TIMEOUT = 240  # seconds per case
REPEATS = 3
# (a, b, output) quantisations: one whose constants the gated form is refused for (add_c16, the statement's own form) and one it is
# admitted for (add_c16<fma>): tests/test_gpu_add.py's "unequal" and "halves"
QUANTS = [((0.05, 3), (0.031, -7), (0.07, -5)), ((0.05, 3), (0.05, -7), (0.1, -5))]


def median_ms(fn, reps, warm=3):
    import torch
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


def repeated(fn, reps):
    """(median of REPEATS medians, their spread)"""
    ms = [median_ms(fn, reps) for _ in range(REPEATS)]
    return float(np.median(ms)), float((max(ms) - min(ms)) / np.median(ms))


def one(idx, reps):
    import torch
    from microflow_rs_amd import _lib, ops
    assert torch.cuda.is_available(), "needs the GPU"
    H, W, C = SIZES[idx]
    elems = H * W * C
    n = BATCH * elems
    a = torch.randint(-128, 128, (n,), dtype=torch.int8, device="cuda")
    b = torch.randint(-128, 128, (n,), dtype=torch.int8, device="cuda")
    c = torch.empty_like(a)
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    t_torch, s_torch = repeated(lambda: torch.add(a, b, out=c), reps)
    t_copy, s_copy = repeated(lambda: c.copy_(a), reps)
    t_copy3 = t_copy * 1.5
    for quants in QUANTS:  # the statement's own form, then the gated one
        op = ops.prepare_add(elems, *quants, ops.AddOptions())

        def run():
            _lib.check(L.mf_op_run2(op._h, a.data_ptr(), b.data_ptr(), BATCH, c.data_ptr(), stream))
        name = op.kernel
        t_add, s_add = repeated(run, reps)
        fast = c.clone()
        op.set_generic(True)
        run()
        same = bool(torch.equal(c, fast))
        del fast
        report(H, W, C, n, name, t_add, s_add, t_torch, s_torch, t_copy3, s_copy, same)


def report(H, W, C, n, name, t_add, s_add, t_torch, s_torch, t_copy3, s_copy, same):
    print("%3dx%3dx%3d batch %d (%6.1f MB per operand)  %-12s %8.4f ms (spread %.3f)  torch.add %8.4f ms (spread %.3f)  x%5.2f  "
          "copy x 3/2 %8.4f ms (spread %.3f)  x%5.2f  hbm_frac %.3f (%.2f TB/s)  same=%s" % (
              H, W, C, BATCH, n / 1e6, name, t_add, s_add, t_torch, s_torch, t_add / t_torch, t_copy3, s_copy, t_add / t_copy3,
              3 * n / (t_add * 1e-3) / HBM, 3 * n / (t_add * 1e-3) / 1e12, same), flush=True)


def model(reps):
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    assert torch.cuda.is_available(), "needs the GPU"
    res = {}
    for residual in (True, False):
        m = mf.Model(tw.inverted_residual_net(np.random.default_rng(31), MODEL_SHAPE, MODEL_BLOCKS, residual=residual))
        m.prepare(MODEL_BATCH)
        x = torch.randint(-128, 128, (MODEL_BATCH, m.input_elems), dtype=torch.int8, device="cuda")
        out = m.run_quantized(x).clone()
        names = [m.op(i)["kernel"] for i in range(m.num_ops)]
        t, s = repeated(lambda: m.run_quantized(x, out=out), reps)
        _, per = m.time_device(x, out, MODEL_BATCH, warmup=2, iters=reps, per_op=True)
        adds = [per[i] for i in range(m.num_ops) if m.op(i)["kind"] == 0]
        res[residual] = t
        print("inverted_residual_net %s batch %d residual=%-5s %8.4f ms (spread %.3f)  adds %d: %s ms  launches: %s" % (
            "x".join(map(str, MODEL_SHAPE)), MODEL_BATCH, residual, t, s, len(adds), " ".join("%.4f" % v for v in adds),
            "+".join(n.split("<")[0] for n in names if n and not n.startswith("("))), flush=True)
    print("the adds cost %.4f ms of %.4f (%.1f %%)" % (res[True] - res[False], res[True], 100.0 * (res[True] - res[False]) / res[True]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", type=int, default=-1, help="run this size in this process (what the parent starts per size)")
    ap.add_argument("--model", action="store_true", help="a whole residual model against the same blocks without the adds")
    a = ap.parse_args()
    if a.only >= 0:
        return one(a.only, a.reps)
    if a.model and os.environ.get("TIME_ADD_CHILD"):
        return model(a.reps)
    cases = [["--model"]] if a.model else [["--only", str(i)] for i in range(len(SIZES))]
    for args in cases:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps)] + args, timeout=STEP_TIMEOUT,
                               env=dict(os.environ, TIME_ADD_CHILD="1"))
        except subprocess.TimeoutExpired:
            sys.exit("case %s ran into its %d s limit: nothing more is started" % (" ".join(args), STEP_TIMEOUT))
        if r.returncode != 0:
            sys.exit("case %s ended with status %d: nothing more is started" % (" ".join(args), r.returncode))


if __name__ == "__main__":
    main()
