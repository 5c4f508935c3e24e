#!/usr/bin/env python3
"""GPU box: classifier heads AveragePool2D -> Reshape -> FullyConnected (-> Softmax) as one pool_fc_chain launch (k_pool_fc.hip)
against the same model with fusion off (avgpool_c4 + fc_rt / fc_generic / fc_rowwave + softmax_table: what ran before the group
existed), in the same process, back to back.

    python scripts/time_pool_fc.py [--reps 20] [--only 3]

One line per shape: the median of --reps runs of each path, each timed with HIP events after warm-up, their ratio, and hbm_frac
= batch x (H W C + N_last) bytes (the least a launch must move) over the fused time against 8.0 TB/s (the MI355X spec figure; a
plain copy reaches 5.3 - 5.6 TB/s, profiles/r03/hbm_copy_ceiling.txt).  Every shape runs in a child process of its own under a
time limit, so that one shape's trouble ends that shape only; the outputs of the two paths are compared too."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM = 8.0e12
# (H, W, C, FullyConnected sizes, softmax, batch)
SHAPES = [(2, 2, 256, (10,), True, 65536), (3, 3, 256, (2,), True, 65536), (4, 4, 256, (10,), True, 65536), (14, 14, 16, (20,), True, 65536),
          (7, 7, 64, (10,), True, 65536), (7, 7, 1024, (10,), True, 16384), (8, 8, 128, (100, 10), True, 65536)]
STEP_TIMEOUT = 240  # seconds per shape


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


def one(idx, reps):
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    assert torch.cuda.is_available(), "needs the GPU"
    H, W, C, sizes, softmax, batch = SHAPES[idx]
    m = mf.Model(tw.pool_head(np.random.default_rng(idx), (H, W, C), sizes, softmax=softmax))
    m.prepare(batch)
    x = torch.randint(-128, 128, (batch, m.input_elems), dtype=torch.int8, device="cuda")
    out = m.run_quantized(x).clone()
    ref = out.clone()
    fused_names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    t_fused = median_ms(lambda: m.run_quantized(x, out=out), reps)
    assert torch.equal(out, ref)
    m.set_fusion(False)
    names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    t_ops = median_ms(lambda: m.run_quantized(x, out=out), reps)
    same = bool(torch.equal(out, ref))
    m.set_fusion(True)
    hb = batch * (H * W * C + sizes[-1])
    print("%2dx%2dx%4d -> %-8s batch %6d  %-20s %8.4f ms  fusion off %8.4f ms (%s)  x%5.2f  hbm_frac %.3f (%.2f TB/s)  same=%s" % (
        H, W, C, "-".join(map(str, sizes)), batch, fused_names[0], t_fused, t_ops, "+".join(n for n in names if n and not n.startswith("(")),
        t_ops / t_fused, hb / (t_fused * 1e-3) / HBM, hb / (t_fused * 1e-3) / 1e12, same), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", type=int, default=-1, help="run this shape in this process (what the parent starts per shape)")
    a = ap.parse_args()
    if a.only >= 0:
        return one(a.only, a.reps)
    for idx in range(len(SHAPES)):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--only", str(idx)], timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            sys.exit("shape %d ran into its %d s limit: nothing more is started" % (idx, STEP_TIMEOUT))
        if r.returncode != 0:
            sys.exit("shape %d ended with status %d: nothing more is started" % (idx, r.returncode))


if __name__ == "__main__":
    main()
