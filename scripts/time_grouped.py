#!/usr/bin/env python3
"""GPU box: grouped Conv2D (k_conv_grp.hip conv_grp_rt) against its yardsticks.

    python scripts/time_grouped.py --mode op    [--batch 4096] [--gen-batch 64] [--reps 20]
        conv_grp_rt at --batch images against conv2d_generic (set_generic) at --gen-batch images scaled to the batch; parity checked
    python scripts/time_grouped.py --mode ops   [--root DIR]
        the block-diagonal dense filter through prepare_conv_2d (zero filter zero points: every element outside a channel's group is 0):
        what a tree without the feature can run -- the YARDSTICK.  --root names the tree whose library runs it (default: this one)
    python scripts/time_grouped.py --mode model [--model-batch 1024]
        tools/tflite_writer.resnext (56x56x32 input, width 128, G = 32): per-operator kernel names and times, the total

Every figure is the median of --reps samples of 10 back-to-back launches timed with HIP events after warm-up, in three repeats: the
median of the three medians and their spread ((max - min) / median).  Every case runs in a child process of its own under a time
limit; the first that fails ends the run."""
import argparse
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#         name               H   W   C    N   K  G
CASES = [("resnext-56x128",  56, 56, 128, 128, 3, 32),
         ("resnext-28x256",  28, 28, 256, 256, 3, 32),
         ("resnext-14x512",  14, 14, 512, 512, 3, 32),
         ("shuffle-28x240",  28, 28, 240, 240, 1, 3),
         ("shuffle-14x480",  14, 14, 480, 480, 1, 8),
         ("conv-32x64-g2",   32, 32, 64,  64,  3, 2),
         ("conv-32x64-g4",   32, 32, 64,  64,  3, 4)]
STEP_TIMEOUT = 300
REPEATS = 3
INNER = 10  # launches per sample, back to back between one pair of events


def median_ms(fn, reps, warm=3):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(INNER):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / INNER)
    return float(np.median(ts))


def repeats(fn, reps):
    v = [median_ms(fn, reps) for _ in range(REPEATS)]
    return float(np.median(v)), float((max(v) - min(v)) / np.median(v))


def run_case(idx, a):
    sys.path.insert(0, a.root or HERE)
    import torch
    import microflow_rs_amd as mf
    name, H, W, C, N, K, G = CASES[idx]
    Cg, Ng = C // G, N // G
    rng = np.random.default_rng(300 + idx)
    w = rng.integers(-127, 128, (N, K, K, Cg)).astype(np.int8)
    c0 = rng.uniform(-30, 30, N).astype(np.float32)
    c1 = (rng.uniform(0.8, 1.25, N) * 190.0 / (74.0 * 73.3 * np.sqrt(K * K * Cg))).astype(np.float32)
    izp, ozp, osc, z = int(rng.integers(-20, 21)), int(rng.integers(-20, 21)), 0.0235294122, np.zeros(N, np.int8)
    o = mf.ops
    torch.manual_seed(idx)
    x = torch.randint(-128, 128, (a.batch, H, W, C), dtype=torch.int8, device="cuda")
    if a.mode == "ops":   # the dense twin: needs no groups field, so it runs on a tree without the feature
        wd = np.zeros((N, K, K, C), np.int8)
        for n in range(N):
            wd[n, :, :, (n // Ng) * Cg:(n // Ng + 1) * Cg] = w[n]
        op = o.prepare_conv_2d((H, W, C), wd, z, izp, osc, ozp, o.Conv2DOptions(mf.FusedActivation(0), mf.TensorViewPadding(0), (1, 1)), (c0, c1), (H, W))
        y = op(x)
        ms, sp = repeats(lambda: op(x), a.reps)
        print("%-16s | twin %-22s %.4f ms (+-%.1f%%) | checksum %d" % (name, op.kernel, ms, 100 * sp, int(y.to(torch.int64).sum())))
        return 0
    op = o.prepare_conv_2d((H, W, C), w, z, izp, osc, ozp, o.Conv2DOptions(mf.FusedActivation(0), mf.TensorViewPadding(0), (1, 1), (1, 1), G), (c0, c1), (H, W))
    fast_name, y = op.kernel, op(x)
    ms, sp = repeats(lambda: op(x), a.reps)
    op.set_generic(True)
    xg = x[:a.gen_batch]
    ok = bool(torch.equal(op(xg), y[:a.gen_batch]))
    gms, gsp = repeats(lambda: op(xg), a.reps)
    gms *= a.batch / a.gen_batch
    print("%-16s | fast %-22s %.4f ms (+-%.1f%%) | generic %.3f ms (+-%.1f%%) x%.1f | checksum %d | parity %s"
          % (name, fast_name, ms, 100 * sp, gms, 100 * gsp, gms / ms, int(y.to(torch.int64).sum()), "ok" if ok else "MISMATCH"))
    return 0 if ok else 1


def run_model(a):
    import torch
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tools"))
    import tflite_writer as tw
    import microflow_rs_amd as mf
    m = mf.model(tw.resnext(np.random.default_rng(7), side=56, C=32, stem=64, blocks=((1, 128, 256), (2, 256, 512)), groups=32, classes=10))
    B = a.model_batch
    m.prepare(B)
    x = torch.randint(-128, 128, (B, 56, 56, 32), dtype=torch.int8, device="cuda")
    y = torch.empty((B, m.output_elems), dtype=torch.int8, device="cuda")
    v = [m.time_device(x, y, B, 3, a.reps, True) for _ in range(REPEATS)]
    tot = [t for t, _ in v]
    print("resnext(56x56x32, widths 128 / 256, G 32) batch %d: %.3f ms (+-%.1f%%), %.2f k inferences/s" % (B, np.median(tot), 100 * (max(tot) - min(tot)) / np.median(tot), B / np.median(tot)))
    for i in range(m.num_ops):
        o = m.op(i)
        print("  %d %-16s g%-3d %-34s %.3f ms" % (i, o["name"], o["groups"], o["kernel"], float(np.median([per[i] for _, per in v]))))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("op", "ops", "model"), default="op")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--gen-batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--root", default=None)
    ap.add_argument("--case", type=int, default=None)
    ap.add_argument("--model-batch", type=int, default=1024)
    a = ap.parse_args()
    if a.case is not None:
        return run_model(a) if a.mode == "model" else run_case(a.case, a)
    for i in range(1 if a.mode == "model" else len(CASES)):   # (the model is one case, in a child of its own like the others)
        cmd = [sys.executable, os.path.abspath(__file__), "--mode", a.mode, "--case", str(i), "--batch", str(a.batch), "--gen-batch", str(a.gen_batch), "--reps", str(a.reps),
               "--model-batch", str(a.model_batch)]
        r = subprocess.run(cmd + (["--root", a.root] if a.root else []), timeout=STEP_TIMEOUT, cwd=HERE)
        if r.returncode != 0:
            print("case %d failed (exit %d): stopping" % (i, r.returncode))
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
