#!/usr/bin/env python3
"""GPU box: RESIZE_NEAREST_NEIGHBOR + Conv2D in one launch (k_upconv.hip upconv_rt) against its yardsticks.

    python scripts/time_upconv.py --mode op    [--batch 4096] [--gen-batch 64] [--reps 20]
        upconv_rt at --batch images against upconv_generic (set_generic) at --gen-batch images scaled to the batch, parity checked; and
        this tree's two launches: resize_nn_c4, then the convolution's own kernel on the resized tensor (parity checked)
    python scripts/time_upconv.py --mode ops   [--root DIR]
        the input resized with torch.repeat_interleave and fed to conv_2d through prepare_conv_2d without the upsample field: what a tree
        without the feature can run -- the YARDSTICK.  The convolution's launch and the torch resize are timed apart.  --root names the
        tree whose library runs it (default: this one)
    python scripts/time_upconv.py --mode model [--model-batch 1024]
        tools/tflite_writer.upsample_autoencoder((64, 64, 4), (16, 32, 64)) and unet1((64, 64, 4), (16, 32)): per-operator kernel names
        and times, the totals; under MF_DEV=1 MF_NO_UPCONV=1 the two-launch route of this tree

Every figure is the median of --reps samples of 10 back-to-back launches timed with HIP events after warm-up, in three repeats: the
median of the three medians and their spread ((max - min) / median).  Every case runs in a child process of its own under a time
limit; the first that fails ends the run."""
import argparse
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#         name              H   W   C    N    K  factor      (of the source)
CASES = [("8x8x64-32",      8,  8,  64,  32,  3, 2),
         ("16x16x32-16",    16, 16, 32,  16,  3, 2),
         ("32x32x16-16",    32, 32, 16,  16,  3, 2),
         ("16x16x64-64",    16, 16, 64,  64,  3, 2),
         ("8x8x128-128",    8,  8,  128, 128, 3, 2),
         ("16x16x32-32-k5", 16, 16, 32,  32,  5, 2),
         ("8x8x64-64-x4",   8,  8,  64,  64,  3, 4)]
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
    name, H, W, C, N, K, F = CASES[idx]
    UH, UW = H * F, W * F
    rng = np.random.default_rng(400 + idx)
    w = rng.integers(-127, 128, (N, K, K, C)).astype(np.int8)
    c0 = rng.uniform(-30, 30, N).astype(np.float32)
    c1 = (rng.uniform(0.8, 1.25, N) * 190.0 / (74.0 * 73.3 * np.sqrt(K * K * C))).astype(np.float32)
    izp, ozp, osc, z = int(rng.integers(-20, 21)), int(rng.integers(-20, 21)), 0.0235294122, np.zeros(N, np.int8)
    o = mf.ops
    base = (mf.FusedActivation(0), mf.TensorViewPadding(0), (1, 1))
    torch.manual_seed(idx)
    x = torch.randint(-128, 128, (a.batch, H, W, C), dtype=torch.int8, device="cuda")
    conv = o.prepare_conv_2d((UH, UW, C), w, z, izp, osc, ozp, o.Conv2DOptions(*base), (c0, c1), (UH, UW))   # (no upsample field: any tree)
    if a.mode == "ops":
        up = lambda: x.repeat_interleave(F, 1).repeat_interleave(F, 2)   # noqa: E731
        xu = up()
        y = conv(xu)
        ms, sp = repeats(lambda: conv(xu), a.reps)
        ums, usp = repeats(up, a.reps)
        print("%-16s | conv %-16s %.4f ms (+-%.1f%%) | torch resize %.4f ms (+-%.1f%%) | checksum %d"
              % (name, conv.kernel, ms, 100 * sp, ums, 100 * usp, int(y.to(torch.int64).sum())))
        return 0
    op = o.prepare_conv_2d((H, W, C), w, z, izp, osc, ozp, o.Conv2DOptions(*base, upsample=(F, F)), (c0, c1), (UH, UW))
    rs = o.prepare_resize_nearest((H, W, C), (F, F))
    fast_name, y = op.kernel, op(x)
    ms, sp = repeats(lambda: op(x), a.reps)
    ok = bool(torch.equal(conv(rs(x)), y))
    rms, rsp = repeats(lambda: rs(x), a.reps)
    xu = rs(x)
    cms, csp = repeats(lambda: conv(xu), a.reps)
    op.set_generic(True)
    xg = x[:a.gen_batch]
    ok = ok and bool(torch.equal(op(xg), y[:a.gen_batch]))
    gms, gsp = repeats(lambda: op(xg), a.reps)
    gms *= a.batch / a.gen_batch
    gbs = a.batch * (H * W * C + UH * UW * N) / ms / 1e6
    tmacs = a.batch * UH * UW * N * K * K * C / ms / 1e9
    print("%-16s | %-14s %.4f ms (+-%.1f%%) %.0f GB/s %.1f TMAC/s | generic %.2f ms (+-%.1f%%) | two launches: %s %.4f ms (+-%.1f%%) + %s %.4f ms (+-%.1f%%) | conv alone / fused x%.2f | checksum %d | parity %s"
          % (name, fast_name, ms, 100 * sp, gbs, tmacs, gms, 100 * gsp, rs.kernel, rms, 100 * rsp, conv.kernel, cms, 100 * csp, cms / ms,
             int(y.to(torch.int64).sum()), "ok" if ok else "MISMATCH"))
    return 0 if ok else 1


def run_model(idx, a):
    import torch
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tools"))
    import tflite_writer as tw
    import microflow_rs_amd as mf
    name, blob = [("upsample_autoencoder((64, 64, 4), (16, 32, 64))", lambda: tw.upsample_autoencoder(np.random.default_rng(7), (64, 64, 4), (16, 32, 64))),
                  ("unet1((64, 64, 4), (16, 32))", lambda: tw.unet1(np.random.default_rng(7), (64, 64, 4), (16, 32)))][idx]
    m = mf.model(blob())
    B = a.model_batch
    m.prepare(B)
    x = torch.randint(-128, 128, (B, 64, 64, 4), dtype=torch.int8, device="cuda")
    y = torch.empty((B, m.output_elems), dtype=torch.int8, device="cuda")
    v = [m.time_device(x, y, B, 3, a.reps, True) for _ in range(REPEATS)]
    tot = [t for t, _ in v]
    print("%s batch %d: %.3f ms (+-%.1f%%), %.2f k inferences/s" % (name, B, np.median(tot), 100 * (max(tot) - min(tot)) / np.median(tot), B / np.median(tot)))
    for i in range(m.num_ops):
        o = m.op(i)
        print("  %d %-24s %-34s %.3f ms" % (i, o["name"], o["kernel"], float(np.median([per[i] for _, per in v]))))
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
        return run_model(a.case, a) if a.mode == "model" else run_case(a.case, a)
    for i in range(2 if a.mode == "model" else len(CASES)):
        cmd = [sys.executable, os.path.abspath(__file__), "--mode", a.mode, "--case", str(i), "--batch", str(a.batch), "--gen-batch", str(a.gen_batch), "--reps", str(a.reps),
               "--model-batch", str(a.model_batch)]
        r = subprocess.run(cmd + (["--root", a.root] if a.root else []), timeout=STEP_TIMEOUT, cwd=HERE)
        if r.returncode != 0:
            print("case %d failed (exit %d): stopping" % (i, r.returncode))
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
