#!/usr/bin/env python3
"""GPU box: Conv2D / DepthwiseConv2D with dilation factors (k_conv_dil.hip conv_dil_rt, k_dw_gemm.hip dw_gemm_rt) against three yardsticks.

    python scripts/time_dilated.py [--batch 4096] [--gen-batch 256] [--reps 20] [--root DIR]

Per case, one line:
  fast     the dilated operator on its fast kernel at --batch images
  (a)      the same operator on the generic kernel (set_generic) at --gen-batch images, scaled to the batch; parity of the two checked
  (b)      what a tree without the feature can run: the undilated conv_2d / depthwise_conv_2d with the zero-stuffed KeH x KeW filter
           (zero filter zero points: the same accumulator, plus the dead multiply-adds); its output is checked against the fast kernel's.
           --root names the tree whose library runs it (default: this one -- undilated operators route as on the parent commit)
  (c)      the undilated sibling of the shape (same filter, factors 1 x 1) on conv_gemm_rt / dw_gemm_rt or whatever it routes to: what
           the plane staging and the wider halo cost

    python scripts/time_dilated.py --model [--model-batch 16384]     # tools/tflite_writer.tcn(T = 128, C = 32, 32 filters, d = 1, 2, 4, 8):
                                                                     # per-operator kernel names and times, the total

Every figure is the median of --reps samples of 10 back-to-back launches timed with HIP events after warm-up, in three repeats: the median of the three medians and
their spread ((max - min) / median).  Every case runs in a child process of its own under a time limit; the first that fails ends the run."""
import argparse
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#         name            H   W    C   N   KH KW dh dw same  dw?
CASES = [("tcn-d1",        1, 128, 32, 32, 1, 3, 1, 1, True, False),
         ("tcn-d2",        1, 128, 32, 32, 1, 3, 1, 2, True, False),
         ("tcn-d4",        1, 128, 32, 32, 1, 3, 1, 4, True, False),
         ("tcn-d8",        1, 128, 32, 32, 1, 3, 1, 8, True, False),
         ("conv-32x32x32", 32, 32, 32, 64, 3, 3, 2, 2, True, False),
         ("stem-c4",       32, 32, 4,  16, 3, 3, 2, 2, True, False),
         ("dw-28x28x16",   28, 28, 16, 16, 3, 3, 2, 2, True, True),
         ("dw-d3x3",       28, 28, 16, 16, 3, 3, 3, 3, True, True),      # 5.4x the taps: the dilated dw_gemm_rt
         ("dw-c24-d3x3",   28, 28, 24, 24, 3, 3, 3, 3, True, True),      # ... where the stuffed 7x7 has no dw_mm_rt (C % 16 != 0)
         ("conv-d3x3",     32, 32, 32, 64, 3, 3, 3, 3, True, False)]     # 5.4x on a 3x3 Conv2D
STEP_TIMEOUT = 300
REPEATS = 3


INNER = 10  # launches per sample, back to back between one pair of events: a launch of 0.05 ms alone is mostly its own overhead


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
    name, H, W, C, N, KH, KW, dh, dw, same, depthwise = CASES[idx]
    rng = np.random.default_rng(200 + idx)
    w = rng.integers(-127, 128, (KH, KW, N) if depthwise else (N, KH, KW, C)).astype(np.int8)
    c0 = rng.uniform(-30, 30, N).astype(np.float32)
    c1 = (rng.uniform(0.8, 1.25, N) * 190.0 / (74.0 * 73.3 * np.sqrt(KH * KW * (1 if depthwise else C)))).astype(np.float32)
    izp, ozp, osc, z = int(rng.integers(-20, 21)), int(rng.integers(-20, 21)), 0.0235294122, np.zeros(N, np.int8)
    o = mf.ops
    cls, prep = (o.DepthwiseConv2DOptions, o.prepare_depthwise_conv_2d) if depthwise else (o.Conv2DOptions, o.prepare_conv_2d)
    pad = mf.TensorViewPadding(0 if same else 1)
    x = torch.randint(-128, 128, (a.batch, H, W, C), dtype=torch.int8, device="cuda")
    # (b) the zero-stuffed filter, undilated; (c) the sibling.  Neither needs the dilation field, so both run on a tree without it
    keh, kew = (KH - 1) * dh + 1, (KW - 1) * dw + 1
    ws = np.zeros((keh, kew, N) if depthwise else (N, keh, kew, C), np.int8)
    if depthwise:
        ws[::dh, ::dw, :] = w
    else:
        ws[:, ::dh, ::dw, :] = w
    stuffed = prep((H, W, C), ws, z, izp, osc, ozp, cls(mf.FusedActivation(0), pad, (1, 1)), (c0, c1), (H, W))
    sib = prep((H, W, C), w, z, izp, osc, ozp, cls(mf.FusedActivation(0), pad, (1, 1)), (c0, c1), (H, W))
    yb = stuffed(x)
    bms, bsp = repeats(lambda: stuffed(x), a.reps)
    cms, csp = repeats(lambda: sib(x), a.reps)
    line = "%-14s | (b) %s %.4f ms (+-%.1f%%) | (c) %s %.4f ms (+-%.1f%%)" % (name, stuffed.kernel, bms, 100 * bsp, sib.kernel, cms, 100 * csp)
    ok = True
    if not a.root and (dh, dw) != (1, 1):
        op = prep((H, W, C), w, z, izp, osc, ozp, cls(mf.FusedActivation(0), pad, (1, 1), (dh, dw)), (c0, c1), (H, W))
        fast_name, y = op.kernel, op(x)
        ms, sp = repeats(lambda: op(x), a.reps)
        op.set_generic(True)
        xg = x[:a.gen_batch]
        ok = bool(torch.equal(op(xg), y[:a.gen_batch])) and bool(torch.equal(y, yb))
        gms, gsp = repeats(lambda: op(xg), a.reps)
        gms *= a.batch / a.gen_batch
        line = "%-14s | fast %s %.4f ms (+-%.1f%%) | (a) %s %.3f ms (+-%.1f%%) x%.1f" % (name, fast_name, ms, 100 * sp, op.kernel, gms, 100 * gsp, gms / ms) + \
               line[14:] + " | fast/(b) x%.2f fast/(c) x%.2f | parity %s" % (bms / ms, cms / ms, "ok" if ok else "MISMATCH")
    print(line)
    return 0 if ok else 1


def run_model(a):
    import torch
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tools"))
    import tflite_writer as tw
    import microflow_rs_amd as mf
    m = mf.model(tw.tcn(np.random.default_rng(7), T=128, C=32, filters=32))
    B = a.model_batch
    m.prepare(B)
    x = torch.randint(-128, 128, (B, 1, 128, 32), dtype=torch.int8, device="cuda")
    y = torch.empty((B, m.output_elems), dtype=torch.int8, device="cuda")
    v = [m.time_device(x, y, B, 3, a.reps, True) for _ in range(REPEATS)]
    tot = [t for t, _ in v]
    print("tcn(T 128, C 32, 32 filters) batch %d: %.3f ms (+-%.1f%%), %.2f M inferences/s" % (B, np.median(tot), 100 * (max(tot) - min(tot)) / np.median(tot), B / np.median(tot) / 1e3))
    for i in range(m.num_ops):
        o = m.op(i)
        print("  %d %-16s %-34s %.3f ms" % (i, o["name"], o["kernel"], float(np.median([per[i] for _, per in v]))))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--gen-batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--root", default=None)
    ap.add_argument("--case", type=int, default=None)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--model-batch", type=int, default=16384)
    a = ap.parse_args()
    if a.model:
        return run_model(a)
    if a.case is not None:
        return run_case(a.case, a)
    for i in range(len(CASES)):
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(i), "--batch", str(a.batch), "--gen-batch", str(a.gen_batch), "--reps", str(a.reps)]
        r = subprocess.run(cmd + (["--root", a.root] if a.root else []), timeout=STEP_TIMEOUT, cwd=HERE)
        if r.returncode != 0:
            print("case %d failed (exit %d): stopping" % (i, r.returncode))
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
