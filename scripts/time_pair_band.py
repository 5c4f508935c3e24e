#!/usr/bin/env python3
"""GPU box: DepthwiseConv2D 3x3 + Conv2D 1x1 pairs too large for chain_rt as one pair_band_rt launch (k_pair_band.hip) against
the same model with fusion off (dw3x3_rt + pw_rt / conv_gemm_rt: what ran before the group existed), in the same process, back
to back.

    python scripts/time_pair_band.py [--reps 20] [--only 3] [--deep]

--deep times the second shape set instead: pairs of 256 < C <= 512 input channels, pair_band_deep_rt (k_pair_band_deep.hip).

One line per shape: the median of --reps runs of each path, each timed with HIP events after warm-up, the spread of the repeats
((max - min) / median of each path), their ratio, and hbm_frac = batch x (H W C + OH OW N) bytes (the least a launch must move) over
the fused time against 8.0 TB/s (the MI355X spec figure; a plain copy reaches 5.3 - 5.6 TB/s, profiles/r03/hbm_copy_ceiling.txt).
Every shape runs in a child process of its own under a time limit, so that one shape's trouble ends that shape only; the outputs
of the two paths are compared too."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM = 8.0e12
# (H, W, C, stride, N, batch): the first six pairs of a MobileNet-v1 at 224 x 224, then three sizes between them and chain_rt's limit
SHAPES = [(112, 112, 32, 1, 64, 1024), (112, 112, 64, 2, 128, 1024), (56, 56, 128, 1, 128, 1024), (56, 56, 128, 2, 256, 1024),
          (28, 28, 256, 1, 256, 1024), (28, 28, 256, 2, 512, 1024), (96, 96, 32, 1, 64, 4096), (64, 64, 64, 2, 128, 4096),
          (48, 48, 128, 1, 128, 4096)]
# --deep: the 512-channel pairs of a MobileNet-v1 at 224 .. 96 input, the pair behind them at 256 input, widths 0.75 and 0.625, a
# one-pass 1x1 and an odd image
DEEP_SHAPES = [(14, 14, 512, 1, 512, 4096), (12, 12, 512, 1, 512, 4096), (10, 10, 512, 1, 512, 4096), (8, 8, 512, 1, 512, 4096),
               (6, 6, 512, 1, 512, 4096), (16, 16, 512, 2, 1024, 4096), (14, 14, 384, 1, 384, 4096), (14, 14, 320, 1, 320, 4096),
               (14, 14, 512, 1, 256, 4096), (7, 7, 512, 1, 512, 4096)]
STEP_TIMEOUT = 240  # seconds per shape


def times_ms(fn, reps, warm=3):
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
    return float(np.median(ts)), float((max(ts) - min(ts)) / np.median(ts))


def one(idx, reps, shapes):
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    assert torch.cuda.is_available(), "needs the GPU"
    H, W, C, S, N, batch = shapes[idx]
    m = mf.Model(tw.conv_net(np.random.default_rng(idx), (H, W, C), [("dw", 0, 3, S), ("conv", N, 1, 1)], act_scale=6.0 / 255.0))
    m.prepare(batch)
    x = torch.randint(-128, 128, (batch, m.input_elems), dtype=torch.int8, device="cuda")
    out = m.run_quantized(x).clone()
    ref = out.clone()
    fused_names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    t_fused, s_fused = times_ms(lambda: m.run_quantized(x, out=out), reps)
    assert torch.equal(out, ref)
    m.set_fusion(False)
    names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    t_ops, s_ops = times_ms(lambda: m.run_quantized(x, out=out), reps)
    same = bool(torch.equal(out, ref))
    m.set_fusion(True)
    OH, OW = -(-H // S), -(-W // S)
    hb = batch * (H * W * C + OH * OW * N)
    print("%3dx%3dx%3d%s -> %-4d batch %5d  %-34s %8.4f ms (spread %.3f)  fusion off %8.4f ms (spread %.3f; %s)  x%5.2f  hbm_frac %.3f (%.2f TB/s)  same=%s" % (
        H, W, C, "s2" if S == 2 else "  ", N, batch, fused_names[0], t_fused, s_fused, t_ops, s_ops, "+".join(n for n in names if n and not n.startswith("(")),
        t_ops / t_fused, hb / (t_fused * 1e-3) / HBM, hb / (t_fused * 1e-3) / 1e12, same), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", type=int, default=-1, help="run this shape in this process (what the parent starts per shape)")
    ap.add_argument("--deep", action="store_true", help="the 256 < C <= 512 shape set (pair_band_deep_rt)")
    a = ap.parse_args()
    shapes = DEEP_SHAPES if a.deep else SHAPES
    if a.only >= 0:
        return one(a.only, a.reps, shapes)
    for idx in range(len(shapes)):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--only", str(idx)] + (["--deep"] if a.deep else []),
                               timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            sys.exit("shape %d ran into its %d s limit: nothing more is started" % (idx, STEP_TIMEOUT))
        if r.returncode != 0:
            sys.exit("shape %d ended with status %d: nothing more is started" % (idx, r.returncode))


if __name__ == "__main__":
    main()
