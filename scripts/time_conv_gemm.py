#!/usr/bin/env python3
"""GPU box: Conv2D shapes that ran conv2d_generic before conv_gemm_rt (k_conv_gemm.hip) -- the new kernel against conv2d_generic
(set_generic), one line per shape.

    python scripts/time_conv_gemm.py [--batch 4096] [--reps 10]

ms is the median of --reps launches at --batch images, each timed with HIP events after warm-up; conv2d_generic is timed on
--gbatch images (it is 2 - 3 orders of magnitude slower) and scaled to --batch.  hbm_frac is batch x (H W C + OH OW N) bytes (the
least a launch must move) over time against 8.0 TB/s; TMAC/s counts batch OH OW N KH KW C real multiply-adds.  same: the fast
path's first --gbatch images equal conv2d_generic's bytes."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import microflow_rs_amd as mf  # noqa: E402
from microflow_rs_amd import _lib  # noqa: E402

HBM = 8.0e12
# H, W, C, N, KH, KW, stride, filter zero points: the shapes of the table in DESIGN 4.10 (ImageNet stems, few-channel inputs
# with many outputs, C % 16 != 0, weights beyond conv_mm_rt's 96 KiB, N % 4 != 0)
SHAPES = [(224, 224, 3, 32, 3, 3, 2, False), (224, 224, 3, 64, 7, 7, 2, False), (128, 128, 3, 16, 3, 3, 1, False),
          (32, 32, 3, 96, 3, 3, 1, False), (16, 16, 24, 24, 3, 3, 1, False), (16, 16, 20, 40, 3, 3, 1, False),
          (16, 16, 24, 24, 1, 1, 2, False), (8, 8, 128, 128, 3, 3, 1, False), (8, 8, 96, 96, 3, 3, 1, False),
          (8, 8, 128, 256, 3, 3, 2, False), (4, 4, 512, 512, 3, 3, 1, False), (8, 8, 64, 10, 3, 3, 1, False),
          (16, 16, 24, 24, 3, 3, 1, True)]


def median_ms(fn, reps, warm=2):
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


def case(H, W, C, N, KH, KW, s, wz, batch, gbatch, reps):
    rng = np.random.default_rng(H * 31 + C * 7 + N)
    OH, OW = -(-H // s), -(-W // s)
    f = rng.integers(-128, 128, (N, KH, KW, C)).astype(np.int8)
    zp = rng.integers(-20, 20, N).astype(np.int8) if wz else np.zeros(N, np.int8)
    c0 = rng.uniform(-30, 30, N).astype(np.float32)
    c1 = (rng.uniform(0.5, 1.5, N) * 40.0 / (5476.0 * np.sqrt(KH * KW * C))).astype(np.float32)
    opts = mf.ops.Conv2DOptions(mf.FusedActivation(1), mf.TensorViewPadding.SAME, (s, s))
    op = mf.ops.prepare_conv_2d((H, W, C), f, zp, -3, 0.0235294122, 5, opts, (c0, c1), (OH, OW))
    x = torch.randint(-128, 128, (batch, H, W, C), dtype=torch.int8, device="cuda")
    y = torch.empty(batch * OH * OW * N, dtype=torch.int8, device="cuda")
    yg = torch.empty(gbatch * OH * OW * N, dtype=torch.int8, device="cuda")
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    kern = op.kernel
    t_new = median_ms(lambda: _lib.check(L.mf_op_run(op._h, x.data_ptr(), batch, y.data_ptr(), st)), reps)
    op.set_generic(True)
    t_gen = median_ms(lambda: _lib.check(L.mf_op_run(op._h, x.data_ptr(), gbatch, yg.data_ptr(), st)), max(3, reps // 3), warm=1)
    op.set_generic(False)
    same = bool(torch.equal(y[:yg.numel()], yg))
    t_gen *= batch / gbatch
    hb = batch * (H * W * C + OH * OW * N)
    mac = batch * OH * OW * N * KH * KW * C
    print("%3dx%3dx%3d -> %3d %dx%d s%d%s batch %5d  %-18s %9.3f ms  conv2d_generic %10.1f ms (scaled)  x%7.1f  %7.1f GB/s  "
          "hbm_frac %.3f  %6.1f TMAC/s  same=%s" % (H, W, C, N, KH, KW, s, " wzp" if wz else "    ", batch, kern, t_new, t_gen,
                                                    t_gen / t_new, hb / (t_new * 1e-3) / 1e9, hb / (t_new * 1e-3) / HBM,
                                                    mac / (t_new * 1e-3) / 1e12, same), flush=True)
    return kern, t_gen / t_new, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--gbatch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    bad = []
    for sh in SHAPES:
        H = sh[0]
        gb = min(a.gbatch, 8) if H >= 128 else a.gbatch
        kern, speed, same = case(*sh, a.batch, gb, a.reps)
        if not kern.startswith("conv_gemm_rt") or speed < 10.0 or not same:
            bad.append(sh)
    print("shapes missing the floor (conv_gemm_rt, >= 10x conv2d_generic, bit-exact):", bad if bad else "none")


if __name__ == "__main__":
    main()
