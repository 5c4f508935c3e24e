#!/usr/bin/env python3
"""GPU box: DepthwiseConv2D shapes that ran dwconv_generic before dw_gemm_rt (k_dw_gemm.hip) and one-channel depthwise layers that
now run conv_gemm_rt -- the new kernel against dwconv_generic (set_generic), one line per shape.

    python scripts/time_dw_gemm.py [--batch 16384] [--reps 10] [--out profiles/r07/time_dw_gemm.txt]

ms is the median of --reps launches at --batch images, each timed with HIP events after warm-up; dwconv_generic is timed on --gbatch
images (it is one to two orders of magnitude slower) and scaled to --batch.  hbm_frac is batch x (H W C + OH OW N) bytes (the least
a launch must move) over time against 8.0 TB/s.  For the rows with filter zero points and C % 16 == 0, dw_mm_rt is timed on the
same shape without them (the price of the zero-point term).  same: the fast path's first --gbatch images equal dwconv_generic's."""
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
# H, W, C, N, KH, KW, stride, SAME, filter zero points, u8: the table of DESIGN 4.11
SHAPES = [(56, 56, 72, 72, 5, 5, 2, True, False, False), (28, 28, 120, 120, 5, 5, 1, True, False, False),
          (48, 48, 8, 8, 5, 5, 1, True, False, False), (24, 24, 24, 24, 7, 7, 1, True, False, False),
          (32, 32, 6, 6, 3, 3, 1, True, False, False), (32, 32, 3, 3, 3, 3, 1, True, True, False),
          (7, 7, 36, 36, 3, 3, 1, True, False, False), (24, 24, 32, 32, 5, 5, 1, True, True, False),
          (28, 28, 120, 120, 5, 5, 1, True, True, True), (20, 20, 16, 16, 3, 3, 1, False, True, False),
          (224, 224, 1, 16, 5, 5, 2, True, True, False)]


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


def prepare(H, W, C, N, K, s, same, wz, u8, seed):
    rng = np.random.default_rng(seed)
    dt = np.uint8 if u8 else np.int8
    lo, hi = (0, 256) if u8 else (-128, 128)
    OH, OW = (-(-H // s), -(-W // s)) if same else ((H - K) // s + 1, (W - K) // s + 1)
    w = rng.integers(lo, hi, (K, K, N)).astype(dt)
    zp = (rng.integers(-20, 20, N) + (128 if u8 else 0)).astype(dt) if wz else np.full(N, 128 if u8 else 0, dt)
    c0 = rng.uniform(-30, 30, N).astype(np.float32)
    c1 = (rng.uniform(0.5, 1.5, N) * 40.0 / (5476.0 * np.sqrt(K * K))).astype(np.float32)
    opts = mf.ops.DepthwiseConv2DOptions(mf.FusedActivation(1), mf.TensorViewPadding(0 if same else 1), (s, s))
    op = mf.ops.prepare_depthwise_conv_2d((H, W, C), w, zp, lo + 3, 0.0235294122, lo + 5, opts, (c0, c1), (OH, OW))
    return op, OH, OW


def case(H, W, C, N, K, KW, s, same, wz, u8, batch, gbatch, reps, out):
    assert K == KW  # (square filters in this table)
    op, OH, OW = prepare(H, W, C, N, K, s, same, wz, u8, H * 31 + C * 7 + N)
    x = torch.randint(-128, 128, (batch, H, W, C), dtype=torch.int8, device="cuda")
    y = torch.empty(batch * OH * OW * N, dtype=torch.int8, device="cuda")
    yg = torch.empty(gbatch * OH * OW * N, dtype=torch.int8, device="cuda")
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    kern = op.kernel
    t_new = median_ms(lambda: _lib.check(L.mf_op_run(op._h, x.data_ptr(), batch, y.data_ptr(), st)), reps)
    op.set_generic(True)
    t_gen = median_ms(lambda: _lib.check(L.mf_op_run(op._h, x.data_ptr(), gbatch, yg.data_ptr(), st)), max(3, reps // 3), warm=1)
    op.set_generic(False)
    same_bytes = bool(torch.equal(y[:yg.numel()], yg))
    t_gen *= batch / gbatch
    hb = batch * (H * W * C + OH * OW * N)
    extra = ""
    if wz and C % 16 == 0 and C == N:  # the same shape without filter zero points: dw_mm_rt
        op0, _, _ = prepare(H, W, C, N, K, s, same, False, u8, H * 31 + C * 7 + N)
        t0 = median_ms(lambda: _lib.check(L.mf_op_run(op0._h, x.data_ptr(), batch, y.data_ptr(), st)), reps)
        extra = "  (%s without wzp: %.3f ms)" % (op0.kernel, t0)
    line = ("%3dx%3dx%3d -> %3d %dx%d s%d %s%s%s batch %5d  %-22s %8.3f ms  dwconv_generic %9.1f ms (scaled)  x%6.1f  %7.1f GB/s  "
            "hbm_frac %.3f  same=%s%s" % (H, W, C, N, K, K, s, "SAME " if same else "VALID", " wzp" if wz else "    ", " u8" if u8 else "   ",
                                         batch, kern, t_new, t_gen, t_gen / t_new, hb / (t_new * 1e-3) / 1e9, hb / (t_new * 1e-3) / HBM,
                                         same_bytes, extra))
    print(line, flush=True)
    out.append(line)
    return kern, t_gen / t_new, same_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--gbatch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "time_dw_gemm.txt"))
    a = ap.parse_args()
    lines = ["device: " + torch.cuda.get_device_name(0)]
    print(lines[0], flush=True)
    bad = []
    for sh in SHAPES:
        gb = min(a.gbatch, 16) if sh[0] >= 112 else a.gbatch
        kern, speed, same = case(*sh, a.batch, gb, a.reps, lines)
        if not kern.startswith(("dw_gemm_rt", "conv_gemm_rt<dw")) or speed < 10.0 or not same:
            bad.append(sh)
    lines.append("shapes missing the floor (dw_gemm_rt / conv_gemm_rt<dw>, >= 10x dwconv_generic, bit-exact): %s" % (bad if bad else "none"))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
