#!/usr/bin/env python3
"""GPU box: Conv2D + AveragePool2D stages as one conv_pool_rt launch (k_conv_pool.hip) against the same model with fusion off (the
convolution's own launch + avgpool_c4 / avgpool_generic: what ran before the group existed), in the same process, back to back.

    python scripts/time_conv_pool.py [--reps 20] [--repeats 3] [--sweep] [--pool max] [--yardsticks] [--only 3]

One line per case: per path the median over --repeats of the median of --reps runs (each run timed with HIP events after warm-up)
and the spread of those repeats ((max - min) / median), the ratio fusion off / default, whether the ratio clears the larger of the
two spreads, hbm_frac = batch x (H W C + POH POW N) bytes (the least the stage must move) over the default time against 8.0 TB/s
(the MI355X spec figure; a plain copy reaches 5.3 - 5.6 TB/s, profiles/r03/hbm_copy_ceiling.txt), and whether the two paths gave
the same bytes.  Under MF_DEV=1 MF_CONV_POOL_ALL=1 the classes the route excludes run as one launch too (what the exclusions are
read off); under MF_DEV=1 MF_NO_CONV_POOL=1 the first column is the routing the group replaces.  Every case runs in a child
process of its own under a time limit; the first that fails or runs into its limit ends the run, and nothing more is started.

--pool max writes the stages with a MaxPool2D (one conv_maxpool_rt launch, k_conv_maxpool.hip, against the convolution's own launch +
maxpool_c4 / maxpool_generic).  --yardsticks times, per case and in one process, what the max-pool paths are expected to match: the
stage's default path with an AveragePool2D against the same stage with a MaxPool2D (the same weights), and -- the first two lines --
avgpool_c4 against maxpool_c4 alone on 16x16x64 2x2 s2 and 48x48x8 3x3 s2 SAME at batch 65 536."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM = 8.0e12
# (label, (H, W, C), N, K, conv_pool options, batch); N = None: the whole tools/tflite_writer.lenet model
CASES = [("lenet stage 1", (28, 28, 1), 6, 5, dict(act="relu"), 65536),
         ("lenet stage 2", (12, 12, 6), 16, 5, dict(act="relu"), 65536),
         ("lenet", (28, 28, 1), None, 0, dict(), 65536),
         ("cifar stage 1", (32, 32, 3), 32, 3, dict(padding="same", act="relu"), 4096),
         ("16x16x32-64", (16, 16, 32), 64, 3, dict(padding="same", act="relu"), 4096),
         ("96x96x1-8", (96, 96, 1), 8, 3, dict(padding="same", act="relu"), 4096),
         ("64x64x4-64 (bands)", (64, 64, 4), 64, 3, dict(padding="same", act="relu"), 4096),
         ("16x16x64-64", (16, 16, 64), 64, 3, dict(padding="same", act="relu"), 4096),
         # beyond the issue's list: what the exclusion rule of fused_conv_pool_create is read off
         ("48x48x8-96 p3 (bands)", (48, 48, 8), 96, 3, dict(padding="same", act="relu", pool=(3, 3), pool_padding="same"), 4096),
         ("32x32x32-64", (32, 32, 32), 64, 3, dict(padding="same", act="relu"), 4096),
         ("12x12x1-8 5x5", (12, 12, 1), 8, 5, dict(act="relu"), 65536),
         ("24x24x8-16", (24, 24, 8), 16, 3, dict(padding="same", act="relu"), 16384)]
# --sweep: few-channel stages on 16x16 images (the convolutions conv_rows_lds takes alone) over C, N and the filter, at batch 16 384
SWEEP = [("16x16x%d-%d %dx%d" % (C, N, K, K), (16, 16, C), N, K, dict(padding="same", act="relu"), 16384)
         for K in (3, 5) for C in (3, 4, 8, 12) for N in (8, 16, 32, 64)]
STEP_TIMEOUT = 240  # seconds per case


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


POOL_OPS = [("16x16x64 p2x2s2", (16, 16, 64), (2, 2), "valid", (8, 8)), ("48x48x8 p3x3s2 same", (48, 48, 8), (3, 3), "same", (24, 24))]


def _model(tw, idx, shape, N, K, kw, pool):
    rng = np.random.default_rng(idx)
    return tw.lenet(rng, shape, pool=pool) if N is None else tw.conv_pool(rng, shape, N, K, wmax=32, pool_op=pool, **kw)


def _alternate(runs, reps, repeats):
    """-> per run (median of the repeats' medians, spread of the repeats); the runs alternate inside every repeat"""
    ts = [[] for _ in runs]
    for _ in range(repeats):
        for t, fn in zip(ts, runs):
            t.append(median_ms(fn, reps))
    return [(float(np.median(t)), (max(t) - min(t)) / float(np.median(t))) for t in ts]


def yardstick(idx, reps, repeats, cases):
    """avg against max in one process: the two pool operators alone (idx < len(POOL_OPS)), else the stage's default path"""
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    assert torch.cuda.is_available(), "needs the GPU"
    if idx < len(POOL_OPS):
        label, (H, W, C), filt, pad, out_hw = POOL_OPS[idx]
        batch = 65536
        opts = mf.ops.AveragePool2DOptions(mf.FusedActivation(0), mf.TensorViewPadding(0 if pad == "same" else 1), (2, 2))
        ops = [f((H, W, C), filt, 0.05, -3, opts, (1.0, 0.0), out_hw) for f in (mf.ops.prepare_average_pool_2d, mf.ops.prepare_max_pool_2d)]
        x = torch.randint(-128, 128, (batch, H, W, C), dtype=torch.int8, device="cuda")
        names = [o.kernel for o in ops]
        runs = [lambda o=o: o(x) for o in ops]
        hb = batch * (H * W * C + out_hw[0] * out_hw[1] * C)
    else:
        label, shape, N, K, kw, batch = cases[idx - len(POOL_OPS)]
        ms = [mf.Model(_model(tw, idx - len(POOL_OPS), shape, N, K, kw, pool)) for pool in ("avg", "max")]
        for m in ms:
            m.prepare(batch)
        x = torch.randint(-128, 128, (batch, ms[0].input_elems), dtype=torch.int8, device="cuda")
        outs = [m.run_quantized(x).clone() for m in ms]
        names = ["+".join(n for n in (m.op(i)["kernel"] for i in range(m.num_ops)) if n and not n.startswith("(")) for m in ms]
        runs = [lambda m=m, o=o: m.run_quantized(x, out=o) for m, o in zip(ms, outs)]
        hb = batch * (ms[0].input_elems + ms[0].output_elems)
    (avg, s_avg), (mx, s_mx) = _alternate(runs, reps, repeats)
    spread = max(s_avg, s_mx)
    print("%-22s batch %6d  avg %8.4f ms (spread %4.1f %%)  max %8.4f ms (spread %4.1f %%)  max / avg %5.3f  %-22s max path %.2f TB/s\n"
          "    avg: %s\n    max: %s" % (label, batch, avg, 100 * s_avg, mx, 100 * s_mx, mx / avg,
                                       "within the larger spread" if mx / avg - 1.0 <= spread else "SLOWER by more", hb / (mx * 1e-3) / 1e12, names[0], names[1]),
          flush=True)


def one(idx, reps, repeats, cases, pool="avg"):
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    assert torch.cuda.is_available(), "needs the GPU"
    label, shape, N, K, kw, batch = cases[idx]
    m = mf.Model(_model(tw, idx, shape, N, K, kw, pool))
    m.prepare(batch)
    x = torch.randint(-128, 128, (batch, m.input_elems), dtype=torch.int8, device="cuda")
    out = m.run_quantized(x).clone()
    ref = out.clone()
    on_names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    run = lambda: m.run_quantized(x, out=out)
    t_on, t_off = [], []
    same = True
    for _ in range(repeats):            # the two paths alternate, so that a drift of the clocks meets both
        t_on.append(median_ms(run, reps))
        same = same and bool(torch.equal(out, ref))
        m.set_fusion(False)
        off_names = [m.op(i)["kernel"] for i in range(m.num_ops)]
        t_off.append(median_ms(run, reps))
        same = same and bool(torch.equal(out, ref))
        m.set_fusion(True)
    on, off = float(np.median(t_on)), float(np.median(t_off))
    s_on, s_off = (max(t_on) - min(t_on)) / on, (max(t_off) - min(t_off)) / off
    ratio = off / on
    hb = batch * (m.input_elems + m.output_elems)
    launches = lambda names: "+".join(n for n in names if n and not n.startswith("("))
    print("%-20s batch %6d  default %8.4f ms (spread %4.1f %%)  fusion off %8.4f ms (spread %4.1f %%)  x%5.2f  %-12s hbm_frac %.3f (%.2f TB/s)  same=%s\n"
          "    default:    %s\n    fusion off: %s" % (
              label, batch, on, 100 * s_on, off, 100 * s_off, ratio, "clears" if ratio - 1.0 > max(s_on, s_off) else "does NOT clear",
              hb / (on * 1e-3) / HBM, hb / (on * 1e-3) / 1e12, same, launches(on_names), launches(off_names)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sweep", action="store_true", help="the few-channel sweep instead of the cases")
    ap.add_argument("--pool", choices=("avg", "max"), default="avg", help="the stages' pool operator")
    ap.add_argument("--yardsticks", action="store_true", help="avg against max in one process: the two pool operators alone, then every case's default path")
    ap.add_argument("--only", type=int, default=-1, help="run this case in this process (what the parent starts per case)")
    a = ap.parse_args()
    cases = SWEEP if a.sweep else CASES
    if a.only >= 0:
        return yardstick(a.only, a.reps, a.repeats, cases) if a.yardsticks else one(a.only, a.reps, a.repeats, cases, a.pool)
    for idx in range(len(cases) + (len(POOL_OPS) if a.yardsticks else 0)):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--repeats", str(a.repeats), "--only", str(idx), "--pool", a.pool] +
                               (["--sweep"] if a.sweep else []) + (["--yardsticks"] if a.yardsticks else []),
                               timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            sys.exit("case %d ran into its %d s limit: nothing more is started" % (idx, STEP_TIMEOUT))
        if r.returncode != 0:
            sys.exit("case %d ended with status %d: nothing more is started" % (idx, r.returncode))


if __name__ == "__main__":
    main()
