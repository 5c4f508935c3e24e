#!/usr/bin/env python3
"""GPU box: Conv2D + AveragePool2D stages as one conv_pool_rt launch (k_conv_pool.hip) against the same model with fusion off (the
convolution's own launch + avgpool_c4 / avgpool_generic: what ran before the group existed), in the same process, back to back.

    python scripts/time_conv_pool.py [--reps 20] [--repeats 3] [--sweep] [--only 3]

One line per case: per path the median over --repeats of the median of --reps runs (each run timed with HIP events after warm-up)
and the spread of those repeats ((max - min) / median), the ratio fusion off / default, whether the ratio clears the larger of the
two spreads, hbm_frac = batch x (H W C + POH POW N) bytes (the least the stage must move) over the default time against 8.0 TB/s
(the MI355X spec figure; a plain copy reaches 5.3 - 5.6 TB/s, profiles/r03/hbm_copy_ceiling.txt), and whether the two paths gave
the same bytes.  Under MF_DEV=1 MF_CONV_POOL_ALL=1 the classes the route excludes run as one launch too (what the exclusions are
read off); under MF_DEV=1 MF_NO_CONV_POOL=1 the first column is the routing the group replaces.  Every case runs in a child
process of its own under a time limit; the first that fails or runs into its limit ends the run, and nothing more is started."""
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


def one(idx, reps, repeats, cases):
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    assert torch.cuda.is_available(), "needs the GPU"
    label, shape, N, K, kw, batch = cases[idx]
    rng = np.random.default_rng(idx)
    m = mf.Model(tw.lenet(rng, shape) if N is None else tw.conv_pool(rng, shape, N, K, wmax=32, **kw))
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
    ap.add_argument("--only", type=int, default=-1, help="run this case in this process (what the parent starts per case)")
    a = ap.parse_args()
    cases = SWEEP if a.sweep else CASES
    if a.only >= 0:
        return one(a.only, a.reps, a.repeats, cases)
    for idx in range(len(cases)):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--repeats", str(a.repeats), "--only", str(idx)] + (["--sweep"] if a.sweep else []),
                               timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            sys.exit("case %d ran into its %d s limit: nothing more is started" % (idx, STEP_TIMEOUT))
        if r.returncode != 0:
            sys.exit("case %d ended with status %d: nothing more is started" % (idx, r.returncode))


if __name__ == "__main__":
    main()
