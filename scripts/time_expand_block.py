#!/usr/bin/env python3
"""GPU box: Conv2D 1x1 expand + DepthwiseConv2D 3x3 + Conv2D 1x1 project blocks as one block_band_rt launch (k_block_band.hip) against
the same model with fusion off (one launch per operator), in the same process, back to back.

    python scripts/time_expand_block.py [--reps 20] [--only 3] [--sweep]

--sweep times a second set instead: the blocks that did not clear the routing rule at the batches above, each at batches 16 .. 4096 (one
model, one line per batch).  Below some batch three launches cost more than the work inside them; fused_block_create's batch limits
 are read off this table.

Under MF_DEV=1 MF_NO_EXPAND_BLOCK=1 the first column is the routing without the block group (the expand's own launch, then the pair's
group where it has one): the other half of the routing rule of DESIGN 4.16.

One line per shape: the median of --reps runs of each path, each timed with HIP events after warm-up, the spread of the repeats
((max - min) / median of each path), their ratio, and hbm_frac = batch x (H W C + OH OW N) bytes (the least a launch must move) over
the first path's time against 8.0 TB/s (the MI355X spec figure; a plain copy reaches 5.3 - 5.6 TB/s, profiles/r03/hbm_copy_ceiling.txt).
Every shape runs in a child process of its own under a time limit, so that one shape's trouble ends that shape only; the outputs
of the two paths are compared too.  The last line is a model of four blocks (tests/test_gpu_expand_block.py's) with its head."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM = 8.0e12
# (H, W, C, E, stride, N, batch): MobileNet-v2's blocks at 224 and at 96 input as far as E <= 256 goes
SHAPES = [(112, 112, 16, 96, 2, 24, 512), (56, 56, 24, 144, 1, 24, 1024), (56, 56, 24, 144, 2, 32, 1024), (28, 28, 32, 192, 1, 32, 4096),
          (28, 28, 32, 192, 2, 64, 4096), (48, 48, 16, 96, 2, 24, 2048), (24, 24, 24, 144, 1, 24, 4096), (12, 12, 32, 192, 1, 32, 8192),
          (6, 6, 32, 192, 2, 64, 16384)]
WHOLE = [op for (E, S, N) in ((96, 1, 24), (144, 2, 32), (192, 1, 32), (192, 2, 64)) for op in (("conv", E, 1, 1), ("dw", 0, 3, S), ("conv", N, 1, 1))]
WHOLE_BATCH = 4096
# --sweep: (H, W, C, E, stride, N) of the classes at parity or slower at large batches: one k step of E, four k steps at stride 2 with
# N <= 32, four k steps at stride 1; then the four-block model (index len(SWEEP_SHAPES))
SWEEP_SHAPES = [(6, 6, 8, 32, 1, 8), (9, 7, 16, 64, 1, 24), (13, 11, 12, 48, 1, 20), (12, 12, 16, 64, 1, 16), (10, 10, 24, 144, 2, 32),
                (28, 28, 24, 144, 2, 32), (56, 56, 24, 144, 2, 32), (14, 14, 32, 192, 1, 32), (28, 28, 32, 192, 1, 32), (24, 24, 24, 144, 1, 24)]
SWEEP_BATCHES = (16, 64, 128, 256, 512, 1024, 4096)
STEP_TIMEOUT = 240  # seconds per shape


def times_ms(fn, reps, warm=3, inner=1):
    """median and spread of `reps` samples; a sample is `inner` calls back to back between one pair of events, divided by inner (a
    single launch of 15 us between two events measures the events: the sweep's small batches take ten per sample)"""
    import torch
    one = fn
    if inner > 1:
        def fn():
            for _ in range(inner):
                one()
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
        ts.append(a.elapsed_time(b) / inner)
    return float(np.median(ts)), float((max(ts) - min(ts)) / np.median(ts))


def one(idx, reps):
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    assert torch.cuda.is_available(), "needs the GPU"
    if idx < len(SHAPES):
        H, W, C, E, S, N, batch = SHAPES[idx]
        blob = tw.conv_net(np.random.default_rng(idx), (H, W, C), [("conv", E, 1, 1), ("dw", 0, 3, S), ("conv", N, 1, 1)], act_scale=6.0 / 255.0)
        OH, OW = -(-H // S), -(-W // S)
        hb = batch * (H * W * C + OH * OW * N)
        label = "%3dx%3dx%3d -> %3d%s -> %-3d" % (H, W, C, E, "s2" if S == 2 else "  ", N)
    else:
        batch = WHOLE_BATCH
        blob = tw.conv_net(np.random.default_rng(idx), (28, 28, 16), WHOLE, head=10, act_scale=6.0 / 255.0)
        hb = batch * (28 * 28 * 16 + 10)
        label = "four blocks from 28x28x16 + head"
    m = mf.Model(blob)
    m.prepare(batch)
    x = torch.randint(-128, 128, (batch, m.input_elems), dtype=torch.int8, device="cuda")
    out = m.run_quantized(x).clone()
    ref = out.clone()
    first = [m.op(i)["kernel"] for i in range(m.num_ops)]
    t_first, s_first = times_ms(lambda: m.run_quantized(x, out=out), reps)
    assert torch.equal(out, ref)
    m.set_fusion(False)
    names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    t_ops, s_ops = times_ms(lambda: m.run_quantized(x, out=out), reps)
    same = bool(torch.equal(out, ref))
    m.set_fusion(True)
    print("%s batch %5d  %-60s %8.4f ms (spread %.3f)  fusion off %8.4f ms (spread %.3f; %s)  x%5.2f  hbm_frac %.3f (%.2f TB/s)  same=%s" % (
        label, batch, "+".join(n for n in first if n and not n.startswith("(")), t_first, s_first, t_ops, s_ops, "+".join(n for n in names if n and not n.startswith("(")),
        t_ops / t_first, hb / (t_first * 1e-3) / HBM, hb / (t_first * 1e-3) / 1e12, same), flush=True)


def sweep(idx, reps):
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    assert torch.cuda.is_available(), "needs the GPU"
    if idx < len(SWEEP_SHAPES):
        H, W, C, E, S, N = SWEEP_SHAPES[idx]
        blob = tw.conv_net(np.random.default_rng(idx), (H, W, C), [("conv", E, 1, 1), ("dw", 0, 3, S), ("conv", N, 1, 1)], act_scale=6.0 / 255.0)
        label = "%3dx%3dx%3d -> %3d%s -> %-3d" % (H, W, C, E, "s2" if S == 2 else "  ", N)
    else:
        blob = tw.conv_net(np.random.default_rng(idx), (28, 28, 16), WHOLE, head=10, act_scale=6.0 / 255.0)
        label = "four blocks from 28x28x16 + head"
    m = mf.Model(blob)
    m.prepare(max(SWEEP_BATCHES))
    for batch in SWEEP_BATCHES:
        x = torch.randint(-128, 128, (batch, m.input_elems), dtype=torch.int8, device="cuda")
        out = m.run_quantized(x).clone()
        ref = out.clone()
        first = [m.op(i)["kernel"] for i in range(m.num_ops)]
        t_first, s_first = times_ms(lambda: m.run_quantized(x, out=out), reps, inner=10)
        m.set_fusion(False)
        t_ops, s_ops = times_ms(lambda: m.run_quantized(x, out=out), reps, inner=10)
        same = bool(torch.equal(out, ref))
        m.set_fusion(True)
        print("%s batch %5d  %-44s %8.4f ms (spread %.3f)  fusion off %8.4f ms (spread %.3f)  x%5.2f  same=%s" % (
            label, batch, "+".join(n.split(";")[0] for n in first if n and not n.startswith("("))[:44], t_first, s_first, t_ops, s_ops, t_ops / t_first, same), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", type=int, default=-1, help="run this shape in this process (what the parent starts per shape)")
    ap.add_argument("--sweep", action="store_true", help="the blocks at parity or slower at large batches, at batches 16 .. 4096")
    a = ap.parse_args()
    if a.only >= 0:
        return sweep(a.only, a.reps) if a.sweep else one(a.only, a.reps)
    for idx in range(len(SWEEP_SHAPES if a.sweep else SHAPES) + 1):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--only", str(idx)] + (["--sweep"] if a.sweep else []),
                               timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            sys.exit("shape %d ran into its %d s limit: nothing more is started" % (idx, STEP_TIMEOUT))
        if r.returncode != 0:
            sys.exit("shape %d ended with status %d: nothing more is started" % (idx, r.returncode))


if __name__ == "__main__":
    main()
