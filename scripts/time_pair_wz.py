#!/usr/bin/env python3
"""GPU box: DepthwiseConv2D 3x3 + Conv2D 1x1 pairs with filter zero points as one pair_wz_rt launch (k_pair_wz.hip)
against the same model with fusion off (dw3x3_rt<S,wzp> + pw_rt<K,N,wzp>: what ran before the group existed), in the same process,
back to back; then whole person_detect-shaped models with zero points on every filter.

    python scripts/time_pair_wz.py [--reps 20] [--only 3]

One line per case: the median of --reps runs of each path, each timed with HIP events after warm-up, the spread of the repeats
((max - min) / median of each path), their ratio, and whether the ratio clears the larger spread -- the rule by which pair_wz_create
keeps a shape class.  Every case runs in a child process of its own under a time limit, so that one case's trouble ends that case
only; the outputs of the two paths are compared too."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

# ("pair", H, W, C, stride, N, u8, batch): per-channel zero points on both members; ("model", side, width, u8, batch)
CASES = [("pair", 48, 48, 16, 2, 32, False, 16384), ("pair", 24, 24, 32, 1, 32, False, 16384), ("pair", 24, 24, 32, 2, 64, False, 16384),
         ("pair", 12, 12, 64, 1, 64, False, 16384), ("pair", 12, 12, 64, 2, 128, False, 16384), ("pair", 6, 6, 128, 1, 128, False, 16384),
         ("pair", 6, 6, 128, 2, 256, False, 16384), ("pair", 3, 3, 256, 1, 256, False, 16384),
         ("pair", 24, 24, 32, 2, 64, True, 16384), ("pair", 6, 6, 128, 1, 128, True, 16384),
         ("model", 96, 1.0, False, 65536), ("model", 96, 1.0, True, 65536), ("model", 80, 1.0, False, 65536)]
STEP_TIMEOUT = 240  # seconds per case


def pair_model(rng, H, W, C, S, N, u8):
    """the pair with person_detect's activation quantisation (scale 6 / 255, relu6 = the whole range) and per-channel filter zero points
    off the middle on BOTH members (tools/tflite_writer.conv_net keeps the depthwise ones at the middle)"""
    import tflite_writer as tw
    lo, hi = (0, 256) if u8 else (-128, 128)
    mid = (lo + hi) // 2
    OH, OW = -(-H // S), -(-W // S)
    q = (0.0235294122, lo)
    layers = []
    for dw, n, taps, s, oshape in ((True, C, 9, S, (1, OH, OW, C)), (False, N, C, 1, (1, OH, OW, N))):
        sc = (rng.uniform(0.6, 1.4, n) * 2.2 / (74.0 * np.sqrt(taps))).astype(np.float32)
        zp = rng.integers(mid - 12, mid + 13, n)
        zp[zp == mid] = mid + 5
        d = dict(op="depthwise_conv_2d" if dw else "conv_2d", fscale=sc, fzp=zp, bias=rng.integers(-300, 300, n),
                 bscale=(sc * np.float32(q[0])).astype(np.float32), bzp=np.zeros(n, np.int64), padding="same", strides=(s, s), act="relu6",
                 out_shape=oshape, out_q=q)
        d["weights" if dw else "filters"] = rng.integers(lo, hi, (1, 3, 3, n) if dw else (n, 1, 1, C))
        layers.append(d)
    return tw.build_model((1, H, W, C), q, layers, tw.UINT8 if u8 else tw.INT8)


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


def one(idx, reps):
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    assert torch.cuda.is_available(), "needs the GPU"
    case = CASES[idx]
    if case[0] == "pair":
        _, H, W, C, S, N, u8, batch = case
        blob = pair_model(np.random.default_rng(idx), H, W, C, S, N, u8)
        what = "%3dx%3dx%3d%s -> %-3d %s" % (H, W, C, "s2" if S == 2 else "  ", N, "u8" if u8 else "i8")
    else:
        _, side, width, u8, batch = case
        blob = tw.person_detect_like(np.random.default_rng(idx), side, width, tw.UINT8 if u8 else tw.INT8, True)
        what = "person_detect_like(%d, %.1f, wzp) %s" % (side, width, "u8" if u8 else "i8")
    m = mf.Model(blob)
    m.prepare(batch)
    if u8:
        x = torch.randint(0, 256, (batch, m.input_elems), dtype=torch.uint8, device="cuda")
    else:
        x = torch.randint(-128, 128, (batch, m.input_elems), dtype=torch.int8, device="cuda")
    out = m.run_quantized(x).clone()
    ref = out.clone()
    fused_names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    groups = [n for n in fused_names if n.startswith("pair_wz_rt<")]
    t_fused, s_fused = times_ms(lambda: m.run_quantized(x, out=out), reps)
    assert torch.equal(out, ref)
    m.set_fusion(False)
    names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    t_ops, s_ops = times_ms(lambda: m.run_quantized(x, out=out), reps)
    same = bool(torch.equal(out, ref))
    m.set_fusion(True)
    ratio, spread = t_ops / t_fused, max(s_fused, s_ops)
    detail = groups[0] if case[0] == "pair" and groups else "%d pair_wz_rt groups of %d launches" % (len(groups), sum(1 for n in fused_names if not n.startswith("(")))
    off = "+".join(n for n in names if n and not n.startswith("(")) if case[0] == "pair" else "%d launches" % sum(1 for n in names if not n.startswith("("))
    print("%-40s batch %5d  %-34s %8.4f ms (spread %.3f)  fusion off %8.4f ms (spread %.3f; %s)  x%5.2f  %s  same=%s" % (
        what, batch, detail, t_fused, s_fused, t_ops, s_ops, off, ratio, "keeps" if ratio - 1.0 > spread else "NOT FASTER", same), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", type=int, default=-1, help="run this case in this process (what the parent starts per case)")
    a = ap.parse_args()
    if a.only >= 0:
        return one(a.only, a.reps)
    for idx in range(len(CASES)):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--only", str(idx)], timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            sys.exit("case %d ran into its %d s limit: nothing more is started" % (idx, STEP_TIMEOUT))
        if r.returncode != 0:
            sys.exit("case %d ended with status %d: nothing more is started" % (idx, r.returncode))


if __name__ == "__main__":
    main()
