#!/usr/bin/env python3
"""GPU box: one-channel convolution -> FullyConnected (-> Softmax) models as one conv1_fc_rt launch (k_conv1_fc.hip) against the same
build with MF_DEV=1 MF_NO_CONV1_FC=1 -- the launches these models had before the kernel existed (NOT set_fusion(False), which also
splits FullyConnected + Softmax).

    python scripts/time_conv1_fc.py [--reps 20] [--repeats 3] [--only 2] [--batches 4096,65536]

One child process per (case, batch, routing), each with its own time limit.  A row: the median of --reps whole-model runs on a
device-resident batch (HIP events, back to back after warm-up), the spread (max - min) / median of --repeats such medians, the ratio
parent / one launch, the HBM fraction of the one launch on batch x (H W + N_fc) bytes at 8 TB/s, and whether the two routings gave
the same bytes.  The routing rule: a class of shapes keeps the one launch only where the ratio is above
1 + the larger spread.  profiles/r10/time_conv1_fc.txt was taken before that rule went in (fused.hip: fused_batch_ok): since then a
model whose FullyConnected has an fc_rt launch of its own runs the parent's launches above batch 4096, and its 65 536 row shows
the same launches on both sides."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM = 8.0e12
# (label, (H, W), stem, classes, u8)
CASES = [
    ("49x40 dw 10x8 s2 N8 -> 12", (49, 40), ("dw", 8, 10, 8, (2, 2), "same"), 12, False),
    ("49x40 dw 10x8 s2 N8 -> 35", (49, 40), ("dw", 8, 10, 8, (2, 2), "same"), 35, False),
    ("49x40 conv 10x8 s2 N8 -> 12", (49, 40), ("conv", 8, 10, 8, (2, 2), "same"), 12, False),
    ("49x40 conv 10x8 s2 N8 -> 35", (49, 40), ("conv", 8, 10, 8, (2, 2), "same"), 35, False),
    ("49x40 dw 10x8 s2 N16 -> 12", (49, 40), ("dw", 16, 10, 8, (2, 2), "same"), 12, False),
    ("32x40 dw 8x8 s2 N8 -> 12", (32, 40), ("dw", 8, 8, 8, (2, 2), "same"), 12, False),
    ("64x64 conv 5x5 s2 N8 -> 12", (64, 64), ("conv", 8, 5, 5, (2, 2), "same"), 12, False),
    ("49x40 conv 10x8 s2 N8 -> 12 u8", (49, 40), ("conv", 8, 10, 8, (2, 2), "same"), 12, True),
]


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


def child(args):
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    idx, batch = (int(v) for v in args.child.split(","))
    _, shape, stem, classes, u8 = CASES[idx]
    blob = tw.kws_like(np.random.default_rng(100 + idx), shape, stem, classes, elem=tw.UINT8 if u8 else tw.INT8, fc_wzp=5 if u8 else 0, wmax=32)
    m = mf.Model(blob)
    m.prepare(batch)
    lo, hi, dt = (0, 256, torch.uint8) if u8 else (-128, 128, torch.int8)
    x = torch.randint(lo, hi, (batch, m.input_elems), dtype=dt, device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    y = torch.empty((batch, m.output_elems), dtype=dt, device="cuda")
    run = lambda: m.run_quantized(x, out=y)  # noqa: E731
    meds = [median_ms(run, args.reps) for _ in range(args.repeats)]
    before = m.device_ops()
    run()
    launches = m.device_ops() - before
    np.save(args.out, y.cpu().numpy())
    print(json.dumps({"kernels": [m.op(i)["kernel"] for i in range(m.num_ops)], "ms": meds, "launches": launches}))


def run_child(idx, batch, args, out, extra_env):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MF_")}
    env.update(extra_env)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "%d,%d" % (idx, batch), "--reps", str(args.reps), "--repeats",
                            str(args.repeats), "--out", out], env=env, capture_output=True, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        raise SystemExit("case %d at batch %d ran into its time limit: nothing more is started" % (idx, batch))
    if r.returncode:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit("child failed with exit status %d: nothing more is started" % r.returncode)
    return json.loads(r.stdout.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--batches", default="4096,65536")
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    with tempfile.TemporaryDirectory() as tmp:
        for idx, (label, (H, W), _, classes, _) in enumerate(CASES):
            if args.only is not None and idx != args.only:
                continue
            for batch in (int(v) for v in args.batches.split(",")):
                o = [os.path.join(tmp, "%d.npy" % i) for i in range(2)]
                one = run_child(idx, batch, args, o[0], {})
                par = run_child(idx, batch, args, o[1], {"MF_DEV": "1", "MF_NO_CONV1_FC": "1"})
                same = bool(np.array_equal(np.load(o[0]), np.load(o[1])))
                t1, t0 = float(np.median(one["ms"])), float(np.median(par["ms"]))
                s1, s0 = (max(one["ms"]) - min(one["ms"])) / t1, (max(par["ms"]) - min(par["ms"])) / t0
                frac = batch * (H * W + classes) / (t1 * 1e-3) / HBM
                print("%-32s batch %6d | %-28s %d launch  %8.1f us  spread %4.1f %%  HBM %.3f | parent %d launches  %8.1f us  spread %4.1f %%"
                      " (%s) | ratio %.2f  keeps=%s | same=%s"
                      % (label, batch, one["kernels"][0], one["launches"], t1 * 1e3, 100 * s1, frac, par["launches"], t0 * 1e3, 100 * s0,
                         " + ".join(k for k in par["kernels"] if k and not k.startswith("(fused")), t0 / t1, t0 / t1 > 1.0 + max(s0, s1), same),
                      flush=True)


if __name__ == "__main__":
    main()
