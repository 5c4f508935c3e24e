#!/usr/bin/env python3
"""GPU box: one-channel convolutions whose image rows are not whole dwords on conv_rows_bytes (k_rt.hip) against the same build with
MF_DEV=1 MF_NO_CONV_ROWS_BYTES=1 -- conv2d_generic / dwconv_generic, what these shapes ran before -- and against the whole-dword
sibling of each shape (W rounded up to a multiple of 4, same filter) on conv_rows_lds: what the byte-granular staging costs.

    python scripts/time_conv_rows_bytes.py [--batch 16384] [--reps 20] [--repeats 3] [--only 2] [--out profiles/r12/time_conv_rows_bytes.txt]

One child process per (case, routing), each with its own time limit; after a child that fails or runs into its limit nothing more is
started.  A time is the median of --reps launches on a device-resident batch (HIP events after warm-up); the spread is
(max - min) / median of --repeats such medians.  HBM is batch x (H W + OH OW N) bytes, the least a launch must move, over the time
against 8.0 TB/s.  same: the two routings gave the same bytes.  The routing rule: a shape class keeps the new launch only where
generic / new is above 1 + the larger spread.  The last row is the whole DS-CNN keyword spotter (tools/tflite_writer.ds_cnn)."""
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
# (label, kind, H, W, N, KH, KW, stride)   all SAME, one input channel
CASES = [
    ("49x10 conv 10x4 s2 -> 64", "conv", 49, 10, 64, 10, 4, 2),
    ("49x13 dw 10x8 s2 -> 8", "dw", 49, 13, 8, 10, 8, 2),
    ("49x43 conv 3x3 -> 16", "conv", 49, 43, 16, 3, 3, 1),
    ("101x13 conv 5x5 -> 32", "conv", 101, 13, 32, 5, 5, 1),
    ("131x129 conv 3x3 s2 -> 8", "conv", 131, 129, 8, 3, 3, 2),
]
MODEL = len(CASES)                                     # the case index of the ds_cnn model


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


def prepare(mf, kind, H, W, N, KH, KW, s, seed):
    rng = np.random.default_rng(seed)
    OH, OW = -(-H // s), -(-W // s)
    c0 = rng.uniform(-30, 30, N).astype(np.float32)
    c1 = (rng.uniform(0.5, 1.5, N) * 40.0 / (5476.0 * np.sqrt(KH * KW))).astype(np.float32)
    zp = np.zeros(N, np.int8)
    if kind == "conv":
        f = rng.integers(-128, 128, (N, KH, KW, 1)).astype(np.int8)
        opts = mf.ops.Conv2DOptions(mf.FusedActivation(1), mf.TensorViewPadding(0), (s, s))
        return mf.ops.prepare_conv_2d((H, W, 1), f, zp, -125, 0.0235294122, -123, opts, (c0, c1), (OH, OW)), OH, OW
    w = rng.integers(-128, 128, (KH, KW, N)).astype(np.int8)
    opts = mf.ops.DepthwiseConv2DOptions(mf.FusedActivation(1), mf.TensorViewPadding(0), (s, s))
    return mf.ops.prepare_depthwise_conv_2d((H, W, 1), w, zp, -125, 0.0235294122, -123, opts, (c0, c1), (OH, OW)), OH, OW


def child(args):
    import torch
    import microflow_rs_amd as mf
    from microflow_rs_amd import _lib
    idx, batch = args.child, args.batch
    gen = torch.Generator("cuda").manual_seed(5)
    if idx == MODEL:
        import tflite_writer as tw
        m = mf.Model(tw.ds_cnn(np.random.default_rng(100)))
        m.prepare(batch)
        x = torch.randint(-128, 128, (batch, m.input_elems), dtype=torch.int8, device="cuda", generator=gen)
        y = torch.empty((batch, m.output_elems), dtype=torch.int8, device="cuda")
        meds = [median_ms(lambda: m.run_quantized(x, out=y), args.reps) for _ in range(args.repeats)]
        np.save(args.npy, y.cpu().numpy())
        print(json.dumps({"kernels": [m.op(i)["kernel"] for i in range(m.num_ops)], "ms": meds}))
        return
    _, kind, H, W, N, KH, KW, s = CASES[idx]
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    res = {}
    for tag, w in (("shape", W), ("sibling", (W + 3) & ~3)):
        op, OH, OW = prepare(mf, kind, H, w, N, KH, KW, s, 7 + idx)
        x = torch.randint(-128, 128, (batch, H, w, 1), dtype=torch.int8, device="cuda", generator=gen)
        y = torch.empty(batch * OH * OW * N, dtype=torch.int8, device="cuda")
        run = lambda: _lib.check(L.mf_op_run(op._h, x.data_ptr(), batch, y.data_ptr(), st))  # noqa: E731
        res[tag] = {"kernel": op.kernel, "ms": [median_ms(run, args.reps) for _ in range(args.repeats)], "bytes": batch * (H * w + OH * OW * N)}
        if tag == "shape":
            np.save(args.npy, y.cpu().numpy())
    print(json.dumps(res))


def run_child(idx, args, npy, extra_env):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MF_")}
    env.update(extra_env)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(idx), "--batch", str(args.batch), "--reps", str(args.reps),
                            "--repeats", str(args.repeats), "--npy", npy], env=env, capture_output=True, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        raise SystemExit("case %d ran into its time limit: nothing more is started" % idx)
    if r.returncode:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit("child failed with exit status %d: nothing more is started" % r.returncode)
    return json.loads(r.stdout.strip().split("\n")[-1])


def stat(ms):
    t = float(np.median(ms))
    return t, (max(ms) - min(ms)) / t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "time_conv_rows_bytes.txt"))
    ap.add_argument("--child", type=int, default=None)
    ap.add_argument("--npy", default=None)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    off = {"MF_DEV": "1", "MF_NO_CONV_ROWS_BYTES": "1"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    report = open(args.out, "w")

    def emit(line):                                    # (line by line: a child that fails leaves the rows before it)
        print(line, flush=True)
        report.write(line + "\n")
        report.flush()

    emit("batch %d, median of %d launches, spread of %d repeats; HBM on batch x (H W + OH OW N) bytes at 8.0 TB/s" % (args.batch, args.reps, args.repeats))
    with tempfile.TemporaryDirectory() as tmp:
        o = [os.path.join(tmp, "%d.npy" % i) for i in range(2)]
        for idx in range(MODEL + 1):
            if args.only is not None and idx != args.only:
                continue
            new, old = run_child(idx, args, o[0], {}), run_child(idx, args, o[1], off)
            same = bool(np.array_equal(np.load(o[0]), np.load(o[1])))
            if idx == MODEL:
                (t1, s1), (t0, s0) = stat(new["ms"]), stat(old["ms"])
                emit("ds_cnn 49x10 (whole model) | %8.3f ms  spread %4.1f %% | switch %8.3f ms  spread %4.1f %% | ratio %.2f | same=%s"
                     % (t1, 100 * s1, t0, 100 * s0, t0 / t1, same))
                emit("  default: " + " + ".join(k for k in new["kernels"] if k))
                emit("  switch : " + " + ".join(k for k in old["kernels"] if k))
                continue
            (t1, s1), (t0, s0), (ts, ss) = stat(new["shape"]["ms"]), stat(old["shape"]["ms"]), stat(new["sibling"]["ms"])
            emit("%-26s | %-24s %8.3f ms  spread %4.1f %%  HBM %.3f | %-15s %9.3f ms  spread %4.1f %%  ratio %6.1f  keeps=%s | sibling %-14s"
                 " %8.3f ms  spread %4.1f %%  HBM %.3f  new/sibling %.2f | same=%s"
                 % (CASES[idx][0], new["shape"]["kernel"], t1, 100 * s1, new["shape"]["bytes"] / (t1 * 1e-3) / HBM, old["shape"]["kernel"], t0,
                    100 * s0, t0 / t1, t0 / t1 > 1.0 + max(s0, s1), new["sibling"]["kernel"], ts, 100 * ss,
                    new["sibling"]["bytes"] / (ts * 1e-3) / HBM, t1 / ts, same))
    report.close()


if __name__ == "__main__":
    main()
