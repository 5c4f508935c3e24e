#!/usr/bin/env python3
"""GPU box: deep Conv2D shapes on conv_stream_rt (k_conv_stream.hip) against the kernel the same build runs for them with the
selection off (MF_DEV=1 MF_NO_CONV_STREAM=1: conv_gemm_rt, or conv2d_generic for K' > 8192), one table line per shape and row count.

    python scripts/time_conv_stream.py [--batch 4096] [--reps 20] [--sweep] [--only I,J,..]

Every (shape, side) is one child process with its own time limit (the switches are read once per process): the stream side runs
under MF_CONV_STREAM_MIN_ROWS=64, so that every row count of a sweep selects the new kernel.  A time is the median of --reps launches
timed with HIP events after warm-up; each is taken three times and printed as the median of the three with their spread (max - min).
`wins` holds where the new kernel beats the old one by more than the larger of the two spreads -- the rule stream_min_rows and the class
exclusions of k::conv_stream_plan are read from.  same: the stream side's first images equal conv2d_generic's bytes, in
the timed process.  For a 1x1 stride-1 shape the stream child also times fc_mfma on the same M x K x N: the ceiling of this kernel.
--sweep adds the row counts 256 .. 65 536 on nine of the shapes.  A shape may carry its own batch (the large images: the same rows as
the others at batch 4096).  The first child that fails or runs out of time ends the run: nothing more is started on the GPU."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# H, W, C, N, K, stride (SAME) [, batch]
SHAPES = [(8, 8, 256, 256, 3, 1), (8, 8, 256, 512, 3, 2), (4, 4, 512, 512, 3, 1), (2, 2, 512, 512, 3, 1), (8, 8, 128, 128, 3, 1),
          (14, 14, 512, 512, 1, 1), (7, 7, 512, 1024, 1, 1), (7, 7, 1024, 1024, 1, 1), (8, 8, 256, 512, 1, 2), (2, 2, 1024, 1024, 3, 1),
          # beyond the issue's list: two filters of at most 96 KiB (on pw_rt / conv_mm_rt today), C = 128 with more outputs, larger images
          (7, 7, 256, 128, 1, 1), (8, 8, 128, 128, 1, 2), (8, 8, 128, 256, 3, 1), (14, 14, 256, 256, 3, 1, 1024), (28, 28, 256, 256, 3, 1, 256),
          (56, 56, 256, 256, 3, 1, 64)]
SWEPT = (2, 4, 6, 10, 11, 12, 13, 14, 15)
SWEEP_ROWS = [256 << i for i in range(9)]


def child(H, W, C, N, K, s, side, batches, reps):
    sys.path.insert(0, ROOT)
    import torch
    import microflow_rs_amd as mf
    from microflow_rs_amd import _lib

    def med3(fn):
        out = []
        for _ in range(3):
            for _ in range(3):
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
            out.append(float(np.median(ts)))
        return out

    rng = np.random.default_rng(H * 31 + C * 7 + N + K)
    OH, OW = -(-H // s), -(-W // s)
    f = rng.integers(-128, 128, (N, K, K, C)).astype(np.int8)
    c0 = rng.uniform(-30, 30, N).astype(np.float32)
    c1 = (rng.uniform(0.5, 1.5, N) * 40.0 / (5476.0 * np.sqrt(K * K * C))).astype(np.float32)
    opts = mf.ops.Conv2DOptions(mf.FusedActivation(1), mf.TensorViewPadding.SAME, (s, s))
    op = mf.ops.prepare_conv_2d((H, W, C), f, np.zeros(N, np.int8), -3, 0.0235294122, 5, opts, (c0, c1), (OH, OW))
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    for batch in batches:
        x = torch.randint(-128, 128, (batch, H, W, C), dtype=torch.int8, device="cuda")
        y = torch.empty(batch * OH * OW * N, dtype=torch.int8, device="cuda")
        rec = {"batch": batch, "rows": batch * OH * OW, "label": op.kernel, "kernel": op.kernel_at(batch)}
        rec["ms"] = med3(lambda: _lib.check(L.mf_op_run(op._h, x.data_ptr(), batch, y.data_ptr(), st)))
        if side == "stream":
            gb = min(batch, max(1, 2048 // (OH * OW)))
            yg = torch.empty(gb * OH * OW * N, dtype=torch.int8, device="cuda")
            op.set_generic(True)
            _lib.check(L.mf_op_run(op._h, x.data_ptr(), gb, yg.data_ptr(), st))
            op.set_generic(False)
            rec["same"] = bool(torch.equal(y[:yg.numel()], yg))
            if K == 1 and s == 1:   # the ceiling: fc_mfma on the same M x K x N
                fc = mf.ops.prepare_fully_connected(batch * H * W, f.reshape(N, C), 0, 0.0235294122, 5, mf.ops.FullyConnectedOptions(mf.FusedActivation(1)),
                                                    (c0, float(c1[0]), np.zeros(N, np.int32), 0))
                rec["fc_kernel"] = fc.kernel
                rec["fc_ms"] = med3(lambda: _lib.check(L.mf_op_run(fc._h, x.data_ptr(), 1, y.data_ptr(), st)))
        print("REC " + json.dumps(rec), flush=True)


def run_side(shape, side, batches, reps, limit):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MF_")}
    env["MF_DEV"] = "1"
    env.update({"MF_CONV_STREAM_MIN_ROWS": "64"} if side == "stream" else {"MF_NO_CONV_STREAM": "1"})
    cmd = [sys.executable, os.path.abspath(__file__), "--child", ",".join(map(str, shape)), side, ",".join(map(str, batches)), "--reps", str(reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired:
        print("%s side of %s: no result within %d s: stopping" % (side, shape, limit), flush=True)
        return None
    if r.returncode != 0:
        print("%s side of %s failed (exit %d): stopping\n%s" % (side, shape, r.returncode, r.stderr[-1500:]), flush=True)
        return None
    return {rec["batch"]: rec for rec in (json.loads(l[4:]) for l in r.stdout.splitlines() if l.startswith("REC "))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--child", nargs=3)
    a = ap.parse_args()
    if a.child:
        return child(*[int(v) for v in a.child[0].split(",")], a.child[1], [int(v) for v in a.child[2].split(",")], a.reps)
    only = [int(v) for v in a.only.split(",")] if a.only else range(len(SHAPES))
    med = lambda v: float(np.median(v))  # noqa: E731
    for i in only:
        H, W, C, N, K, s = SHAPES[i][:6]
        OHW = -(-H // s) * -(-W // s)
        batches = sorted({(SHAPES[i] + (a.batch,))[6]} | ({-(-r // OHW) for r in SWEEP_ROWS} if a.sweep and i in SWEPT else set()))
        new = run_side(SHAPES[i][:6], "stream", batches, a.reps, a.limit)
        old = run_side(SHAPES[i][:6], "base", batches, a.reps, a.limit) if new is not None else None
        if new is None or old is None:   # a child failed, faulted or hung: nothing more is started on the GPU
            return 1
        for b in batches:
            n, o = new.get(b), old.get(b)
            if not n or not o:
                continue
            tn, to, sn, so = med(n["ms"]), med(o["ms"]), max(n["ms"]) - min(n["ms"]), max(o["ms"]) - min(o["ms"])
            mac = n["rows"] * N * K * K * C
            line = "%2dx%2dx%4d -> %4d %dx%d s%d rows %6d  %-19s %8.3f ms (+-%.3f) %7.1f TMAC/s | %-14s %9.3f ms (+-%.3f) | x%6.2f wins=%s same=%s" % (
                H, W, C, N, K, K, s, n["rows"], n["kernel"], tn, sn, mac / (tn * 1e-3) / 1e12, o["kernel"], to, so, to / tn,
                to - tn > max(sn, so), n.get("same"))
            if "fc_ms" in n:
                line += " | %s %.3f ms: %.2f of it" % (n["fc_kernel"], med(n["fc_ms"]), med(n["fc_ms"]) / tn)
            print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
