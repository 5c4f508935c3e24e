#!/usr/bin/env python3
"""GPU box: deep Conv2D shapes with 2:4-pruned filters on conv_stream_sp24 (k_conv_stream_sparse.hip) against conv_stream_rt on the SAME
pruned filter, one table line per shape and row count.

    python scripts/time_conv_sparse.py --root <tree of the parent commit, built> [--batch 4096] [--reps 20] [--sweep] [--only I,J,..]

The yardstick is the parent build (--root), which runs conv_stream_rt; the same build under MF_DEV=1 MF_NO_CONV_SPARSE=1 is the
cross-check (`off`) and should agree with the parent within the spread.  The sparse side runs under MF_CONV_SPARSE_ALL=1, and every side
under MF_CONV_STREAM_MIN_ROWS=64, so that every row count of a sweep selects the stream kernels whatever the thresholds say.  Every
(shape, side) is one child process with its own time limit (the switches are read once per process).  A time is the median of --reps
launches timed with HIP events after warm-up; each is taken three times and printed as the median of the three with their spread
(max - min).  `wins` holds where the sparse kernel beats the parent by more than the larger of the two spreads -- the rule
k::conv_stream_sp24_min_rows is read from.  same: the first images equal conv2d_generic's bytes, in the timed process.
The filters keep the two largest magnitudes of every group of four along (ky, kx, c) (make_fc_model.prune_2_4).  --sweep adds the row
counts 256 .. 65 536 on the swept shapes.  The first child that fails or runs out of time ends the run: nothing more is started on the GPU."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# H, W, C, N, K, stride (SAME): the 3x3 and 1x1 rows of DESIGN 4.28's table
SHAPES = [(8, 8, 256, 256, 3, 1), (8, 8, 256, 512, 3, 2), (4, 4, 512, 512, 3, 1), (2, 2, 512, 512, 3, 1), (8, 8, 128, 128, 3, 1),
          (2, 2, 1024, 1024, 3, 1), (14, 14, 512, 512, 1, 1), (7, 7, 512, 1024, 1, 1), (7, 7, 1024, 1024, 1, 1), (8, 8, 256, 512, 1, 2)]
SWEPT = (0, 2, 4, 7, 8)
SWEEP_ROWS = [256 << i for i in range(9)]
SIDES = {"sparse": {"MF_CONV_SPARSE_ALL": "1"}, "parent": {}, "off": {"MF_NO_CONV_SPARSE": "1"}}


def child(root, H, W, C, N, K, s, batches, reps):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch
    import microflow_rs_amd as mf
    from microflow_rs_amd import _lib
    from make_fc_model import prune_2_4

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
    f = prune_2_4(rng.integers(-128, 128, (N, K, K, C)).astype(np.int8))
    c0 = rng.uniform(-30, 30, N).astype(np.float32)
    c1 = (rng.uniform(0.5, 1.5, N) * 40.0 / (5476.0 * np.sqrt(K * K * C / 2))).astype(np.float32)
    opts = mf.ops.Conv2DOptions(mf.FusedActivation(1), mf.TensorViewPadding.SAME, (s, s))
    op = mf.ops.prepare_conv_2d((H, W, C), f, np.zeros(N, np.int8), -3, 0.0235294122, 5, opts, (c0, c1), (OH, OW))
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    for batch in batches:
        x = torch.randint(-128, 128, (batch, H, W, C), dtype=torch.int8, device="cuda")
        y = torch.empty(batch * OH * OW * N, dtype=torch.int8, device="cuda")
        rec = {"batch": batch, "rows": batch * OH * OW, "kernel": op.kernel_at(batch)}
        rec["ms"] = med3(lambda: _lib.check(L.mf_op_run(op._h, x.data_ptr(), batch, y.data_ptr(), st)))
        gb = min(batch, max(1, 2048 // (OH * OW)))
        yg = torch.empty(gb * OH * OW * N, dtype=torch.int8, device="cuda")
        op.set_generic(True)
        _lib.check(L.mf_op_run(op._h, x.data_ptr(), gb, yg.data_ptr(), st))
        op.set_generic(False)
        rec["same"] = bool(torch.equal(y[:yg.numel()], yg))
        print("REC " + json.dumps(rec), flush=True)


def run_side(root, shape, side, batches, reps, limit):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MF_")}
    env.update({"MF_DEV": "1", "MF_CONV_STREAM_MIN_ROWS": "64"}, **SIDES[side])
    cmd = [sys.executable, os.path.abspath(__file__), "--child", root, ",".join(map(str, shape)), ",".join(map(str, batches)), "--reps", str(reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, env=env, cwd=root)
    except subprocess.TimeoutExpired:
        print("%s side of %s: no result within %d s: stopping" % (side, shape, limit), flush=True)
        return None
    if r.returncode != 0:
        print("%s side of %s failed (exit %d): stopping\n%s" % (side, shape, r.returncode, r.stderr[-1500:]), flush=True)
        return None
    return {rec["batch"]: rec for rec in (json.loads(l[4:]) for l in r.stdout.splitlines() if l.startswith("REC "))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", help="the built tree of the parent commit: the yardstick")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--child", nargs=3)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], *[int(v) for v in a.child[1].split(",")], [int(v) for v in a.child[2].split(",")], a.reps)
    if not a.root:
        ap.error("--root: the sparse kernel is compared with the parent commit's build, not with itself")
    only = [int(v) for v in a.only.split(",")] if a.only else range(len(SHAPES))
    med = lambda v: float(np.median(v))  # noqa: E731
    spr = lambda v: max(v) - min(v)  # noqa: E731
    for i in only:
        H, W, C, N, K, s = SHAPES[i]
        OHW = -(-H // s) * -(-W // s)
        batches = sorted({a.batch} | ({-(-r // OHW) for r in SWEEP_ROWS} if a.sweep and i in SWEPT else set()))
        res = {}
        for side, root in (("sparse", ROOT), ("parent", os.path.abspath(a.root)), ("off", ROOT)):
            res[side] = run_side(root, SHAPES[i], side, batches, a.reps, a.limit)
            if res[side] is None:   # a child failed, faulted or hung: nothing more is started on the GPU
                return 1
        for b in batches:
            n, o, x = res["sparse"].get(b), res["parent"].get(b), res["off"].get(b)
            if not n or not o or not x:
                continue
            tn, to, tx = med(n["ms"]), med(o["ms"]), med(x["ms"])
            mac = n["rows"] * N * K * K * C
            print("%2dx%2dx%4d -> %4d %dx%d s%d rows %6d  %-21s %8.4f ms (+-%.4f) %7.1f TMAC/s | parent %-19s %8.4f ms (+-%.4f) | off %8.4f ms (+-%.4f) | x%5.2f wins=%s same=%s" % (
                H, W, C, N, K, K, s, n["rows"], n["kernel"], tn, spr(n["ms"]), mac / (tn * 1e-3) / 1e12, o["kernel"], to, spr(o["ms"]), tx, spr(x["ms"]),
                to / tn, to - tn > max(spr(n["ms"]), spr(o["ms"])), n["same"] and o["same"] and x["same"]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
