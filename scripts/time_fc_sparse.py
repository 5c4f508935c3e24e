#!/usr/bin/env python3
"""GPU box: FullyConnected with 2:4-sparse weights -- fc_sparse24 (k_fc_sparse.hip) against fc_mfma on the same pruned weights (a
child process with MF_DEV=1 MF_NO_FC_SPARSE=1) and against fc_mfma on the unpruned weights.

    python scripts/time_fc_sparse.py [--reps 20]

One row per shape and weight zero point: the median of --reps launches of the operator, each timed with HIP events, back to back
after warm-up; POP/s counts the dense-equivalent 2 M K N operations, frac is that rate over 5.0 POP/s (the dense int8 MFMA peak);
same = the output bytes of fc_sparse24 and of fc_mfma on the pruned weights are identical."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MFMA_I8 = 5.0e15
SHAPES = [(4096, 4096, 4096), (8192, 4096, 4096), (65536, 1024, 1024), (4096, 512, 4096)]


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


def measure(M, K, N, wzp, pruned, reps, out_path):
    """one operator: (kernel label, median ms); its output to out_path"""
    import torch
    import microflow_rs_amd as mf
    from microflow_rs_amd import _lib
    from make_fc_model import prune_2_4
    rng = np.random.default_rng(M + K + N)
    w = rng.integers(-128, 128, (N, K), dtype=np.int8)
    if pruned:
        w = prune_2_4(w)
    c0 = rng.uniform(-3, 3, N).astype(np.float32)
    c1 = np.float32(1.0 / (40.0 * 74.0 * 74.0 * np.sqrt(K)))
    c2 = rng.integers(-4096, 4096, N).astype(np.int32)
    op = mf.ops.prepare_fully_connected(1, w, wzp, 0.05, 3, mf.ops.FullyConnectedOptions(), (c0, c1, c2, int(127.5 * K * wzp)))
    x = torch.randint(-128, 128, (M, K), dtype=torch.int8, device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    y = torch.empty(M * N, dtype=torch.int8, device="cuda")
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    run = lambda: _lib.check(L.mf_op_run(op._h, x.data_ptr(), M, y.data_ptr(), st))  # noqa: E731
    t = median_ms(run, reps)
    np.save(out_path, y.cpu().numpy())
    return op.kernel, t


def child(args):
    M, K, N, wzp, pruned = (int(v) for v in args.child.split(","))
    kern, t = measure(M, K, N, wzp, pruned, args.reps, args.out)
    print(json.dumps({"kernel": kern, "ms": t}))


def run_child(M, K, N, wzp, pruned, reps, out, extra_env):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MF_")}
    env.update(extra_env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "%d,%d,%d,%d,%d" % (M, K, N, wzp, pruned), "--reps", str(reps),
                        "--out", out], env=env, capture_output=True, text=True, timeout=900)
    if r.returncode:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit("child failed with exit status %d" % r.returncode)
    return json.loads(r.stdout.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--child", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        for M, K, N in SHAPES:
            for wzp in (0, -3):
                o = [os.path.join(tmp, "%d.npy" % i) for i in range(3)]
                sp = run_child(M, K, N, wzp, 1, args.reps, o[0], {})
                dn = run_child(M, K, N, wzp, 1, args.reps, o[1], {"MF_DEV": "1", "MF_NO_FC_SPARSE": "1"})
                un = run_child(M, K, N, wzp, 0, args.reps, o[2], {})
                same = bool(np.array_equal(np.load(o[0]), np.load(o[1])))
                pops = 2.0 * M * K * N / (sp["ms"] * 1e-3)
                print("fc %6d x %4d x %4d wzp %2d  %-16s %8.1f us  %5.2f POP/s  frac %.3f | %s pruned %8.1f us  x%.2f | %s dense %8.1f us  "
                      "x%.2f | same=%s" % (M, K, N, wzp, sp["kernel"], sp["ms"] * 1e3, pops / 1e15, pops / MFMA_I8, dn["kernel"],
                                           dn["ms"] * 1e3, dn["ms"] / sp["ms"], un["kernel"], un["ms"] * 1e3, un["ms"] / sp["ms"], same),
                      flush=True)


if __name__ == "__main__":
    main()
