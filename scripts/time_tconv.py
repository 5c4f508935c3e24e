#!/usr/bin/env python3
"""GPU box: TRANSPOSE_CONV (k_tconv.hip) at decoder shapes, against its generic kernel and against what a user of a tree without
the operator could run.

    python scripts/time_tconv.py --mode op                   # tconv_phase_rt at --batch (4096) images; tconv_generic on --gen-batch
                                                             # (256) images, scaled to the full batch; parity of the two in the run
    python scripts/time_tconv.py --mode ops [--root DIR]     # the yardstick: the input zero-stuffed with its zero point (built with
                                                             # torch OUTSIDE the timed region) through conv_2d with the flipped filter
                                                             # at VALID.  Runs on any commit: --root names the tree whose library is
                                                             # measured (the PARENT, which has no TRANSPOSE_CONV); two images of the
                                                             # result are checked against tests/tconv_ref.py of THIS tree
    python scripts/time_tconv.py --mode model                # tools/tflite_writer.conv_autoencoder((64, 64, 4), (16, 32, 64)) at
                                                             # batch 16 384: per-operator kernel names and times, the total

Every figure is the median of --reps (20) launches timed with HIP events after warm-up, in three repeats: the median of the three
medians and their spread ((max - min) / median).  GB/s and the HBM fraction count batch x (H W C + OH OW N) bytes; TMAC/s counts the
operator's real multiply-adds (every input pixel through every tap that lands inside the output).  Every case runs in a child process of
its own under a time limit; the first that fails or runs into its limit ends the run."""
import argparse
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#        H   W   C    N   K  s
CASES = [(8, 8, 64, 32, 3, 2), (16, 16, 32, 16, 3, 2), (16, 16, 16, 16, 4, 2), (32, 32, 64, 32, 2, 2), (8, 8, 128, 128, 3, 2), (16, 16, 64, 64, 3, 1)]
STEP_TIMEOUT = 300
REPEATS = 3
HBM_TBS = 8.0  # MI355X peak


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


def repeats(fn, reps):
    v = [median_ms(fn, reps) for _ in range(REPEATS)]
    return float(np.median(v)), float((max(v) - min(v)) / np.median(v))


def problem(idx):
    """the case's tensors and constants (fixed seed): SAME at stride s, output H s x W s"""
    H, W, C, N, K, s = CASES[idx]
    rng = np.random.default_rng(100 + idx)
    w = rng.integers(-127, 128, (N, K, K, C)).astype(np.int8)
    c0 = rng.uniform(-30, 30, N).astype(np.float32)
    c1 = (rng.uniform(0.8, 1.25, N) * 190.0 / (74.0 * 73.3 * np.sqrt(K * K * C / (s * s)))).astype(np.float32)
    return dict(H=H, W=W, C=C, N=N, K=K, s=s, OH=H * s, OW=W * s, w=w, c0=c0, c1=c1, izp=int(rng.integers(-20, 21)), ozp=int(rng.integers(-20, 21)),
                oscale=0.0235294122, padt=max(0, (H - 1) * s + K - H * s) // 2)


def real_macs(p):
    taps = sum(1 for i in range(p["H"]) for k in range(p["K"]) if 0 <= i * p["s"] + k - p["padt"] < p["OH"])
    return taps * taps * p["C"] * p["N"]  # (square images, filters and strides: the count factors into rows x columns)


def run_op(idx, a):
    import torch
    import microflow_rs_amd as mf
    p = problem(idx)
    opts = mf.ops.TransposeConvOptions(mf.FusedActivation(0), mf.TensorViewPadding(0), (p["s"], p["s"]))
    op = mf.ops.prepare_transpose_conv((p["H"], p["W"], p["C"]), p["w"], np.zeros(p["N"], np.int8), p["izp"], p["oscale"], p["ozp"], opts,
                                       (p["c0"], p["c1"]), (p["OH"], p["OW"]))
    x = torch.randint(-128, 128, (a.batch, p["H"], p["W"], p["C"]), dtype=torch.int8, device="cuda")
    name = op.kernel
    fast = op(x)
    ms, sp = repeats(lambda: op(x), a.reps)
    op.set_generic(True)
    xg = x[:a.gen_batch]
    parity = bool(torch.equal(op(xg), fast[:a.gen_batch]))
    gms, gsp = repeats(lambda: op(xg), a.reps)
    gms *= a.batch / a.gen_batch
    byts = a.batch * (p["H"] * p["W"] * p["C"] + p["OH"] * p["OW"] * p["N"])
    gbs = byts / ms / 1e6
    print("%dx%dx%d->%d %dx%d s%d | %s %.4f ms (+-%.1f%%) | %s %.3f ms scaled from %d images (+-%.1f%%) x%.1f | %.0f GB/s %.3f of HBM | %.2f TMAC/s | parity %s"
          % (p["H"], p["W"], p["C"], p["N"], p["K"], p["K"], p["s"], name, ms, 100 * sp, op.kernel, gms, a.gen_batch, 100 * gsp, gms / ms, gbs,
             gbs / (HBM_TBS * 1000), a.batch * real_macs(p) / ms / 1e9, "ok" if parity else "MISMATCH"))
    return 0 if parity else 1


def run_ops(idx, a):
    """the zero-stuffed yardstick on the tree at --root"""
    sys.path.insert(0, a.root)
    import torch
    import microflow_rs_amd as mf
    sys.path.insert(0, HERE)
    from tests import tconv_ref as T
    p = problem(idx)
    H, W, C, N, K, s, OH, OW = (p[k] for k in ("H", "W", "C", "N", "K", "s", "OH", "OW"))
    x = torch.randint(-128, 128, (a.batch, H, W, C), dtype=torch.int8, device="cuda")
    first = K - 1 - p["padt"]                     # where input row 0 lands in the stuffed image
    SH, SW = OH + K - 1, OW + K - 1
    stuffed = torch.full((a.batch, SH, SW, C), p["izp"], dtype=torch.int8, device="cuda")
    ny, nx = len(range(first, SH, s)[:H]), len(range(first, SW, s)[:W])
    stuffed[:, first:first + ny * s:s, first:first + nx * s:s, :] = x[:, :ny, :nx, :]
    wf = np.ascontiguousarray(p["w"][:, ::-1, ::-1, :])
    opts = mf.ops.Conv2DOptions(mf.FusedActivation(0), mf.TensorViewPadding(1), (1, 1))
    op = mf.ops.prepare_conv_2d((SH, SW, C), wf, np.zeros(N, np.int8), p["izp"], p["oscale"], p["ozp"], opts, (p["c0"], p["c1"]), (OH, OW))
    got = op(stuffed)
    want = T.transpose_conv(x[:2].cpu().numpy(), p["w"], p["izp"], [0], (s, s), (OH, OW), p["c0"], p["c1"], p["ozp"], p["oscale"])
    parity = np.array_equal(got[:2].cpu().numpy(), want)
    ms, sp = repeats(lambda: op(stuffed), a.reps)
    print("%dx%dx%d->%d %dx%d s%d | yardstick %s on the %dx%d zero-stuffed input %.4f ms (+-%.1f%%) | parity with the contract %s"
          % (H, W, C, N, K, K, s, op.kernel, SH, SW, ms, 100 * sp, "ok" if parity else "MISMATCH"))
    return 0 if parity else 1


def run_model(a):
    import torch
    sys.path.insert(0, os.path.join(HERE, "tools"))
    import tflite_writer as tw
    import microflow_rs_amd as mf
    m = mf.model(tw.conv_autoencoder(np.random.default_rng(7), (64, 64, 4), (16, 32, 64)))
    B = a.model_batch
    m.prepare(B)
    x = torch.randint(-128, 128, (B, 64, 64, 4), dtype=torch.int8, device="cuda")
    y = torch.empty((B, m.output_elems), dtype=torch.int8, device="cuda")
    v = [m.time_device(x, y, B, 3, a.reps, True) for _ in range(REPEATS)]
    tot = [t for t, _ in v]
    print("conv_autoencoder((64, 64, 4), (16, 32, 64)) batch %d: %.3f ms (+-%.1f%%), %.2f M inferences/s" % (B, np.median(tot), 100 * (max(tot) - min(tot)) / np.median(tot), B / np.median(tot) / 1e3))
    for i in range(m.num_ops):
        o = m.op(i)
        print("  %d %-16s %-28s -> %-18s %.3f ms" % (i, o["name"], o["kernel"], "x".join(map(str, o["out_shape"][1:])), float(np.median([per[i] for _, per in v]))))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("op", "ops", "model"), default="op")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--gen-batch", type=int, default=256)
    ap.add_argument("--model-batch", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", type=int, default=-1, help="run this case in this process (what the parent starts per case)")
    a = ap.parse_args()
    a.root = os.path.abspath(a.root)
    if a.only >= 0 or a.mode == "model":
        if a.mode != "ops":
            sys.path.insert(0, HERE)
        return (run_model(a) if a.mode == "model" else run_op(a.only, a) if a.mode == "op" else run_ops(a.only, a))
    for idx in range(len(CASES)):
        cmd = [sys.executable, os.path.abspath(__file__), "--mode", a.mode, "--root", a.root, "--batch", str(a.batch), "--gen-batch", str(a.gen_batch),
               "--reps", str(a.reps), "--only", str(idx)]
        try:
            r = subprocess.run(cmd, timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            sys.exit("case %d ran into its %d s limit: nothing more is started" % (idx, STEP_TIMEOUT))
        if r.returncode != 0:
            sys.exit("case %d ended with status %d: nothing more is started" % (idx, r.returncode))
    return 0


if __name__ == "__main__":
    sys.exit(main())
