#!/usr/bin/env python3
"""GPU box: CONCATENATION alone, and a fire module's 1x1 expand + its CONCATENATION as ONE launch (k_side_join.hip: side_concat_rt)
against what it replaces, at the fire modules of SqueezeNet 1.1 with the stages at the resolutions a 224 x 224 input gives them.

    python scripts/time_concat.py --mode op                      # concat_c4 at the four fire outputs against torch.cat(dim=-1) on int8
                                                                 # tensors and against a device copy of the same bytes, one process
    python scripts/time_concat.py --mode ops   [--root DIR]      # the yardstick of the fused launch: the 1x1 Conv2D through the
                                                                 # operator API (mf_conv_2d_create, mf_op_run) + torch.cat of the two
                                                                 # tensors, medians summed.  Runs on any commit: --root names the tree
                                                                 # whose library is measured (the PARENT, which has no CONCATENATION)
    python scripts/time_concat.py --mode model                   # a model [side Conv2D 1x1, main Conv2D 3x3, CONCATENATION]: the join's
                                                                 # slot of mf_model_time_device(per_op): the fused launch, or -- under
                                                                 # MF_DEV=1 MF_NO_SIDE_CONCAT=1 -- the two launches in the same slot
    python scripts/time_concat.py --mode squeezenet              # the whole tools/tflite_writer.squeezenet(side=64): per-operator
                                                                 # kernel names and times, the total, parity against fusion off

Every figure is the median of --reps (20) runs timed with HIP events after warm-up, in three repeats: the median of the three medians
and their spread ((max - min) / median).  --batch (65 536) is cut per case to the largest multiple of 1024 that keeps the case's
largest tensor within --cap-gib (4): a 55 x 55 x 128 output is 25 GB at the full batch, and a streaming launch runs at the same rate
on 4 GiB.  The batch used is printed with every line.

Every case runs in a child process of its own under a time limit; the first that fails or runs into its limit ends the run."""
import argparse
import os
import subprocess
import sys

import numpy as np

# (H = W, S, E1, E3): SqueezeNet 1.1's three stages at a 224 input, and the widest fire
CASES = [(55, 16, 64, 64), (27, 32, 128, 128), (13, 48, 192, 192), (13, 64, 256, 256)]
STEP_TIMEOUT = 300
REPEATS = 3
HBM_TBS = 8.0  # MI355X peak, for the fraction printed by --mode op


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


def spread(v):
    return float((max(v) - min(v)) / np.median(v))


def batch_of(idx, a):
    H, S, E1, E3 = CASES[idx]
    per = H * H * (E1 + E3)
    cut = int(a.cap_gib * (1 << 30)) // per // 1024 * 1024
    return max(1024, min(a.batch, cut))


def layers_of(idx):
    """(in_q, side 1x1 conv layer, main 3x3 conv layer, join layer) of case idx, from the writer's per-layer helpers, which are the
    same on every commit; both expands carry one output quantisation and the join copies, as in converter-written files"""
    import tflite_writer as tw
    H, S, E1, E3 = CASES[idx]
    rng = np.random.default_rng(600 + idx)
    in_q = (0.05, -128)
    side = tw._conv_layer(rng, (H, H, S), in_q, False, E1, 1, 1, "same", "relu", act_scale=0.05)
    main = tw._conv_layer(rng, (H, H, S), in_q, False, E3, 3, 1, "same", "relu", act_scale=0.05)
    join = dict(op="concatenation", skip=0, swap=True, axis=-1, out_shape=(1, H, H, E1 + E3), out_q=side["out_q"])
    return in_q, side, main, join


def op_case(idx, a):
    import torch
    from microflow_rs_amd import _lib, ops
    H, S, E1, E3 = CASES[idx]
    batch = batch_of(idx, a)
    rows = H * H
    q = (0.05, -128)
    op = ops.prepare_concatenation(rows, E1, E3, q, q, q)
    x = torch.randint(-128, 128, (batch * rows, E1), dtype=torch.int8, device="cuda")
    y = torch.randint(-128, 128, (batch * rows, E3), dtype=torch.int8, device="cuda")
    out = torch.empty((batch * rows, E1 + E3), dtype=torch.int8, device="cuda")
    src = torch.randint(-128, 128, (batch * rows, E1 + E3), dtype=torch.int8, device="cuda")
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream

    def ours():
        _lib.check(L.mf_op_run2(op._h, x.data_ptr(), y.data_ptr(), batch, out.data_ptr(), stream))
    ours()
    assert bool(torch.equal(out, torch.cat((x, y), dim=-1)))
    t_o = [median_ms(ours, a.reps) for _ in range(REPEATS)]
    t_c = [median_ms(lambda: torch.cat((x, y), dim=-1, out=out), a.reps) for _ in range(REPEATS)]
    t_d = [median_ms(lambda: out.copy_(src), a.reps) for _ in range(REPEATS)]
    mo, mc, md = np.median(t_o), np.median(t_c), np.median(t_d)
    gb = 2.0 * batch * rows * (E1 + E3) / 1e9
    print("op    %2dx%2d %3d+%3d batch %5d  %s %8.4f ms (spread %.3f, %.2f TB/s = %.2f of HBM)  torch.cat %8.4f ms (spread %.3f)  copy %8.4f ms (spread %.3f)"
          "  ours/cat %.3f  ours/copy %.3f" % (H, H, E1, E3, batch, op.kernel, mo, spread(t_o), gb / mo, gb / mo / HBM_TBS, mc, spread(t_c), md, spread(t_d),
                                                mo / mc, mo / md), flush=True)


def ops_case(idx, a):
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    from microflow_rs_amd import _lib, ops
    from microflow_rs_amd.tensor import FusedActivation, TensorViewPadding
    H, S, E1, E3 = CASES[idx]
    batch = batch_of(idx, a)
    in_q, side, main, join = layers_of(idx)
    one = mf.Model(tw.build_model((1, H, H, S), in_q, [side], tw.INT8))     # the convolution alone, for its folded constants
    c0, c1, _, _ = one.op_constants(0)
    conv = ops.prepare_conv_2d((H, H, S), np.asarray(side["filters"], np.int8), side["fzp"], in_q[1], side["out_q"][0], side["out_q"][1],
                               ops.Conv2DOptions(FusedActivation.RELU, TensorViewPadding.SAME, (1, 1)), (c0, c1), (H, H))
    t = torch.randint(-128, 128, (batch, H * H * S), dtype=torch.int8, device="cuda")
    r = torch.randint(-128, 128, (batch * H * H, E3), dtype=torch.int8, device="cuda")
    sbuf = torch.empty((batch * H * H, E1), dtype=torch.int8, device="cuda")
    out = torch.empty((batch * H * H, E1 + E3), dtype=torch.int8, device="cuda")
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream

    def run_conv():
        _lib.check(L.mf_op_run(conv._h, t.data_ptr(), batch, sbuf.data_ptr(), stream))

    def run_cat():
        torch.cat((sbuf, r), dim=-1, out=out)
    tc = [median_ms(run_conv, a.reps) for _ in range(REPEATS)]
    ta = [median_ms(run_cat, a.reps) for _ in range(REPEATS)]
    sums = [p + q for p, q in zip(tc, ta)]
    print("ops   %2dx%2dx%3d -> %3d + %3d batch %5d  %s %8.4f ms (spread %.3f) + torch.cat %8.4f ms (spread %.3f) = %8.4f ms (spread %.3f)" % (
        H, H, S, E1, E3, batch, conv.kernel, np.median(tc), spread(tc), np.median(ta), spread(ta), np.median(sums), spread(sums)), flush=True)


def model_case(idx, a):
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    H, S, E1, E3 = CASES[idx]
    batch = batch_of(idx, a)
    in_q, side, main, join = layers_of(idx)
    m = mf.Model(tw.build_model((1, H, H, S), in_q, [dict(side, side_of=-1), main, join], tw.INT8))
    m.prepare(batch)
    x = torch.randint(-128, 128, (batch, m.input_elems), dtype=torch.int8, device="cuda")
    out = torch.empty((batch, m.output_elems), dtype=torch.int8, device="cuda")
    names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    ts = [m.time_device(x, out, batch, warmup=3, iters=a.reps, per_op=True)[1][2] for _ in range(REPEATS)]
    got = out.clone()
    m.set_fusion(False)
    m.run_quantized(x, out=out)
    same = bool(torch.equal(out, got))
    print("model %2dx%2dx%3d -> %3d + %3d batch %5d  %s | %s  %8.4f ms (spread %.3f)  same as fusion off=%s" % (
        H, H, S, E1, E3, batch, names[0], names[2], np.median(ts), spread(ts), same), flush=True)
    assert same


def squeezenet(a):
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    batch = min(a.batch, 16384)   # (the stem's 32 x 32 x 64 output: 1 GiB per activation buffer)
    m = mf.Model(tw.squeezenet(np.random.default_rng(42), 64))
    m.prepare(batch)
    x = torch.randint(-128, 128, (batch, m.input_elems), dtype=torch.int8, device="cuda")
    out = torch.empty((batch, m.output_elems), dtype=torch.int8, device="cuda")
    names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    runs = [m.time_device(x, out, batch, warmup=2, iters=a.reps, per_op=True) for _ in range(REPEATS)]
    tot = [r[0] for r in runs]
    got = out.clone()
    m.set_fusion(False)
    m.run_quantized(x, out=out)
    same = bool(torch.equal(out, got))
    print("squeezenet-64 batch %d  %8.4f ms (spread %.3f)  same as fusion off=%s" % (batch, np.median(tot), spread(tot), same), flush=True)
    for i, n in enumerate(names):
        per = [r[1][i] for r in runs]
        print("  %2d %-44s %8.4f ms" % (i, n, np.median(per)), flush=True)
    assert same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--cap-gib", type=float, default=4.0, help="the largest tensor of a case stays within this many GiB (the batch is cut)")
    ap.add_argument("--mode", choices=("op", "ops", "model", "squeezenet"), default="model")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree whose library and writer are used")
    ap.add_argument("--only", type=int, default=-1, help="run this case in this process (what the parent process starts per case)")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tools"))
    if a.only >= 0:
        import torch
        assert torch.cuda.is_available(), "needs the GPU"
        return squeezenet(a) if a.mode == "squeezenet" else {"op": op_case, "ops": ops_case, "model": model_case}[a.mode](a.only, a)
    for idx in range(1 if a.mode == "squeezenet" else len(CASES)):
        args = ["--mode", a.mode, "--root", root, "--reps", str(a.reps), "--batch", str(a.batch), "--cap-gib", str(a.cap_gib), "--only", str(idx)]
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            sys.exit("case %s ran into its %d s limit: nothing more is started" % (" ".join(args), STEP_TIMEOUT))
        if r.returncode != 0:
            sys.exit("case %s ended with status %d: nothing more is started" % (" ".join(args), r.returncode))


if __name__ == "__main__":
    main()
