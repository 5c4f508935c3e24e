#!/usr/bin/env python3
"""GPU box: a ResNet projection shortcut -- the 1x1 Conv2D on the skip edge and the ADD that reads it -- as ONE launch
(k_side_join.hip: shortcut_add_rt) against the two launches it replaces, at the shapes of ResNet-8's stacks, a stride-1 widening and ResNet-18's 128 -> 256, batch 65 536.

    python scripts/time_shortcut.py --mode ops   [--root DIR]   # the two operators through the operator API: mf_conv_2d_create +
                                                                 # mf_add_create, mf_op_run / mf_op_run2.  Runs on any commit that has
                                                                 # ADD: --root names the tree whose library is measured (the parent)
    python scripts/time_shortcut.py --mode model                 # a model [side Conv2D, main Conv2D 1x1, ADD]: the ADD's slot of
                                                                 # mf_model_time_device(per_op): the fused launch, or -- under
                                                                 # MF_DEV=1 MF_NO_SHORTCUT_ADD=1 -- the two launches in the same slot
    python scripts/time_shortcut.py --mode resnet8               # the whole tools/tflite_writer.resnet8: per-operator kernel names
                                                                 # and times, the total, parity against fusion off in the same run

Every figure is the median of --reps (20) runs timed with HIP events after warm-up, in three repeats: the median of the three medians
and their spread ((max - min) / median).  The yardstick is --mode ops on the PARENT commit (summed medians of the two operators);
the branch under the switch is the cross-check.  The same quantisations and weights everywhere: the seeds are fixed here.

Every case runs in a child process of its own under a time limit; the first that fails or runs into its limit ends the run."""
import argparse
import os
import subprocess
import sys

import numpy as np

BATCH = 65536
# (H, W, C, stride, N)
# (the three shortcuts of ResNet-8's geometry scaled up one stack, a stride-1 widening, and ResNet-18's 128 -> 256: two k steps, four waves per chunk)
CASES = [(32, 32, 16, 2, 32), (16, 16, 32, 2, 64), (8, 8, 64, 2, 128), (16, 16, 32, 1, 64), (8, 8, 128, 2, 256)]
STEP_TIMEOUT = 300
REPEATS = 3


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


def layers_of(idx):
    """(in_q, side conv layer, main conv layer, add layer) of case idx, from the writer's per-layer helpers (the same on every commit)"""
    import tflite_writer as tw
    H, W, C, s, N = CASES[idx]
    rng = np.random.default_rng(500 + idx)
    in_q = (0.05, -3)
    side = tw._conv_layer(rng, (H, W, C), in_q, False, N, 1, s, "same", "none")
    main = tw._conv_layer(rng, (H, W, C), in_q, False, N, 1, s, "same", "none")
    add = tw._add_layer(rng, 0, side["out_shape"], main["out_q"], side["out_q"], "relu")
    return in_q, side, main, add


def ops_case(idx, reps):
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    from microflow_rs_amd import _lib, ops
    from microflow_rs_amd.tensor import FusedActivation, TensorViewPadding
    H, W, C, s, N = CASES[idx]
    in_q, side, main, add = layers_of(idx)
    one = mf.Model(tw.build_model((1, H, W, C), in_q, [side], tw.INT8))     # the convolution alone, for its folded constants
    c0, c1, _, _ = one.op_constants(0)
    OH, OW = side["out_shape"][1:3]
    conv = ops.prepare_conv_2d((H, W, C), np.asarray(side["filters"], np.int8), side["fzp"], in_q[1], side["out_q"][0], side["out_q"][1],
                               ops.Conv2DOptions(FusedActivation.NONE, TensorViewPadding.SAME, (s, s)), (c0, c1), (OH, OW))
    elems = OH * OW * N
    addop = ops.prepare_add(elems, main["out_q"], side["out_q"], add["out_q"], ops.AddOptions(FusedActivation.RELU))
    t = torch.randint(-128, 128, (BATCH, H * W * C), dtype=torch.int8, device="cuda")
    r = torch.randint(-128, 128, (BATCH, elems), dtype=torch.int8, device="cuda")
    sbuf, out = torch.empty_like(r), torch.empty_like(r)
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream

    def run_conv():
        _lib.check(L.mf_op_run(conv._h, t.data_ptr(), BATCH, sbuf.data_ptr(), stream))

    def run_add():
        _lib.check(L.mf_op_run2(addop._h, r.data_ptr(), sbuf.data_ptr(), BATCH, out.data_ptr(), stream))

    def both():
        run_conv()
        run_add()
    tc = [median_ms(run_conv, reps) for _ in range(REPEATS)]
    ta = [median_ms(run_add, reps) for _ in range(REPEATS)]
    tb = [median_ms(both, reps) for _ in range(REPEATS)]
    sums = [a + b for a, b in zip(tc, ta)]
    print("ops   %2dx%2dx%3d s%d -> %3d batch %d  %s %8.4f ms + %s %8.4f ms = %8.4f ms (spread %.3f)  back to back %8.4f ms (spread %.3f)" % (
        H, W, C, s, N, BATCH, conv.kernel, np.median(tc), addop.kernel, np.median(ta), np.median(sums), spread(sums), np.median(tb), spread(tb)), flush=True)


def model_case(idx, reps):
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    H, W, C, s, N = CASES[idx]
    in_q, side, main, add = layers_of(idx)
    m = mf.Model(tw.build_model((1, H, W, C), in_q, [dict(side, side_of=-1), main, add], tw.INT8))
    m.prepare(BATCH)
    x = torch.randint(-128, 128, (BATCH, m.input_elems), dtype=torch.int8, device="cuda")
    out = torch.empty((BATCH, m.output_elems), dtype=torch.int8, device="cuda")
    names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    ts = [m.time_device(x, out, BATCH, warmup=3, iters=reps, per_op=True)[1][2] for _ in range(REPEATS)]
    got = out.clone()
    m.set_fusion(False)
    m.run_quantized(x, out=out)
    same = bool(torch.equal(out, got))
    print("model %2dx%2dx%3d s%d -> %3d batch %d  %s | %s  %8.4f ms (spread %.3f)  same as fusion off=%s" % (
        H, W, C, s, N, BATCH, names[0], names[2], np.median(ts), spread(ts), same), flush=True)
    assert same


def resnet8(reps):
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    m = mf.Model(tw.resnet8(np.random.default_rng(1)))
    m.prepare(BATCH)
    x = torch.randint(-128, 128, (BATCH, m.input_elems), dtype=torch.int8, device="cuda")
    out = torch.empty((BATCH, m.output_elems), dtype=torch.int8, device="cuda")
    names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    runs = [m.time_device(x, out, BATCH, warmup=2, iters=reps, per_op=True) for _ in range(REPEATS)]
    tot = [r[0] for r in runs]
    got = out.clone()
    m.set_fusion(False)
    m.run_quantized(x, out=out)
    same = bool(torch.equal(out, got))
    print("resnet8 batch %d  %8.4f ms (spread %.3f)  same as fusion off=%s" % (BATCH, np.median(tot), spread(tot), same), flush=True)
    for i, n in enumerate(names):
        per = [r[1][i] for r in runs]
        print("  %2d %-44s %8.4f ms" % (i, n, np.median(per)), flush=True)
    assert same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mode", choices=("ops", "model", "resnet8"), default="model")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree whose library and writer are used")
    ap.add_argument("--only", type=int, default=-1, help="run this case in this process (what the parent process starts per case)")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tools"))
    if a.only >= 0:
        import torch
        assert torch.cuda.is_available(), "needs the GPU"
        return {"ops": ops_case, "model": model_case}[a.mode](a.only, a.reps) if a.mode != "resnet8" else resnet8(a.reps)
    for idx in range(1 if a.mode == "resnet8" else len(CASES)):
        args = ["--mode", a.mode, "--root", root, "--reps", str(a.reps), "--only", str(idx)]
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            sys.exit("case %s ran into its %d s limit: nothing more is started" % (" ".join(args), STEP_TIMEOUT))
        if r.returncode != 0:
            sys.exit("case %s ended with status %d: nothing more is started" % (" ".join(args), r.returncode))


if __name__ == "__main__":
    main()
