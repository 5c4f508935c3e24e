#!/usr/bin/env python3
"""GPU box: PAD, and PAD + VALID convolution as one launch, against what they replace.

    python scripts/time_pad.py --mode pad                  # the PAD operator (pad_c4 / pad_generic) against torch.nn.functional.pad on
                                                           # the same int8 tensor and against a device copy of the output's bytes, in one
                                                           # process; HBM fraction on input + output bytes; parity against torch's pad
    python scripts/time_pad.py --mode ops  [--root DIR]    # the yardstick of the one launch: the VALID convolution on the ALREADY padded
                                                           # input through the operator API + a device copy of the padded tensor -- what
                                                           # a caller who padded beforehand would pay.  Runs on any commit: --root names
                                                           # the tree whose library is measured (the parent)
    python scripts/time_pad.py --mode model                # a model [PAD, convolution]: the PAD's slot + the convolution's of
                                                           # mf_model_time_device(per_op) -- the one launch, or under
                                                           # MF_DEV=1 MF_NO_PAD_CONV=1 the two; parity against fusion off in the same run
    python scripts/time_pad.py --mode mobilenet            # keras_mobilenet_v2 at 96x96, batch 65 536: per-operator names and times,
                                                           # inferences/s, inverted_residual_net's beside it for scale

Every figure is the median of --reps (20) runs timed with HIP events after warm-up, in three repeats: the median of the three medians
and their spread ((max - min) / median).  Every case runs in a child process of its own under a time limit; the first that fails or
runs into its limit ends the run."""
import argparse
import os
import subprocess
import sys

import numpy as np

HBM_PEAK_GBS = 8000.0   # benchlib/roofline.py
# the PAD kernel: (H, W, C, (top, bottom, left, right), batch) -- tensors of tens of MiB
PAD_CASES = [(112, 112, 96, (0, 1, 0, 1), 32), (56, 56, 144, (0, 1, 0, 1), 96), (28, 28, 192, (0, 1, 0, 1), 256), (14, 14, 576, (0, 1, 0, 1), 384),
             (224, 224, 3, (3, 3, 3, 3), 256)]
# the one launch: (depthwise, H, W, C, K, stride, pads, N, batch): MobileNet-v2's stride-2 depthwise layers, its stem, ResNet's stem
CONV_CASES = [(True, 112, 112, 96, 3, 2, (0, 1, 0, 1), 96, 32), (True, 56, 56, 144, 3, 2, (0, 1, 0, 1), 144, 96),
              (True, 28, 28, 192, 3, 2, (0, 1, 0, 1), 192, 256), (True, 14, 14, 576, 3, 2, (0, 1, 0, 1), 576, 384),
              (False, 224, 224, 3, 3, 2, (0, 1, 0, 1), 32, 64), (False, 224, 224, 3, 7, 2, (3, 3, 3, 3), 64, 64),
              (False, 96, 96, 3, 3, 2, (0, 1, 0, 1), 8, 1024), (False, 28, 28, 32, 3, 2, (0, 1, 0, 1), 64, 256)]
STEP_TIMEOUT = 300
REPEATS = 3
IRN_BLOCKS = [(24, 5, 1, 8), (72, 5, 2, 24), (120, 5, 1, 40), (24, 7, 1, 24), (36, 3, 1, 16)]


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


def pad_case(idx, reps):
    import torch
    import torch.nn.functional as F
    from microflow_rs_amd import _lib, ops
    H, W, C, (t, b, l, r), batch = PAD_CASES[idx]
    zp = -7
    op = ops.prepare_pad((H, W, C), ((t, b), (l, r)), zp)
    x = torch.randint(-128, 128, (batch, H, W, C), dtype=torch.int8, device="cuda")
    out = torch.empty((batch, H + t + b, W + l + r, C), dtype=torch.int8, device="cuda")
    dup = torch.empty_like(out)
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream

    def ours():
        _lib.check(L.mf_op_run(op._h, x.data_ptr(), batch, out.data_ptr(), stream))

    def theirs():
        return F.pad(x, (0, 0, l, r, t, b), value=zp)

    def copy():
        dup.copy_(out)
    ours()
    assert torch.equal(out, theirs()), "PAD differs from torch.nn.functional.pad"
    to, tt, tc = ([median_ms(f, reps) for _ in range(REPEATS)] for f in (ours, theirs, copy))
    moved = x.numel() + out.numel()
    frac = moved / (np.median(to) * 1e-3) / (HBM_PEAK_GBS * 1e9)
    print("pad   %3dx%3dx%3d (%d,%d,%d,%d) batch %4d  %-12s %8.4f ms (spread %.3f, %.0f %% of HBM peak on in + out)  torch pad %8.4f ms (spread %.3f)  "
          "copy of the output %8.4f ms (spread %.3f)  ours / torch %.3f" % (H, W, C, t, b, l, r, batch, op.kernel, np.median(to), spread(to), 100 * frac,
                                                                         np.median(tt), spread(tt), np.median(tc), spread(tc), np.median(to) / np.median(tt)), flush=True)


def layers_of(idx):
    import tflite_writer as tw
    dw, H, W, C, K, S, (t, b, l, r), N, batch = CONV_CASES[idx]
    rng = np.random.default_rng(700 + idx)
    in_q = (0.05, -3)
    conv = tw._conv_layer(rng, (H + t + b, W + l + r, C), in_q, dw, N, K, S, "valid", "relu6")
    return in_q, conv


def ops_case(idx, reps):
    """the parent's way: the padded tensor exists (a device copy of it is what producing it costs at least), the VALID convolution runs on it"""
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    from microflow_rs_amd import _lib, ops
    from microflow_rs_amd.tensor import FusedActivation, TensorViewPadding
    dw, H, W, C, K, S, (t, b, l, r), N, batch = CONV_CASES[idx]
    in_q, conv = layers_of(idx)
    PH, PW = H + t + b, W + l + r
    one = mf.Model(tw.build_model((1, PH, PW, C), in_q, [conv], tw.INT8))
    c0, c1, _, _ = one.op_constants(0)
    OH, OW = conv["out_shape"][1:3]
    if dw:
        op = ops.prepare_depthwise_conv_2d((PH, PW, C), np.asarray(conv["weights"], np.int8), conv["fzp"], in_q[1], conv["out_q"][0], conv["out_q"][1],
                                           ops.DepthwiseConv2DOptions(FusedActivation.RELU6, TensorViewPadding.VALID, (S, S)), (c0, c1), (OH, OW))
    else:
        op = ops.prepare_conv_2d((PH, PW, C), np.asarray(conv["filters"], np.int8), conv["fzp"], in_q[1], conv["out_q"][0], conv["out_q"][1],
                                 ops.Conv2DOptions(FusedActivation.RELU6, TensorViewPadding.VALID, (S, S)), (c0, c1), (OH, OW))
    xp = torch.randint(-128, 128, (batch, PH * PW * C), dtype=torch.int8, device="cuda")
    dup = torch.empty_like(xp)
    out = torch.empty((batch, OH * OW * N), dtype=torch.int8, device="cuda")
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream

    def run_conv():
        _lib.check(L.mf_op_run(op._h, xp.data_ptr(), batch, out.data_ptr(), stream))

    def copy():
        dup.copy_(xp)
    tcv = [median_ms(run_conv, reps) for _ in range(REPEATS)]
    tcp = [median_ms(copy, reps) for _ in range(REPEATS)]
    sums = [a + c for a, c in zip(tcv, tcp)]
    print("ops   %s %3dx%3dx%3d %dx%d s%d (%d,%d,%d,%d) -> %3d batch %4d  %s on the padded input %8.4f ms + copy of the padded tensor %8.4f ms = %8.4f ms (spread %.3f)" % (
        "dw  " if dw else "conv", H, W, C, K, K, S, t, b, l, r, N, batch, op.kernel, np.median(tcv), np.median(tcp), np.median(sums), spread(sums)), flush=True)


def model_case(idx, reps):
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    dw, H, W, C, K, S, (t, b, l, r), N, batch = CONV_CASES[idx]
    in_q, conv = layers_of(idx)
    m = mf.Model(tw.build_model((1, H, W, C), in_q, [tw._pad_layer((H, W, C), in_q, ((t, b), (l, r))), conv], tw.INT8))
    m.prepare(batch)
    x = torch.randint(-128, 128, (batch, m.input_elems), dtype=torch.int8, device="cuda")
    out = torch.empty((batch, m.output_elems), dtype=torch.int8, device="cuda")
    names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    ts = [sum(m.time_device(x, out, batch, warmup=3, iters=reps, per_op=True)[1][:2]) for _ in range(REPEATS)]
    got = out.clone()
    m.set_fusion(False)
    m.run_quantized(x, out=out)
    same = bool(torch.equal(out, got))
    print("model %s %3dx%3dx%3d %dx%d s%d (%d,%d,%d,%d) -> %3d batch %4d  %s | %s  %8.4f ms (spread %.3f)  same as fusion off=%s" % (
        "dw  " if dw else "conv", H, W, C, K, K, S, t, b, l, r, N, batch, names[0], names[1], np.median(ts), spread(ts), same), flush=True)
    assert same


def mobilenet(idx, reps):
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    batch = 65536
    name, blob = [("keras_mobilenet_v2 96x96 w0.25", lambda: tw.keras_mobilenet_v2(np.random.default_rng(40), 96, 0.25)),
                  ("inverted_residual_net 28x28x8", lambda: tw.inverted_residual_net(np.random.default_rng(25), (28, 28, 8), IRN_BLOCKS))][idx]
    m = mf.Model(blob())
    m.prepare(batch)
    x = torch.randint(-128, 128, (batch, m.input_elems), dtype=torch.int8, device="cuda")
    out = torch.empty((batch, m.output_elems), dtype=torch.int8, device="cuda")
    names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    runs = [m.time_device(x, out, batch, warmup=2, iters=reps, per_op=True) for _ in range(REPEATS)]
    tot = [r[0] for r in runs]
    got = out.clone()
    m.set_fusion(False)
    m.run_quantized(x, out=out)
    same = bool(torch.equal(out, got))
    print("%s batch %d  %8.3f ms (spread %.3f)  %.0f inferences/s  same as fusion off=%s" % (name, batch, np.median(tot), spread(tot),
                                                                                          batch / (np.median(tot) * 1e-3), same), flush=True)
    for i, n in enumerate(names):
        print("  %2d %-12s %-60s %8.4f ms" % (i, m.op(i)["name"], n, np.median([r[1][i] for r in runs])), flush=True)
    assert same


MODES = {"pad": (pad_case, len(PAD_CASES)), "ops": (ops_case, len(CONV_CASES)), "model": (model_case, len(CONV_CASES)), "mobilenet": (mobilenet, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mode", choices=tuple(MODES), default="model")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree whose library and writer are used")
    ap.add_argument("--only", type=int, default=-1, help="run this case in this process (what the parent process starts per case)")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tools"))
    if a.only >= 0:
        import torch
        assert torch.cuda.is_available(), "needs the GPU"
        return MODES[a.mode][0](a.only, a.reps)
    for idx in range(MODES[a.mode][1]):
        args = ["--mode", a.mode, "--root", root, "--reps", str(a.reps), "--only", str(idx)]
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            sys.exit("case %s ran into its %d s limit: nothing more is started" % (" ".join(args), STEP_TIMEOUT))
        if r.returncode != 0:
            sys.exit("case %s ended with status %d: nothing more is started" % (" ".join(args), r.returncode))


if __name__ == "__main__":
    main()
