#!/usr/bin/env python3
"""GPU box: which launch every operator of a fixed corpus of models gets, one line per operator -- index, kernel name, epilogue mode.
Two commits route alike exactly when their dumps are byte-identical (profiles/r11: the fused-group refactor against its parent).

    python scripts/routing_dump.py [--out FILE]        # the environment's MF_* switches apply (MF_DEV=1 MF_NO_STAGE=1 ...)

Autotune stays off, so that model creation is deterministic.  Every model is prepared in a child process of its own under a time
limit; the first child that fails or runs into its limit ends the run, and nothing more is started."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

STEP_TIMEOUT = 120  # seconds per model
BLOCKS = [(24, 5, 1, 8), (72, 5, 2, 24), (120, 5, 1, 40), (24, 7, 1, 24), (36, 3, 1, 16)]


def corpus():
    """[(name, maker of a path or a flatbuffer)]: names and seeds are fixed"""
    import tflite_writer as tw
    import time_pair_band as tpb
    rng = np.random.default_rng
    c = [(n, (lambda n=n: os.path.join(ROOT, "models", n + ".tflite"))) for n in ("sine", "speech", "person_detect")]
    c += [("pd_like-%d" % side, (lambda side=side: tw.person_detect_like(rng(side), side))) for side in (96, 64, 128)]
    c += [("pd_like-96-w0.5", lambda: tw.person_detect_like(rng(11), 96, 0.5)),
          ("pd_like-96-wzp", lambda: tw.person_detect_like(rng(12), 96, 1.0, tw.INT8, True)),
          ("pd_like-96-u8", lambda: tw.person_detect_like(rng(13), 96, 1.0, tw.UINT8)),
          ("pd_like-64-u8-wzp", lambda: tw.person_detect_like(rng(14), 64, 1.0, tw.UINT8, True)),
          ("mlp-20-33-7", lambda: tw.mlp(rng(20), [20, 33, 7])),
          ("mlp-20-33-7-sm", lambda: tw.mlp(rng(21), [20, 33, 7], softmax=True)),
          ("pool_head-5x5x320", lambda: tw.pool_head(rng(22), (5, 5, 320), (17, 10), softmax=True)),
          ("kws-dw", lambda: tw.kws_like(rng(23), (10, 8), ("dw", 8, 3, 3, (1, 1), "same"), 4)),
          ("kws-conv", lambda: tw.kws_like(rng(24), (12, 16), ("conv", 12, 5, 2, (1, 2), "valid"), 12)),
          ("inverted_residual", lambda: tw.inverted_residual_net(rng(25), (28, 28, 8), BLOCKS)),
          ("conv_net", lambda: tw.conv_net(rng(26), (24, 24, 16), [("conv", 32, 3, 2), ("dw", 0, 3, 1), ("conv", 48, 1, 1), ("dw", 0, 3, 2), ("conv", 64, 1, 1)], head=10))]
    bands = [("band", i, s) for i, s in enumerate(tpb.SHAPES)] + [("band-deep", 0, tpb.DEEP_SHAPES[0])]
    for tag, i, (H, W, C, S, N, _batch) in bands:
        c.append(("%s-%dx%dx%d%s-%d" % (tag, H, W, C, "s2" if S == 2 else "", N),
                  lambda i=i, H=H, W=W, C=C, S=S, N=N: tw.conv_net(rng(i), (H, W, C), [("dw", 0, 3, S), ("conv", N, 1, 1)], act_scale=6.0 / 255.0)))
    return c


def corpus_all():
    """corpus() -- whose names and bytes tests/golden/writer_blobs.json pins -- and behind it the models of operators added since: new
    entries at the end only, so that an older tree's dump is a prefix of this one's"""
    import tflite_writer as tw
    rng = np.random.default_rng
    return corpus() + [("keras_mobilenet_v2-96-w0.25", lambda: tw.keras_mobilenet_v2(rng(40), 96, 0.25)),   # PAD, MEAN
                       ("keras_resnet_stem-64", lambda: tw.keras_resnet_stem(rng(41), 64)),
                       ("squeezenet-64", lambda: tw.squeezenet(rng(42), 64)),                                   # CONCATENATION
                       ("fire_net-8x8x64-s2", lambda: tw.fire_net(rng(43), (8, 8, 64), [(16, 64, 64), (32, 128, 128, 2, "31")], head=10)),
                       ("dense_net-8x8x16", lambda: tw.dense_net(rng(44), (8, 8, 16), (16, 32), head=10))]


def one(idx):
    import microflow_rs_amd as mf
    name, make = corpus_all()[idx]
    m = mf.Model(make(), autotune=False)
    m.prepare(64)
    print("# " + name)
    for i in range(m.num_ops):
        print("%d %s %d" % (i, m.op(i)["kernel"], m.op_epilogue_mode(i)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", type=int, default=-1, help="dump this model in this process (what the parent starts per model)")
    ap.add_argument("--out", default=None, help="write the dump here instead of standard output")
    a = ap.parse_args()
    if a.only >= 0:
        return one(a.only)
    lines = []
    for idx in range(len(corpus_all())):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", str(idx)], timeout=STEP_TIMEOUT, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            sys.exit("model %d ran into its %d s limit: nothing more is started" % (idx, STEP_TIMEOUT))
        if r.returncode != 0:
            sys.exit("model %d ended with status %d: nothing more is started" % (idx, r.returncode))
        lines.append(r.stdout)
    text = "".join(lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
