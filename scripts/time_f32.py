#!/usr/bin/env python3
"""GPU box: M::predict (f32 in HBM -> f32 out) against run_quantized (int8 in, int8 out) on one model at one batch, in the same
process: median of HIP-event timings, spread = (max - min) / median, and parity (predict's floats are the dequantised bytes of
run_quantized on the same quantised input).

usage: time_f32.py MODEL BATCH [iters]     one measurement, in this process
       time_f32.py --all [iters]           the table of profiles/r09/f32_entry.txt: one child process per row, each with its own time limit
       time_f32.py --conv [iters]          the table of profiles/r10/f32_conv_entry.txt (Conv2D-stem models), in the same way
MODEL: person_detect | speech | sine (models/*.tflite), pd_like:SIDE (tools/tflite_writer.person_detect_like(side=SIDE)),
       mlp:K-N1-N2...[+sm] (tools/tflite_writer.mlp), pool_head:HxWxC-N1...[+sm] (tools/tflite_writer.pool_head),
       conv_net:HxWxC-L1-L2... (tools/tflite_writer.conv_net with head=10; a layer is cNkKsS, a KxK Conv2D to N channels at stride S,
       or dwKsS, a KxK depthwise)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [("person_detect", 65536), ("speech", 4096), ("speech", 65536), ("sine", 65536), ("pd_like:64", 65536), ("mlp:20-33-7+sm", 65536),
        ("pool_head:7x7x64-10+sm", 65536)]
# conv_rows_lds: an RGB stem + two depthwise / 1x1 pairs, a LeNet-style greyscale stem; conv_gemm_rt: an ImageNet stem (row bands), a 128 x 128 stem
CONV_ROWS = [("conv_net:96x96x3-c16k3s2-dw3s1-c32k1s1-dw3s2-c64k1s1", 65536), ("conv_net:28x28x1-c6k5s1", 65536), ("conv_net:224x224x3-c64k7s2", 4096),
             ("conv_net:128x128x3-c16k3s2", 16384)]


def blob(name):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    if name in ("person_detect", "speech", "sine"):
        return open(os.path.join(ROOT, "models", name + ".tflite"), "rb").read()
    import tflite_writer as tw
    kind, arg = name.split(":", 1)
    rng = np.random.default_rng(41)
    if kind == "pd_like":
        return tw.person_detect_like(rng, side=int(arg))
    if kind == "mlp":
        sm = arg.endswith("+sm")
        return tw.mlp(rng, [int(v) for v in arg.replace("+sm", "").split("-")], softmax=sm)
    if kind == "pool_head":
        shape, _, sizes = arg.replace("+sm", "").partition("-")
        return tw.pool_head(rng, tuple(int(v) for v in shape.split("x")), tuple(int(v) for v in sizes.split("-")), softmax=arg.endswith("+sm"))
    if kind == "conv_net":
        import re
        shape, *layers = arg.split("-")
        convs = []
        for l in layers:
            f = re.fullmatch(r"(c(\d+)|dw)k?(\d+)s(\d+)", l)
            if not f:
                raise SystemExit("conv_net layer %r: cNkKsS or dwKsS" % l)
            convs.append(("dw", 0, int(f.group(3)), int(f.group(4))) if f.group(1) == "dw" else ("conv", int(f.group(2)), int(f.group(3)), int(f.group(4))))
        return tw.conv_net(rng, tuple(int(v) for v in shape.split("x")), convs, head=10)
    raise SystemExit("unknown model %r" % name)


def one(name, B, iters):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import microflow_rs_amd as mf
    from microflow_rs_amd import _lib
    from microflow_rs_amd.model import synth_i8
    m = mf.Model(blob(name))
    m.prepare(B, device=0)
    L = _lib.lib()
    u8 = m.dtype == np.uint8
    x = synth_i8(0x4D4643 + 3, 0, B * m.input_elems)
    if u8:
        x = x.view(torch.uint8)
    y = torch.empty(B * m.output_elems, dtype=x.dtype, device="cuda")
    xf = ((x.reshape(B, -1).float() - float(m.input_zero_point)) * float(m.input_scale)).contiguous()
    yf = torch.empty((B, m.output_elems), dtype=torch.float32, device="cuda")
    _lib.check(L.mf_model_set_stream(m._h, torch.cuda.current_stream().cuda_stream))

    def stat(fn):
        fn(), fn()
        ts = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        ts.sort()
        med = ts[len(ts) // 2]
        return med, (ts[-1] - ts[0]) / med

    ti, si = stat(lambda: _lib.check(L.mf_model_run_quantized(m._h, x.data_ptr(), B, y.data_ptr(), _lib.MF_MEM_DEVICE)))
    tf, sf = stat(lambda: _lib.check(L.mf_model_predict(m._h, xf.data_ptr(), B, yf.data_ptr(), _lib.MF_MEM_DEVICE)))
    torch.cuda.synchronize()
    same = bool(torch.equal(yf.reshape(-1), (y.float() - float(m.output_zero_point)) * float(m.output_scale)))
    ops = ""
    if hasattr(m, "device_ops"):
        a = m.device_ops()
        _lib.check(L.mf_model_predict(m._h, xf.data_ptr(), B, yf.data_ptr(), _lib.MF_MEM_DEVICE))
        b = m.device_ops()
        _lib.check(L.mf_model_run_quantized(m._h, x.data_ptr(), B, y.data_ptr(), _lib.MF_MEM_DEVICE))
        ops = " | launches predict %d run_quantized %d" % (b - a, m.device_ops() - b)
        torch.cuda.synchronize()
    print("%-16s %6d | run_quantized %8.4f ms (spread %4.1f %%) | predict %8.4f ms (spread %4.1f %%, %7.2f M/s) | parity %s%s"
          % (name, B, ti, 100 * si, tf, 100 * sf, B / tf / 1e3, same, ops), flush=True)
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] in ("--all", "--conv"):
        for name, B in (ROWS if sys.argv[1] == "--all" else CONV_ROWS):
            # (a failed or timed-out row ends the table: nothing more is started on a card that may be in trouble)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(B)] + sys.argv[2:3], timeout=240)
            if r.returncode:
                sys.exit(r.returncode)
        sys.exit(0)
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    sys.exit(one(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 20))
