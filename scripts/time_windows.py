#!/usr/bin/env python3
"""GPU box: a model over about 65 536 sliding windows of one source (Model.run_windows / predict_windows; k_windows.hip) against
what a caller could do before the window entry points existed, in the same process, back to back.

    python scripts/time_windows.py [--reps 20] [--sweep] [--only 3]

Per case (a T source and, with the predict entries, an f32 source):
  (a) run_windows on a device-resident source
  (b) torch's strided view of the source made contiguous on the device (unfold(...).contiguous()), then run_quantized
  (c) run_quantized on an already resident materialised batch: the floor
  (d) run_windows from host memory: the source crosses once
  (e) run_quantized from host-materialised windows: every window crosses
  gather: the gather kernel alone (mf.gather_windows); its rate in output bytes, and source + output bytes as a fraction of the
          5.3 TB/s a plain copy reaches (scripts/ubench/hbm_copy.hip, profiles/r03/hbm_copy_ceiling.txt), beside a device copy of the
          same output bytes timed here
Each figure is the median of three repeats of a median of --reps runs (HIP events for the device paths, the wall clock for the
host-fed ones), with the spread of the three behind it; all paths' results are compared with (c)'s in the same run.  mem = device
bytes a path needs beyond the model's own buffers: (a) source + staging chunk + results, (b) source + materialised batch +
results.  --sweep: (a) at chunk sizes from 1024 windows to the whole batch.  Every case runs in a child process of its own under
a time limit, so that one case's trouble ends that case only."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

COPY_CEILING = 5.3e12
CASES = ["speech hop 1", "speech hop 2", "ds_cnn hop 1", "person_detect 480x640 hop 16"]
STEP_TIMEOUT = 420  # seconds per case


def build(idx):
    import microflow_rs_amd as mf
    import tflite_writer as tw
    models = os.path.join(ROOT, "models")
    if idx == 0:
        return mf.Model(os.path.join(models, "speech.tflite")), mf.Windows.frames(65536 + 48, 40, 49, hop=1)
    if idx == 1:
        return mf.Model(os.path.join(models, "speech.tflite")), mf.Windows.frames(2 * 65535 + 49, 40, 49, hop=2)
    if idx == 2:
        return mf.Model(tw.ds_cnn(np.random.default_rng(3))), mf.Windows.frames(65536 + 48, 10, 49, hop=1)
    return mf.Model(os.path.join(models, "person_detect.tflite")), mf.Windows.image((480, 640), (96, 96), 1, 16, n=75)


def thrice(fn, reps, device=True):
    """median and spread (max - min) of three repeats of a median of `reps` runs, ms"""
    import torch
    meds = []
    for _ in range(3):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            if device:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b))
            else:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
        meds.append(float(np.median(ts)))
    return float(np.median(meds)), max(meds) - min(meds)


def strided(src_d, w):
    """the windows as a strided view of the device source: what unfold() gives, for any description"""
    import torch
    ny = (w.src_rows - w.win_rows) // w.hop_rows + 1
    nx = (w.src_row_elems - w.win_row_elems) // w.hop_elems + 1
    return torch.as_strided(src_d, (w.n_sources, ny, nx, w.win_rows, w.win_row_elems),
                            (w.stride, w.hop_rows * w.pitch, w.hop_elems, w.pitch, 1))


def one(idx, reps, sweep):
    import torch
    import microflow_rs_amd as mf
    assert torch.cuda.is_available(), "needs the GPU"
    m, w = build(idx)
    n, E, N = w.total, w.window_elems, m.output_elems
    m.prepare(1)
    rng = np.random.default_rng(idx)
    host_reps = max(3, reps // 4)
    for f32 in (False, True):
        if f32:
            src = ((rng.integers(-128, 128, w.source_elems) - m.input_zero_point) * float(m.input_scale)).astype(np.float32)
            win, dense = m.predict_windows, m.predict
            odt = torch.float32
        else:
            src = rng.integers(-128, 128, w.source_elems).astype(np.int8)
            win, dense = m.run_windows, m.run_quantized
            odt = torch.int8
        esz = src.itemsize
        src_d = torch.as_tensor(src).cuda()
        out = torch.empty((n, N), dtype=odt, device="cuda")
        out2 = torch.empty((n, N), dtype=odt, device="cuda")
        mat_d = strided(src_d, w).contiguous().reshape(n, E)
        ref = dense(mat_d, out=out2).clone()

        def same(t):
            t = t if isinstance(t, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(t)).cuda()
            a, b = t.reshape(n, N), ref.reshape(n, N)
            return bool(torch.equal(a.view(torch.int32), b.view(torch.int32))) if f32 else bool(torch.equal(a, b))
        tag = "%-30s %s  %d windows x %d" % (CASES[idx], "f32" if f32 else "T  ", n, E)
        if sweep:
            c = 1024
            sizes = []
            while c < n:
                sizes.append(c)
                c *= 2
            for c in sizes + [n]:
                m.set_window_chunk(c)
                t, sp = thrice(lambda: win(src_d, w, out=out), reps)
                print("%s  sweep chunk %6d (%7.1f MB staged)  (a) %8.3f ms +-%.3f  same=%s" % (tag, c, c * E / 1e6, t, sp, same(out)), flush=True)
            m.set_window_chunk(0)
            continue
        ta, sa = thrice(lambda: win(src_d, w, out=out), reps)
        ok_a = same(out)
        tb, sb = thrice(lambda: dense(strided(src_d, w).contiguous().reshape(n, E), out=out2), reps)
        ok_b = same(out2)
        tc, sc = thrice(lambda: dense(mat_d, out=out2), reps)
        td, sd = thrice(lambda: win(src, w), host_reps, device=False)
        ok_d = same(win(src, w))
        mat_h = w.materialize(src)
        te, se = thrice(lambda: dense(mat_h), host_reps, device=False)
        ok_e = same(dense(mat_h))
        del mat_h
        g_out = torch.empty((n, E), dtype=torch.int8, device="cuda")
        q = (float(m.input_scale), int(m.input_zero_point), np.int8) if f32 else None
        tg, sg = thrice(lambda: mf.gather_windows(src_d, w, quantize=q, out=g_out), reps)
        g_out2 = torch.empty_like(g_out)
        tcp, _ = thrice(lambda: g_out2.copy_(g_out), reps)
        chunk_bytes = min(n, max(256, ((128 << 20) // E) & ~255)) * E
        mem_a = src.nbytes + chunk_bytes + n * N * out.element_size()
        mem_b = src.nbytes + n * E * esz + n * N * out.element_size()
        slack = max(sa, sb)
        print("%s\n    (a) %8.3f ms +-%.3f   (b) %8.3f ms +-%.3f   (c) %8.3f ms +-%.3f   (d) %8.3f ms +-%.3f   (e) %8.3f ms +-%.3f\n"
              "    a<=b+spread: %s   d<e: %s   same: a=%s b=%s d=%s e=%s\n"
              "    gather %8.3f ms +-%.3f = %.2f TB/s out, (src + out) / 5.3 TB/s = %.3f; copy of the same bytes %.3f ms\n"
              "    mem (a) %.1f MB  (b) %.1f MB  x%.1f"
              % (tag, ta, sa, tb, sb, tc, sc, td, sd, te, se, ta <= tb + slack, td < te, ok_a, ok_b, ok_d, ok_e, tg, sg, n * E / (tg * 1e-3) / 1e12,
                 (src.nbytes + n * E) / (tg * 1e-3) / COPY_CEILING, tcp, mem_a / 1e6, mem_b / 1e6, mem_b / mem_a), flush=True)
        del mat_d, g_out, g_out2
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sweep", action="store_true", help="(a) at chunk sizes from 1024 windows to the whole batch")
    ap.add_argument("--only", type=int, default=-1, help="run this case in this process (what the parent starts per case)")
    a = ap.parse_args()
    if a.only >= 0:
        return one(a.only, a.reps, a.sweep)
    for idx in range(len(CASES)):
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--only", str(idx)] + (["--sweep"] if a.sweep else [])
        try:
            r = subprocess.run(cmd, timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            sys.exit("case %d ran into its %d s limit: nothing more is started" % (idx, STEP_TIMEOUT))
        if r.returncode != 0:
            sys.exit("case %d ended with status %d: nothing more is started" % (idx, r.returncode))


if __name__ == "__main__":
    main()
