#!/usr/bin/env python3
"""GPU box: RESIZE_BILINEAR (k_resize_bilinear.hip resize_bl_c4) against its yardsticks, in one process per case:

    python scripts/time_resize_bilinear.py [--batch 4096] [--gen-batch 256] [--reps 20]
        resize_bl_c4 at --batch images (parity with resize_bl_generic checked on the first --gen-batch images), and
          - resize_nn_c4 on the same shape: the same bytes moved with no arithmetic (generic where C % 4 != 0);
          - a device copy of (1 + sy sx) x the source bytes (read + write of that many bytes in all);
          - resize_bl_generic (set_generic) at --gen-batch images scaled to the batch.
        GB/s counts (1 + sy sx) H W C bytes per image; the HBM fraction is against 8 TB/s.

Every figure is the median of --reps samples of 10 back-to-back launches timed with HIP events after warm-up, in three repeats: the
median of the three medians and their spread ((max - min) / median).  Every case runs in a child process of its own under a time
limit; the first that fails ends the run."""
import argparse
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "scripts"))
from time_upconv import repeats  # noqa: E402

#         name           H   W   C   sy sx
CASES = [("8x8x64-x2",   8,  8,  64, 2, 2),
         ("16x16x32-x2", 16, 16, 32, 2, 2),
         ("32x32x16-x2", 32, 32, 16, 2, 2),
         ("16x16x21-x2", 16, 16, 21, 2, 2),   # (21 classes: bytes, the generic kernels on both sides)
         ("8x8x64-x4",   8,  8,  64, 4, 4),
         ("14x14x24-x4", 14, 14, 24, 4, 4),   # (dwords)
         ("16x16x32-x3", 16, 16, 32, 3, 3)]   # (the multiply-shift division)
STEP_TIMEOUT = 300
HBM_TBS = 8.0


def run_case(idx, a):
    sys.path.insert(0, HERE)
    import torch
    import microflow_rs_amd as mf
    name, H, W, C, sy, sx = CASES[idx]
    torch.manual_seed(idx)
    x = torch.randint(-128, 128, (a.batch, H, W, C), dtype=torch.int8, device="cuda")
    op = mf.ops.prepare_resize_bilinear((H, W, C), (sy, sx))
    nn = mf.ops.prepare_resize_nearest((H, W, C), (sy, sx))
    fast_name, y = op.kernel, op(x)
    ms, sp = repeats(lambda: op(x), a.reps)
    nms, nsp = repeats(lambda: nn(x), a.reps)
    nbytes = a.batch * H * W * C * (1 + sy * sx)
    src, dst = torch.empty(nbytes // 2, dtype=torch.int8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.int8, device="cuda")
    cms, csp = repeats(lambda: dst.copy_(src), a.reps)
    op.set_generic(True)
    xg = x[:a.gen_batch]
    ok = bool(torch.equal(op(xg), y[:a.gen_batch]))
    gms, gsp = repeats(lambda: op(xg), a.reps)
    gms *= a.batch / a.gen_batch
    gbs = nbytes / ms / 1e6
    print("%-12s | %-18s %.4f ms (+-%.1f%%) %.0f GB/s %.0f%% of HBM | %s %.4f ms (+-%.1f%%) bl / nn x%.2f | copy %.4f ms (+-%.1f%%) bl / copy x%.2f | generic %.2f ms (+-%.1f%%) | checksum %d | parity %s"
          % (name, fast_name, ms, 100 * sp, gbs, gbs / (10 * HBM_TBS), nn.kernel, nms, 100 * nsp, ms / nms, cms, 100 * csp, ms / cms, gms, 100 * gsp,
             int(y.to(torch.int64).sum()), "ok" if ok else "MISMATCH"))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--gen-batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--case", type=int, default=None)
    a = ap.parse_args()
    if a.case is not None:
        return run_case(a.case, a)
    for i in range(len(CASES)):
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(i), "--batch", str(a.batch), "--gen-batch", str(a.gen_batch), "--reps", str(a.reps)]
        r = subprocess.run(cmd, timeout=STEP_TIMEOUT, cwd=HERE)
        if r.returncode != 0:
            print("case %d failed (exit %d): stopping" % (i, r.returncode))
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
