"""The PAD + VALID convolution geometries that the host planner test (tests/test_pad_conv_plan_host.py) and the GPU tests
(tests/test_gpu_pad_conv.py, tests/test_gpu_pad_conv_steps.py) share, and the two-operator models written from them."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# name: (depthwise, H, W, C, K, stride, (top, bottom, left, right), N (Conv2D), filter zero points off the middle)
CASES = {
    "conv3s2_6x6x3": (False, 6, 6, 3, 3, 2, (0, 1, 0, 1), 8, False),
    "conv7s2_14x14x3": (False, 14, 14, 3, 7, 2, (3, 3, 3, 3), 8, False),
    "conv3s2_8x8x16": (False, 8, 8, 16, 3, 2, (0, 1, 0, 1), 32, False),
    "conv3s1_5x5x20": (False, 5, 5, 20, 3, 1, (1, 1, 1, 1), 12, False),
    "dw3s2_8x8x16": (True, 8, 8, 16, 3, 2, (0, 1, 0, 1), 16, False),
    "dw3s2_7x7x16": (True, 7, 7, 16, 3, 2, (1, 1, 1, 1), 16, False),
    "dw5s2_9x9x8": (True, 9, 9, 8, 5, 2, (1, 2, 1, 2), 8, False),
    "dw3s2_8x8x24_wz": (True, 8, 8, 24, 3, 2, (0, 1, 0, 1), 24, True),
}
# Refused by every planner, by their limits: the image rows are 85 bytes, no whole dwords, so conv_gemm_plan and dw_gemm_plan say no
# ((W C) % 4); conv_mm_plan says no (C % 16); and conv_rows_plan, which takes such rows, stops below 16 channels
REFUSED = {"conv3s1_5x5x17": (False, 5, 5, 17, 3, 1, (1, 1, 1, 1), 8, False)}


# ---- row bands, pads beyond the filter, filter zero points, odd bases, many steps (tests/test_gpu_pad_conv_steps.py) -------------------
# Every plan number beside a case is pinned by tests/test_pad_conv_plan_host.py (PINNED below): a later change of an LDS budget that
# turns a banded case into a single-band one, or changes the images per step, fails there and not silently here.
#
# BANDED: images too tall for one tile, so a step is one band of BH output rows (G = 1, NBANDS > 1); batch 4 on the GPU.
BANDED = {
    "conv3s1_90x64x16": (False, 90, 64, 16, 3, 1, (1, 1, 1, 1), 16, False),
    # H = 92, not 91: (91 + 1 - 3) / 2 + 1 = 45 output rows plan as three bands of exactly 15; 92 gives OH = 46 = 16 + 16 + 14, and
    # the last band's last window reads the PAD's bottom row.  The 91-row shapes stay beside them, pinned with the plan they do get.
    "conv3s2_92x64x16_wz": (False, 92, 64, 16, 3, 2, (0, 1, 0, 1), 16, True),
    "conv3s2_91x64x16_wz": (False, 91, 64, 16, 3, 2, (0, 1, 0, 1), 16, True),
    "conv7s2_118x120x3": (False, 118, 120, 3, 7, 2, (3, 3, 3, 3), 8, False),
    "conv3s2_150x100x3_wz": (False, 150, 100, 3, 3, 2, (0, 1, 0, 1), 8, True),
    "conv3s1_58x60x20": (False, 58, 60, 20, 3, 1, (1, 1, 1, 1), 12, False),
    "dw3s2_92x64x16": (True, 92, 64, 16, 3, 2, (0, 1, 0, 1), 16, False),
    "dw3s2_91x64x16": (True, 91, 64, 16, 3, 2, (0, 1, 0, 1), 16, False),
    # H = 86, not 85, for the same reason: 85 rows give OH = 42 = 3 x 14
    "dw3s2_86x56x24_wz": (True, 86, 56, 24, 3, 2, (0, 1, 0, 1), 24, True),
    "dw3s2_85x56x24_wz": (True, 85, 56, 24, 3, 2, (0, 1, 0, 1), 24, True),
    # top and left pads only, wider than the filter's own reach: no fill below or right of the image, two rows of it above
    "conv3s1_71x48x16_tl": (False, 71, 48, 16, 3, 1, (2, 0, 3, 0), 16, False),
    "dw3s1_71x48x16_tl": (True, 71, 48, 16, 3, 1, (2, 0, 3, 0), 16, False),
}
# SMALL: whole images per step, batch 5 like CASES (SMALL_BATCH names the exceptions)
SMALL = {
    "conv3s1_10x8x16_p3": (False, 10, 8, 16, 3, 1, (3, 3, 3, 3), 16, False),   # pads >= K: whole windows lie in fill
    "dw3s1_10x8x16_p3": (True, 10, 8, 16, 3, 1, (3, 3, 3, 3), 16, False),
    "conv3s1_9x9x3_p4": (False, 9, 9, 3, 3, 1, (4, 4, 4, 4), 8, False),
    "conv3s2_6x6x3_wz": (False, 6, 6, 3, 3, 2, (0, 1, 0, 1), 8, True),         # the filter-zero-point twins of three of CASES
    "conv3s2_8x8x16_wz": (False, 8, 8, 16, 3, 2, (0, 1, 0, 1), 32, True),
    "conv3s1_5x5x20_wz": (False, 5, 5, 20, 3, 1, (1, 1, 1, 1), 12, True),
    "conv3s2_5x5x3": (False, 5, 5, 3, 3, 2, (1, 1, 1, 1), 8, False),           # 75-byte images: every byte shift within one step
    "conv3s2_45x31x3": (False, 45, 31, 3, 3, 2, (0, 1, 0, 1), 8, False),       # 7 x 4185-byte images per step: every shift between steps
    "conv3s2_45x31x3_wz": (False, 45, 31, 3, 3, 2, (0, 1, 0, 1), 8, True),
    "conv3s1_7x8x64_n128": (False, 7, 8, 64, 3, 1, (1, 1, 1, 1), 128, False),  # conv_mm_rt's 1024-thread form
}
SMALL_BATCH = {"conv3s2_45x31x3": 23, "conv3s2_45x31x3_wz": 23}                # G = 7: four steps, the last one of two images

# name: (planner the group routes to -- op_create_padded_conv asks conv_rows, dw_mm, dw_gemm, conv_mm, conv_gemm in this order; dw_mm is
# conv_mm_plan_pads in its depthwise mode --, the plan fields pinned, whether the last band is ragged: OH % BH != 0)
PINNED = {
    "conv3s1_90x64x16": ("conv_mm", dict(BH=30, NBANDS=3, RB=32, G=1), False),
    "conv3s2_92x64x16_wz": ("conv_mm", dict(BH=16, NBANDS=3, G=1), True),
    "conv3s2_91x64x16_wz": ("conv_mm", dict(BH=15, NBANDS=3, G=1), False),
    "conv7s2_118x120x3": ("conv_gemm", dict(BH=30, NBANDS=2, padt=3, G=1), True),
    "conv3s2_150x100x3_wz": ("conv_gemm", dict(BH=38, NBANDS=2, G=1), True),
    "conv3s1_58x60x20": ("conv_gemm", dict(BH=29, NBANDS=2, G=1), False),
    "dw3s2_92x64x16": ("dw_mm", dict(BH=16, NBANDS=3, G=1), True),
    "dw3s2_91x64x16": ("dw_mm", dict(BH=15, NBANDS=3, G=1), False),
    "dw3s2_86x56x24_wz": ("dw_gemm", dict(BH=15, NBANDS=3, G=1), True),
    "dw3s2_85x56x24_wz": ("dw_gemm", dict(BH=14, NBANDS=3, G=1), False),
    "conv3s1_71x48x16_tl": ("conv_mm", dict(BH=36, NBANDS=2, padt=2, padl=3, G=1), True),
    "dw3s1_71x48x16_tl": ("dw_mm", dict(BH=36, NBANDS=2, padt=2, padl=3, G=1), True),
    "conv3s1_10x8x16_p3": ("conv_mm", dict(G=12, NBANDS=1, NTHR=256, padt=3, padl=3), False),
    "dw3s1_10x8x16_p3": ("dw_mm", dict(G=12, NBANDS=1, NTHR=256, padt=3, padl=3), False),
    "conv3s1_9x9x3_p4": ("conv_rows", dict(G=8, shy=4, XO=12), False),
    "conv3s2_6x6x3_wz": ("conv_rows", dict(G=8), False),
    "conv3s2_8x8x16_wz": ("conv_mm", dict(G=16, NBANDS=1, NTHR=256), False),
    "conv3s1_5x5x20_wz": ("conv_gemm", dict(G=16, NBANDS=1), False),
    "conv3s2_5x5x3": ("conv_rows", dict(G=8, shy=1, XO=4), False),
    "conv3s2_45x31x3": ("conv_rows", dict(G=7, shy=0, XO=0), False),
    "conv3s2_45x31x3_wz": ("conv_rows", dict(G=7, shy=0, XO=0), False),
    "conv3s1_7x8x64_n128": ("conv_mm", dict(G=10, NBANDS=1, NTHR=1024), False),
    "conv3s1_5x5x20": ("conv_gemm", dict(G=16, NBANDS=1), False),
    "dw3s2_8x8x24_wz": ("dw_gemm", dict(G=16, NBANDS=1), False),
}
BYTE_FORM = ("conv3s2_5x5x3", "conv3s2_45x31x3")    # conv_rows_bytes with C = 3: (H W C) % 4 != 0, images start at every byte shift

# MANY_STEPS: name -> (G, threads per workgroup, batch).  batch = G S + r with 0 < r < G: a ragged last step, and more steps S than
# twice the largest grid the launch code can choose -- the grid is 256 workgroups per CU times what the occupancy query answers,
# at most 2048 threads per CU / NTHR: 8 at 256 threads, 4 at 512 (conv_rows_*), 2 at 1024 -- so that every workgroup walks its step
# loop at least twice whatever the device says: S = 2 x 256 x (2048 / NTHR) + 1.  G and NTHR are the planners' (PINNED; NTHR of the
# kernels with one form: conv_rows_* 512, conv_gemm_rt, dw_gemm_rt and dw_mm_rt 256).  Input + output stay under 256 MiB.
def _many(G, nthr, r):
    assert 0 < r < G
    return G, nthr, G * (2 * 256 * (2048 // nthr) + 1) + r


MANY_STEPS = {
    "conv3s2_5x5x3": _many(8, 512, 3),             # 16 395 images
    "conv3s2_45x31x3": _many(7, 512, 2),           # 14 345 images, 98 MB
    "conv3s1_10x8x16_p3": _many(12, 256, 5),       # 49 169 images, 195 MB
    "dw3s1_10x8x16_p3": _many(12, 256, 5),
    "conv3s1_7x8x64_n128": _many(10, 1024, 3),     # 5 133 images
    "conv3s1_5x5x20": _many(16, 256, 7),           # 65 559 images
    "dw3s2_8x8x24_wz": _many(16, 256, 7),          # 65 559 images, 126 MB
}
EVERY = dict(CASES, **BANDED, **SMALL)


def out_hw(case):
    dw, H, W, C, K, S, (t, b, l, r), N, wz = case
    return (H + t + b - K) // S + 1, (W + l + r - K) // S + 1


def layers(case, rng, elem):
    """-> build_model's arguments for [PAD, the VALID convolution]"""
    import tflite_writer as tw
    dw, H, W, C, K, S, (t, b, l, r), N, wz = case
    lo, hi = (0, 256) if elem == tw.UINT8 else (-128, 128)
    in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, hi - 20)))
    pad = tw._pad_layer((H, W, C), in_q, ((t, b), (l, r)))
    conv = tw._conv_layer(rng, (H + t + b, W + l + r, C), in_q, dw, N, K, S, "valid", "relu6", elem, "all" if wz else "none")
    return (1, H, W, C), in_q, [pad, conv]


def row_image(in_shape, in_q, dt, first=0):
    """every row y one constant, (lo + 1 + first + y) mod the range of T with the input zero point skipped: neighbouring rows differ
    and no row looks like fill, so a band that reads its rows one off changes every output row, not only those at the edge"""
    lo, hi = (0, 256) if dt == np.uint8 else (-128, 128)
    H = in_shape[1]
    vals = [v for v in range(lo, hi) if v != in_q[1]]
    row = np.array([vals[(1 + first + y) % len(vals)] for y in range(H)]).astype(dt)
    return np.broadcast_to(row[:, None, None], tuple(in_shape[1:])).copy()


def images(rng, in_shape, in_q, dt, batch=5, rows=False):
    """batch 5: image 0 all-minimum, image 1 all-maximum, image 2 the zero point everywhere except its outermost rows and columns (a
    window placed one off changes bytes), the rest random.  rows: image 4 is row_image where the batch has one (a random one stays)"""
    x = _images(rng, in_shape, in_q, dt, batch)
    if rows and batch >= 5:
        x[4] = row_image(in_shape, in_q, dt)
    return x


def _images(rng, in_shape, in_q, dt, batch):
    lo, hi = (0, 256) if dt == np.uint8 else (-128, 128)
    x = rng.integers(lo, hi, (batch,) + tuple(in_shape[1:])).astype(dt)
    x[0], x[1] = lo, hi - 1
    edge = x[2].copy()
    edge[edge == in_q[1]] = lo if in_q[1] != lo else hi - 1
    x[2] = in_q[1]
    for sl in ((0, slice(None)), (-1, slice(None)), (slice(None), 0), (slice(None), -1)):
        x[2][sl] = edge[sl]
    return x
