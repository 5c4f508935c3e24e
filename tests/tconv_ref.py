"""TRANSPOSE_CONV's contract (include/microflow_amd.h: mf_transpose_conv_create) restated in numpy for the tests:
the reference has no such operator, so the CPU oracle cannot say what it gives.  No phases here: every input pixel is scattered
through every tap.  The accumulator is int64; every f32 step of the epilogue is an np.float32 operation in the stated order (numpy
rounds each ufunc on its own: no fma); roundf, `as T` and the fused activation are tests/maxpool_ref's.

    acc[oy][ox][n] = sum (x[iy][ix][c] - izp) (w[n][ky][kx][c] - wzp[n or 0])   over iy sh + ky - padt == oy, ix sw + kx - padl == ox
    y = T::from(roundf((f32(ozp) + c0[n]) + c1[n or 0] * f32(acc))), then the activation"""
import numpy as np

from tests import maxpool_ref as R

F = np.float32


def out_hw(H, W, KH, KW, sh, sw, same):
    """the usual output size of each padding (SAME admits any OH with ceil(OH / sh) == H; this is the largest)"""
    return (H * sh, W * sw) if same else ((H - 1) * sh + KH, (W - 1) * sw + KW)


def pads(H, W, KH, KW, sh, sw, OH, OW):
    """TFLite's placement: (padt, padl)"""
    return max(0, (H - 1) * sh + KH - OH) // 2, max(0, (W - 1) * sw + KW - OW) // 2


def accumulators(x, w, izp, wzp, strides, out_hw_):
    """x: [B, H, W, C], w: [N, KH, KW, C] (real values of T), wzp: [N] or [1] -> int64 [B, OH, OW, N]"""
    x, w = np.asarray(x), np.asarray(w)
    B, H, W, C = x.shape
    N, KH, KW, _ = w.shape
    (sh, sw), (OH, OW) = strides, out_hw_
    padt, padl = pads(H, W, KH, KW, sh, sw, OH, OW)
    z = np.broadcast_to(np.asarray(wzp, np.int64).reshape(-1), (N,)) if np.size(wzp) in (1, N) else None
    xs = x.astype(np.int64) - int(izp)
    ws = w.astype(np.int64) - z[:, None, None, None]
    acc = np.zeros((B, OH, OW, N), np.int64)
    for iy in range(H):
        for ky in range(KH):
            oy = iy * sh + ky - padt
            if not 0 <= oy < OH:
                continue
            for ix in range(W):
                for kx in range(KW):
                    ox = ix * sw + kx - padl
                    if 0 <= ox < OW:
                        acc[:, oy, ox, :] += xs[:, iy, ix, :] @ ws[:, ky, kx, :].T
    return acc


def epilogue(acc, c0, c1, ozp, oscale, act, dt):
    N = acc.shape[-1]
    c0 = np.asarray(c0, F).reshape(-1)
    c1 = np.broadcast_to(np.asarray(c1, F).reshape(-1), (N,)) if np.size(c1) in (1, N) else None
    A = F(ozp) + c0                                   # f32(ozp) + c0[n], rounded once
    with np.errstate(over="ignore", invalid="ignore"):
        y = A + c1 * acc.astype(F)                    # the product rounded, then the sum
    q = R.saturate(R.roundf(y), dt)
    return R.activation(q, act, oscale, ozp, dt).astype(dt)


def transpose_conv(x, w, izp, wzp, strides, out_hw_, c0, c1, ozp, oscale, act=None):
    """-> [B, OH, OW, N] of x's type"""
    return epilogue(accumulators(x, w, izp, wzp, strides, out_hw_), c0, c1, ozp, oscale, act, np.asarray(x).dtype)
