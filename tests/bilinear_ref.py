"""RESIZE_BILINEAR's contract (include/microflow_amd.h: mf_resize_bilinear_create) in numpy int64, for the tests."""
import numpy as np


def _axis(n, s):
    """-> (i0, i1, w0, w1) per output index of an axis of n inputs at factor s: the clamped taps and their weights (w0 + w1 = 2 s)"""
    o = np.arange(n * s)
    q, k = o // s, 2 * (o % s) + 1 - s
    i0, f = np.where(k >= 0, q, q - 1), np.where(k >= 0, k, 2 * s + k)
    return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), 2 * s - f, f


def accumulate(x, sy, sx):
    """x: [..., H, W, C] i8 or u8 -> the exact sums [..., sy H, sx W, C] (int64) of the four weighted taps, on the value as x's type"""
    v = np.asarray(x).astype(np.int64)
    y0, y1, a0, a1 = _axis(v.shape[-3], sy)
    x0, x1, b0, b1 = _axis(v.shape[-2], sx)
    a0, a1, b0, b1 = a0[:, None, None], a1[:, None, None], b0[:, None], b1[:, None]
    rows = a0 * v[..., y0, :, :] + a1 * v[..., y1, :, :]
    return b0 * rows[..., x0, :] + b1 * rows[..., x1, :]


def resize_bilinear(x, sy, sx):
    """x: [..., H, W, C] i8 or u8 -> [..., sy H, sx W, C]: one rounding of the exact sum, half away from zero"""
    acc, dd = accumulate(x, sy, sx), 4 * sy * sx
    return (np.sign(acc) * ((np.abs(acc) + dd // 2) // dd)).astype(np.asarray(x).dtype)
