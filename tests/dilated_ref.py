"""conv_2d and depthwise_conv_2d with dilation factors: the contract (include/microflow_amd.h) restated in numpy -- the
reference never reads the factors.  A gather over the taps with explicit bounds tests, an int64 accumulator, tests/tconv_ref's epilogue.

    tap (ky, kx) of output (oy, ox) reads x[oy sh - padt + ky dh][ox sw - padl + kx dw]; outside the image it contributes 0
    SAME: padt = ((KH - 1) dh) / 2, OH = ceil(H / sh); VALID: padt = 0, OH = ceil((H - (KH - 1) dh) / sh); the same in W"""
import numpy as np

from tests import tconv_ref as T


def geometry(H, W, KH, KW, strides, dilation, same):
    (sh, sw), (dh, dw) = strides, dilation   # -> (OH, OW, padt, padl)
    keh, kew = (KH - 1) * dh + 1, (KW - 1) * dw + 1
    if same:
        return -(-H // sh), -(-W // sw), (keh - 1) // 2, (kew - 1) // 2
    return -(-(H - keh + 1) // sh), -(-(W - kew + 1) // sw), 0, 0


def mean_taps(H, W, KH, KW, strides, dilation, same):
    """taps inside the image, averaged over the output pixels (a halo tap contributes exactly 0 to the accumulator)"""
    (sh, sw), (dh, dw), (OH, OW, padt, padl) = strides, dilation, geometry(H, W, KH, KW, strides, dilation, same)
    rows = sum(0 <= oy * sh - padt + ky * dh < H for oy in range(OH) for ky in range(KH)) / OH
    cols = sum(0 <= ox * sw - padl + kx * dw < W for ox in range(OW) for kx in range(KW)) / OW
    return rows * cols


def accumulators(x, w, izp, wzp, strides, dilation, same, depthwise=False):
    """x: [B, H, W, C]; w: [N, KH, KW, C], or depthwise [KH, KW, N] (output n reads channel n, channel 0 where C == 1); real values of
    T; wzp: [N] or [1] -> int64 [B, OH, OW, N]"""
    x, w = np.asarray(x), np.asarray(w)
    B, H, W, C = x.shape
    KH, KW = w.shape[:2] if depthwise else w.shape[1:3]
    N = w.shape[2] if depthwise else w.shape[0]
    (sh, sw), (dh, dw) = strides, dilation
    OH, OW, padt, padl = geometry(H, W, KH, KW, strides, dilation, same)
    z = np.broadcast_to(np.asarray(wzp, np.int64).reshape(-1), (N,))
    xs = x.astype(np.int64) - int(izp)
    acc = np.zeros((B, OH, OW, N), np.int64)
    for oy in range(OH):
        for ox in range(OW):
            for ky in range(KH):
                for kx in range(KW):
                    iy, ix = oy * sh - padt + ky * dh, ox * sw - padl + kx * dw
                    if not (0 <= iy < H and 0 <= ix < W):
                        continue
                    if depthwise:
                        v = xs[:, iy, ix, :] if C == N else xs[:, iy, ix, :1]
                        acc[:, oy, ox, :] += v * (w[ky, kx, :].astype(np.int64) - z)
                    else:
                        acc[:, oy, ox, :] += xs[:, iy, ix, :] @ (w[:, ky, kx, :].astype(np.int64) - z[:, None]).T
    return acc


def conv(x, w, izp, wzp, strides, dilation, same, c0, c1, ozp, oscale, act=None, depthwise=False):
    return T.epilogue(accumulators(x, w, izp, wzp, strides, dilation, same, depthwise), c0, c1, ozp, oscale, act, np.asarray(x).dtype)


def twin(layers):
    """tflite_writer layer dicts, every dilated layer as the undilated one with the KeH x KeW filter whose added taps hold the filter
    zero point ((w - wzp) is 0 there: the contract's accumulator), which the CPU oracle can run"""
    out = []
    for L in layers:
        if "dilation" in L:
            L, (dh, dw), key = dict(L), L["dilation"], "filters" if "filters" in L else "weights"
            f = np.asarray(L[key])
            g = np.empty((f.shape[0], (f.shape[1] - 1) * dh + 1, (f.shape[2] - 1) * dw + 1, f.shape[3]), f.dtype)
            g[:] = np.asarray(L["fzp"]).reshape((-1, 1, 1, 1) if key == "filters" else (1, 1, 1, -1))
            g[:, ::dh, ::dw, :] = f
            L.update({key: g, "dilation": (1, 1)})
        out.append(L)
    return out
