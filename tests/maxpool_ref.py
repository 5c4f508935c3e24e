"""MaxPool2D's arithmetic contract (include/microflow_amd.h) restated in numpy for the tests: the reference has no
such operator, so the CPU oracle cannot say what it gives.  Every f32 step is an np.float32 operation in the stated order (numpy
rounds each ufunc on its own: no fma), roundf is half away from zero, `as T` saturates and sends NaN to 0.

Whole models are checked segment by segment (segments): each run of reference operators between two max pools is written as a
model of its own from the same layer dicts and run through the oracle, with max_pool_2d between the segments."""
import numpy as np

F = np.float32


def roundf(y):
    """roundf of f32 values, half away from zero (|y| + 0.5 is exact in f64 for every finite f32 below 2^52)"""
    y = np.asarray(y, F)
    return np.copysign(np.floor(np.abs(y.astype(np.float64)) + 0.5), y).astype(F)


def saturate(r, dt):
    """Rust's `as T` on f32: NaN -> 0, the rest clamped to T's range"""
    lo, hi = (0, 255) if np.dtype(dt) == np.uint8 else (-128, 127)
    r = np.asarray(r, F)
    return np.clip(np.where(np.isnan(r), F(0), r), lo, hi).astype(np.int32)


def pool_constants(in_scale, in_zp, out_scale, out_zp):
    """microflow-macros/src/ops/average_pool_2d.rs:77-83: (in.scale / out.scale, f32(ozp) - (in.scale * f32(izp)) / out.scale)"""
    s_i, s_o = F(in_scale), F(out_scale)
    c0 = F(s_i / s_o)
    prod = F(s_i * F(in_zp))
    return c0, F(F(out_zp) - F(prod / s_o))


def quantize_scalar(x, scale, zp, dt):
    """src/quantize.rs:16-18"""
    return int(saturate(roundf(F(F(x) / F(scale)) + F(zp)), dt))


def activation(q, act, out_scale, out_zp, dt):
    """src/activation.rs: relu = max(x, zp); relu6 = min(relu(x), quantize(6.0))"""
    if act in (None, "none", 0):
        return q
    q = np.maximum(q, int(out_zp))
    if act in ("relu6", 3):
        q = np.minimum(q, quantize_scalar(6.0, out_scale, out_zp, dt))
    return q


def windows(size, k, stride, same, out):
    """per output index the in-bounds taps of the window along one axis, placed as Tensor4D::view places it"""
    shift = (k - 1) // 2 if same else 0
    res = []
    for o in range(out):
        taps = [i for i in range(o * stride - shift, o * stride - shift + k) if 0 <= i < size]
        if not taps:
            raise ValueError("window %d has no in-bounds tap" % o)
        res.append((taps[0], taps[-1] + 1))
    return res


def max_pool_2d(x, filt, strides, padding, out_hw, c0, c1, act, out_scale, out_zp):
    """x: [B, H, W, C] of int8 / uint8 (real values of T) -> [B, OH, OW, C] of the same type"""
    x = np.asarray(x)
    dt = x.dtype
    assert dt in (np.int8, np.uint8) and x.ndim == 4
    B, H, W, C = x.shape
    same = padding in ("same", 0)
    rows = windows(H, filt[0], strides[0], same, out_hw[0])
    cols = windows(W, filt[1], strides[1], same, out_hw[1])
    m = np.empty((B, out_hw[0], out_hw[1], C), np.int32)
    xi = x.astype(np.int32)
    for oy, (y0, y1) in enumerate(rows):
        for ox, (x0, x1) in enumerate(cols):
            m[:, oy, ox, :] = xi[:, y0:y1, x0:x1, :].max(axis=(1, 2))      # the in-bounds taps only
    y = F(c0) * m.astype(F)                                                 # c0 * f32(m) ...
    y = y + F(c1)                                                           # ... + c1, each rounded to f32
    q = saturate(roundf(y), dt)
    return activation(q, act, out_scale, out_zp, dt).astype(dt)


def segments(tw, O, in_shape, in_q, layers, elem):
    """-> run(xq [B, in_elems]) giving the list of every operator's output [B, out_elems] (the expected tensors of run_until)"""
    parts, cur, shape, q = [], [], tuple(in_shape), in_q
    for L in layers:
        if L["op"] == "max_pool_2d":
            if cur:
                parts.append(("model", O.Model(tw.build_model(cur[0], cur[1], cur[2], elem)), len(cur[2])))
                cur = []
            parts.append(("max", (L, shape, q), 1))
        else:
            if not cur:
                cur = [shape, q, []]
            cur[2].append(L)
        shape, q = tuple(L["out_shape"]), L.get("out_q") or q
    if cur:
        parts.append(("model", O.Model(tw.build_model(cur[0], cur[1], cur[2], elem)), len(cur[2])))

    def run(xq):
        xq = np.asarray(xq)
        outs, t = [], xq.reshape(len(xq), -1)
        for kind, what, _ in parts:
            if kind == "model":
                per = [what.run_quantized(v, layers=True)[1] for v in t]
                for i in range(len(per[0])):
                    outs.append(np.stack([p[i].reshape(-1) for p in per]))
            else:
                L, shp, qi = what
                c0, c1 = pool_constants(qi[0], qi[1], L["out_q"][0], L["out_q"][1])
                y = max_pool_2d(t.reshape((len(t),) + tuple(shp[1:])), L["filter"], L["strides"], L["padding"], L["out_shape"][1:3], c0, c1,
                                L.get("act"), L["out_q"][0], L["out_q"][1])
                outs.append(y.reshape(len(t), -1))
            t = outs[-1]
        return outs
    return run
