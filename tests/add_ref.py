"""ADD's arithmetic contract (include/microflow_amd.h) restated in numpy for the tests: the reference has no such
operator, so the CPU oracle cannot say what it gives.  Every f32 step is an np.float32 operation in the stated order (numpy rounds
each ufunc on its own: no fma); roundf, `as T` and the fused activation are tests/maxpool_ref's.

    ca = sa / so, cb = sb / so
    ta = ca * f32(a - za), tb = cb * f32(b - zb), y = T::from(roundf((f32(zo) + ta) + tb)), then the activation

Whole residual models are checked segment by segment (segments): each run of reference operators is written as a model of its own
from the same layer dicts and run through the oracle -- which knows no ADD -- with the restatements of ADD and MaxPool2D between
the segments and the saved skip tensor carried across."""
import numpy as np

from tests import maxpool_ref as R

F = np.float32


def constants(sa, sb, so):
    """(ca, cb): two f32 divisions"""
    return F(F(sa) / F(so)), F(F(sb) / F(so))


def add(a, b, a_q, b_q, out_q, act=None, consts=None):
    """a, b: arrays of one shape and one type (int8 / uint8, real values of T); *_q = (scale, zero point) -> the same shape and type"""
    a, b = np.asarray(a), np.asarray(b)
    dt = a.dtype
    assert dt in (np.int8, np.uint8) and b.dtype == dt and a.shape == b.shape
    ca, cb = constants(a_q[0], b_q[0], out_q[0]) if consts is None else (F(consts[0]), F(consts[1]))
    ta = ca * (a.astype(np.int32) - int(a_q[1])).astype(F)          # the subtraction in i32, the conversion exact
    tb = cb * (b.astype(np.int32) - int(b_q[1])).astype(F)
    with np.errstate(over="ignore", invalid="ignore"):
        y = (F(out_q[1]) + ta) + tb                                  # each + rounded to f32, in this order
    q = R.saturate(R.roundf(y), dt)
    return R.activation(q, act, out_q[0], out_q[1], dt).astype(dt)


def segments(tw, O, in_shape, in_q, layers, elem):
    """-> run(xq [B, in_elems]) giving the list of every operator's output [B, out_elems] (the expected tensors of run_until)"""
    parts, cur, shape, q = [], [], tuple(in_shape), in_q
    quants = []  # every layer's output quantisation

    def flush():
        nonlocal cur
        if cur:
            parts.append(("model", O.Model(tw.build_model(cur[0], cur[1], cur[2], elem)), len(cur[2])))
            cur = []

    for L in layers:
        if L["op"] == "max_pool_2d":
            flush()
            parts.append(("max", (L, shape, q), 1))
        elif L["op"] == "add":
            flush()
            q_skip = in_q if L["skip"] < 0 else quants[L["skip"]]
            parts.append(("add", (L, q, q_skip), 1))
        else:
            if not cur:
                cur = [shape, q, []]
            cur[2].append(L)
        shape, q = tuple(L["out_shape"]), L.get("out_q") or q
        quants.append(q)
    flush()

    def run(xq):
        xq = np.asarray(xq)
        outs, t = [], xq.reshape(len(xq), -1)
        for kind, what, _ in parts:
            if kind == "model":
                per = [what.run_quantized(v, layers=True)[1] for v in t]
                for i in range(len(per[0])):
                    outs.append(np.stack([p[i].reshape(-1) for p in per]))
            elif kind == "max":
                L, shp, qi = what
                c0, c1 = R.pool_constants(qi[0], qi[1], L["out_q"][0], L["out_q"][1])
                y = R.max_pool_2d(t.reshape((len(t),) + tuple(shp[1:])), L["filter"], L["strides"], L["padding"], L["out_shape"][1:3], c0, c1,
                                  L.get("act"), L["out_q"][0], L["out_q"][1])
                outs.append(y.reshape(len(t), -1))
            else:
                L, q_run, q_skip = what
                skip = xq.reshape(len(xq), -1) if L["skip"] < 0 else outs[L["skip"]]
                if L.get("swap"):
                    y = add(skip, t, q_skip, q_run, L["out_q"], L.get("act"))
                else:
                    y = add(t, skip, q_run, q_skip, L["out_q"], L.get("act"))
                outs.append(y.reshape(len(t), -1))
            t = outs[-1]
        return outs
    return run
