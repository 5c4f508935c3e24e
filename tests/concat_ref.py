"""CONCATENATION's contract (include/microflow_amd.h) restated in numpy for the tests: the reference has no such
operator, so the CPU oracle cannot say what it gives.  Every f32 step is an np.float32 operation in the stated order (numpy rounds
each ufunc on its own: no fma); roundf and `as T` are tests/maxpool_ref's.

    ca = sa / so, cb = sb / so
    per element x of input i:  y = T::from(roundf(f32(zo) + c_i * f32(x - z_i)))
    output row r = row r of a (Ca elements) followed by row r of b (Cb elements)

Whole models with CONCATENATION joins (fire modules, identity skips) are checked as tests/shortcut_ref.segments checks projection
shortcuts: every run of reference operators on the main chain goes through the CPU oracle as a model of its own, the side Conv2D is a
one-layer oracle model fed with the saved tensor it reads, MaxPool2D and ADD are their own restatements, and the join is `concat`
below.  The oracle knows neither joins nor graphs, so nothing here comes from the code under test."""
import numpy as np

from tests import add_ref as A
from tests import maxpool_ref as R

F = np.float32
JOINS = ("add", "concatenation")


def constants(sa, sb, so):
    """(ca, cb): two f32 divisions"""
    return F(F(sa) / F(so)), F(F(sb) / F(so))


def requant(x, c, z, out_q):
    """one input's elements: x an int8 / uint8 array (real values of T), c its constant, z its zero point -> int32 values of T"""
    x = np.asarray(x)
    d = (x.astype(np.int32) - int(z)).astype(F)                      # the subtraction in i32, the conversion exact
    with np.errstate(over="ignore", invalid="ignore"):
        t = F(c) * d                                                 # one multiplication ...
        y = F(out_q[1]) + t                                          # ... one addition, each rounded to f32
    return R.saturate(R.roundf(y), x.dtype)


def concat(a, b, a_q, b_q, out_q, consts=None):
    """a [..., Ca], b [..., Cb] of one type (int8 / uint8, real values of T) and equal leading axes; *_q = (scale, zero point)
    -> [..., Ca + Cb] of the same type"""
    a, b = np.asarray(a), np.asarray(b)
    dt = a.dtype
    assert dt in (np.int8, np.uint8) and b.dtype == dt and a.shape[:-1] == b.shape[:-1]
    ca, cb = constants(a_q[0], b_q[0], out_q[0]) if consts is None else (F(consts[0]), F(consts[1]))
    return np.concatenate([requant(a, ca, a_q[1], out_q), requant(b, cb, b_q[1], out_q)], axis=-1).astype(dt)


def requant_scalar(x, c, z, zo, u8):
    """the same element a second time, with Python scalars and struct-rounded f32 steps (tests/test_concat_host.py checks `requant`
    against it on all 256 bytes)"""
    import math
    import struct

    def f32(v):
        return struct.unpack("<f", struct.pack("<f", v))[0]
    d = f32(float(int(x) - int(z)))
    t = f32(f32(c) * d)            # (the product of two f32 values is exact in f64: one rounding)
    y = f32(f32(float(zo)) + t)
    r = math.copysign(math.floor(abs(y) + 0.5), y)
    lo, hi = (0, 255) if u8 else (-128, 127)
    return int(min(max(r, lo), hi))


def _strip(L):
    return {k: v for k, v in L.items() if k != "side_of"}


def segments(tw, O, in_shape, in_q, layers, elem):
    """-> run(xq [B, in_elems]) giving the list of every operator's output [B, out_elems] in FILE order.  The layer dicts are
    tools/tflite_writer.py's: a conv_2d with side_of = k reads layer k's output (-1: the model input) and does not move the running
    tensor; a join (add, concatenation) names its second operand by `skip` and its operand order by `swap`"""
    shape_of, q_of = {-1: tuple(in_shape)}, {-1: in_q}
    run_shape, run_q = tuple(in_shape), in_q
    before = []
    for i, L in enumerate(layers):
        before.append((run_shape, run_q))
        if "side_of" in L:
            shape_of[i], q_of[i] = tuple(L["out_shape"]), L["out_q"]
            continue
        run_shape, run_q = tuple(L["out_shape"]), L.get("out_q") or run_q
        shape_of[i], q_of[i] = run_shape, run_q
    models = {}

    def model(key, shape, q, ls):
        if key not in models:
            models[key] = O.Model(tw.build_model(shape, q, [_strip(L) for L in ls], elem))
        return models[key]

    def through(m, t):
        per = [m.run_quantized(v, layers=True)[1] for v in t]
        return [np.stack([p[i].reshape(-1) for p in per]) for i in range(len(per[0]))]

    def side(k, outs):
        src = layers[k]["side_of"]
        return through(model(("side", k), shape_of[src], q_of[src], [layers[k]]), outs[src])[0]

    def run(xq):
        xq = np.asarray(xq)
        n = len(xq)
        outs = {-1: xq.reshape(n, -1)}
        cur, i = -1, 0          # cur: the layer whose output is the running tensor
        while i < len(layers):
            L = layers[i]
            if "side_of" in L:
                outs[i] = side(i, outs)
                i += 1
            elif L["op"] in JOINS:
                s = L["skip"]
                q_run, q_skip = before[i][1], q_of[s]
                t, skip = outs[cur], outs[s]
                if L["op"] == "add":
                    y = A.add(skip, t, q_skip, q_run, L["out_q"], L.get("act")) if L.get("swap") else A.add(t, skip, q_run, q_skip, L["out_q"], L.get("act"))
                else:  # rows of channels: [B, rows, C]
                    t = t.reshape(n, -1, before[i][0][-1])
                    skip = skip.reshape(n, -1, shape_of[s][-1])
                    y = concat(skip, t, q_skip, q_run, L["out_q"]) if L.get("swap") else concat(t, skip, q_run, q_skip, L["out_q"])
                outs[i] = y.reshape(n, -1)
                cur, i = i, i + 1
            elif L["op"] == "max_pool_2d":
                shp, qi = before[i]
                c0, c1 = R.pool_constants(qi[0], qi[1], L["out_q"][0], L["out_q"][1])
                y = R.max_pool_2d(outs[cur].reshape((n,) + tuple(shp[1:])), L["filter"], L["strides"], L["padding"], L["out_shape"][1:3], c0, c1,
                                  L.get("act"), L["out_q"][0], L["out_q"][1])
                outs[i] = y.reshape(n, -1)
                cur, i = i, i + 1
            else:  # a run of reference operators on the main chain, up to the next join / max pool (side operators stepped over)
                idx, j = [], i
                while j < len(layers) and layers[j]["op"] not in JOINS + ("max_pool_2d",):
                    if "side_of" not in layers[j]:
                        idx.append(j)
                    j += 1
                got = through(model(("run", i), before[i][0], before[i][1], [layers[k] for k in idx]), outs[cur])
                for k, t in zip(idx, got):
                    outs[k] = t
                cur = idx[-1]
                for k in range(i, j):  # the side operators inside the run, now that every tensor in front of them exists
                    if "side_of" in layers[k]:
                        outs[k] = side(k, outs)
                i = j
        return [outs[k] for k in range(len(layers))]
    return run
