"""PAD's and MEAN's contracts (include/microflow_amd.h) for the tests.  The reference has neither operator:

PAD is np.pad with the tensor's zero point (pad): no arithmetic, the quantisation stays.
MEAN over the axes {1, 2} IS the reference's average_pool_2d over the whole image (mean_as_pool: the layer dicts of that pool, + a
Reshape for keep_dims = False), so the CPU oracle computes it.

Whole models are checked segment by segment (segments, in the manner of maxpool_ref / add_ref): every run of reference operators
between two operators the oracle does not have is written as a model of its own from the same layer dicts and run through the
oracle, with pad / max_pool_2d / add between the segments."""
import numpy as np

from tests import add_ref as A
from tests import maxpool_ref as R


def pad(x, pads, zero_point):
    """x: [B, H, W, C] of int8 / uint8 (real values of T); pads ((top, bottom), (left, right)) -> [B, H + t + b, W + l + r, C]"""
    x = np.asarray(x)
    assert x.dtype in (np.int8, np.uint8) and x.ndim == 4
    (t, b), (l, r) = pads
    return np.pad(x, ((0, 0), (t, b), (l, r), (0, 0)), mode="constant", constant_values=x.dtype.type(zero_point))


def mean_as_pool(L, in_shape):
    """the layers a `mean` layer stands for: AveragePool2D with the whole image as filter (VALID, stride 1, no activation) on the
    layer's own output quantisation, and for keep_dims = False the Reshape to [1, C]"""
    _, H, W, C = in_shape
    out = [dict(op="average_pool_2d", filter=(H, W), padding="valid", strides=(1, 1), act="none", out_shape=(1, 1, 1, C), out_q=L["out_q"])]
    if not L.get("keep_dims", False):
        out.append(dict(op="reshape", out_shape=(1, C), out_q=L["out_q"]))
    return out


def twin_layers(layers, in_shape):
    """the same model with every `mean` written as AveragePool2D (+ Reshape): what a MEAN model must route like"""
    res, shape = [], tuple(in_shape)
    for L in layers:
        res += mean_as_pool(L, shape) if L["op"] == "mean" else [L]
        shape = tuple(L["out_shape"])
    return res


def segments(tw, O, in_shape, in_q, layers, elem):
    """-> run(xq [B, in_elems]) giving the list of every operator's output [B, out_elems] (the expected tensors of run_until)"""
    parts, cur, shape, q = [], [], tuple(in_shape), in_q
    quants = []  # every layer's output quantisation

    def flush():
        nonlocal cur
        if cur:
            parts.append(("model", O.Model(tw.build_model(cur[0], cur[1], cur[2], elem)), cur[3]))
            cur = []

    for L in layers:
        if L["op"] in ("max_pool_2d", "add", "pad"):
            flush()
            if L["op"] == "add":
                parts.append(("add", (L, q, in_q if L["skip"] < 0 else quants[L["skip"]]), None))
            else:
                parts.append((L["op"], (L, shape, q), None))
        else:
            if not cur:
                cur = [shape, q, [], []]  # (..., the oracle's layers, which of them are operators of the model under test)
            if L["op"] == "mean":
                sub = mean_as_pool(L, shape)
                cur[2] += sub
                cur[3] += [False] * (len(sub) - 1) + [True]  # (the Reshape's tensor is the MEAN's: the same bytes)
            else:
                cur[2].append(L)
                cur[3].append(True)
        shape, q = tuple(L["out_shape"]), L.get("out_q") or q
        quants.append(q)
    flush()

    def run(xq):
        xq = np.asarray(xq)
        outs, t = [], xq.reshape(len(xq), -1)
        for kind, what, keep in parts:
            if kind == "model":
                per = [what.run_quantized(v, layers=True)[1] for v in t]
                for i in range(len(per[0])):
                    if keep[i]:
                        outs.append(np.stack([p[i].reshape(-1) for p in per]))
            elif kind == "pad":
                L, shp, qi = what
                outs.append(pad(t.reshape((len(t),) + tuple(shp[1:])), L["pads"], qi[1]).reshape(len(t), -1))
            elif kind == "max_pool_2d":
                L, shp, qi = what
                c0, c1 = R.pool_constants(qi[0], qi[1], L["out_q"][0], L["out_q"][1])
                y = R.max_pool_2d(t.reshape((len(t),) + tuple(shp[1:])), L["filter"], L["strides"], L["padding"], L["out_shape"][1:3], c0, c1,
                                  L.get("act"), L["out_q"][0], L["out_q"][1])
                outs.append(y.reshape(len(t), -1))
            else:
                L, q_run, q_skip = what
                skip = xq.reshape(len(xq), -1) if L["skip"] < 0 else outs[L["skip"]]
                y = A.add(skip, t, q_skip, q_run, L["out_q"], L.get("act")) if L.get("swap") else A.add(t, skip, q_run, q_skip, L["out_q"], L.get("act"))
                outs.append(y.reshape(len(t), -1))
            t = outs[-1]
        return outs
    return run
