"""RESIZE_NEAREST_NEIGHBOR's contract (include/microflow_amd.h: mf_resize_nearest_create) for the tests: out[oy][ox] = in[oy // sy][ox // sx],
no arithmetic.  compose() runs a tflite_writer layer list segment by segment (in the manner of pad_ref.segments): every run of reference
operators through the CPU oracle, with resize / max_pool_2d / concatenation in numpy between the segments."""
import numpy as np

from tests import concat_ref as K
from tests import maxpool_ref as R


def resize(x, sy, sx):
    """x: [..., H, W, C] -> [..., sy H, sx W, C]"""
    return np.repeat(np.repeat(np.asarray(x), sy, axis=-3), sx, axis=-2)


def compose(tw, O, in_shape, in_q, layers, elem, xq):
    """-> the model's output bytes [B, out_elems] for xq [B, H, W, C]"""
    t, shape, q, seg, outs = np.asarray(xq), tuple(in_shape), in_q, [], []

    def flush(t):
        if not seg:
            return t
        m = O.Model(tw.build_model(seg[0][0], seg[0][1], [L for _, _, L in seg], elem))
        del seg[1:], seg[:1]
        return np.stack([m.run_quantized(v.reshape(-1)).reshape(-1) for v in t])

    for L in layers:
        if L["op"] in ("resize_nearest_neighbor", "max_pool_2d", "concatenation"):
            t = flush(t).reshape((len(t),) + shape[1:])
            if L["op"] == "resize_nearest_neighbor":
                t = resize(t, L["out_shape"][1] // shape[1], L["out_shape"][2] // shape[2])
            elif L["op"] == "max_pool_2d":
                c0, c1 = R.pool_constants(q[0], q[1], L["out_q"][0], L["out_q"][1])
                t = R.max_pool_2d(t, L["filter"], L["strides"], L["padding"], L["out_shape"][1:3], c0, c1, L.get("act"), L["out_q"][0], L["out_q"][1])
            else:
                skip, q_skip = outs[L["skip"]]
                t = K.concat(t, skip, q, q_skip, L["out_q"])
        else:
            seg.append((shape, q, L))
        shape, q = tuple(L["out_shape"]), L.get("out_q") or q
        outs.append((None, q))
        if any(M["op"] == "concatenation" and M["skip"] == len(outs) - 1 for M in layers):
            t = flush(t).reshape((len(t),) + shape[1:])   # (a skip source: its tensor is needed by itself)
            outs[-1] = (t, q)
    return flush(t).reshape(len(xq), -1)
