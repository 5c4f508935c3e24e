"""Expected tensors of models with a side operator -- one Conv2D on a skip edge, read by one ADD (a ResNet projection shortcut) --
built as tests/add_ref.segments builds them for identity skips: every run of reference operators on the main chain goes through the
CPU oracle as a model of its own, the side Conv2D is a one-layer oracle model fed with the saved tensor it reads, and the ADD is
tests/add_ref.add.  The oracle knows neither ADD nor graphs, so nothing here comes from the code under test.

    run = segments(tw, O, in_shape, in_q, layers, elem);  outs = run(xq)     # every operator's output, in FILE order

The layer dicts are tools/tflite_writer.py's: a conv_2d with side_of = k reads layer k's output (-1: the model input) and does not move
the running tensor; the add that names it as its skip reads its output beside the running tensor."""
import numpy as np

from tests import add_ref as A
from tests import maxpool_ref as R


def _strip(L):
    return {k: v for k, v in L.items() if k != "side_of"}


def segments(tw, O, in_shape, in_q, layers, elem):
    """-> run(xq [B, in_elems]) giving the list of every operator's output [B, out_elems] in file order"""
    # the running tensor's shape and quantisation in front of every layer, and every layer's output shape and quantisation
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

    def run(xq):
        xq = np.asarray(xq)
        n = len(xq)
        outs = {-1: xq.reshape(n, -1)}
        cur, i = -1, 0          # cur: the layer whose output is the running tensor
        while i < len(layers):
            L = layers[i]
            if "side_of" in L:
                src = L["side_of"]
                outs[i] = through(model(("side", i), shape_of[src], q_of[src], [L]), outs[src])[0]
                i += 1
            elif L["op"] == "add":
                skip = outs[L["skip"]]
                q_run, q_skip = before[i][1], q_of[L["skip"]]
                t = outs[cur]
                y = A.add(skip, t, q_skip, q_run, L["out_q"], L.get("act")) if L.get("swap") else A.add(t, skip, q_run, q_skip, L["out_q"], L.get("act"))
                outs[i] = y.reshape(n, -1)
                cur, i = i, i + 1
            elif L["op"] == "max_pool_2d":
                shp, qi = before[i]
                c0, c1 = R.pool_constants(qi[0], qi[1], L["out_q"][0], L["out_q"][1])
                y = R.max_pool_2d(outs[cur].reshape((n,) + tuple(shp[1:])), L["filter"], L["strides"], L["padding"], L["out_shape"][1:3], c0, c1,
                                  L.get("act"), L["out_q"][0], L["out_q"][1])
                outs[i] = y.reshape(n, -1)
                cur, i = i, i + 1
            else:  # a run of reference operators on the main chain, up to the next add / max pool (side operators stepped over)
                idx, j = [], i
                while j < len(layers) and layers[j]["op"] not in ("add", "max_pool_2d"):
                    if "side_of" not in layers[j]:
                        idx.append(j)
                    j += 1
                got = through(model(("run", i), before[i][0], before[i][1], [layers[k] for k in idx]), outs[cur])
                for k, t in zip(idx, got):
                    outs[k] = t
                cur = idx[-1]
                # the side operators inside the run, now that every tensor in front of them exists
                for k in range(i, j):
                    if "side_of" in layers[k]:
                        src = layers[k]["side_of"]
                        outs[k] = through(model(("side", k), shape_of[src], q_of[src], [layers[k]]), outs[src])[0]
                i = j
        return [outs[k] for k in range(len(layers))]
    return run
