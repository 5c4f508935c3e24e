"""One reference interpreter for every model the loader takes: chains of tools/tflite_writer.py's layer dicts with skip edges.

    run = interpret(tw, O, in_shape, in_q, layers, elem);  outs = run(xq)     # every operator's output [B, out_elems], in FILE order

It combines what the family tests already have and adds no arithmetic of its own:
  - every run of reference operators on the main chain goes through the CPU oracle as a model of its own (as the `segments` functions
    of maxpool_ref / add_ref / pad_ref / concat_ref / shortcut_ref do), dilated and grouped convolutions as their undilated / dense
    twins (dilated_ref.twin, grouped_ref.twin) and MEAN as the whole-image AveragePool2D it is (pad_ref.twin_layers);
  - a side Conv2D (side_of = k: it reads layer k's output, -1 the model input, and does not move the running tensor) is a one-layer
    oracle model fed with the saved tensor it reads;
  - max_pool_2d, add, pad, concatenation, transpose_conv and resize_nearest_neighbor are the numpy restatements of their contracts
    (maxpool_ref.max_pool_2d, add_ref.add, pad_ref.pad, concat_ref.concat, tconv_ref.transpose_conv, resize_ref.resize); TRANSPOSE_CONV's
    two constants are written as tests/test_gpu_tconv.py's composed autoencoder writes them.
A join names its second operand by `skip` (a layer, a side operator among them, or -1) and its operand order by `swap`; a skip source
behind Reshapes is the Reshape's layer, whose tensor is the same bytes.  The oracle knows neither joins nor graphs, so nothing here
comes from the code under test.  tests/test_composed_graph_host.py pins it to the six older interpreters on models of their families."""
import numpy as np

from tests import add_ref as A
from tests import concat_ref as K
from tests import dilated_ref as D
from tests import grouped_ref as G
from tests import maxpool_ref as R
from tests import pad_ref as P
from tests import resize_ref as Z
from tests import tconv_ref as T

F = np.float32
JOINS = ("add", "concatenation")
OWN = JOINS + ("max_pool_2d", "pad", "transpose_conv", "resize_nearest_neighbor")   # what the oracle does not have


def _strip(L):
    return {k: v for k, v in L.items() if k != "side_of"}


def interpret(tw, O, in_shape, in_q, layers, elem):
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
        """the oracle's model of the layers ls on a tensor of `shape`, and which of its layers are operators of the model under test"""
        if key not in models:
            ls = [_strip(L) for L in ls]
            keep = []
            for L in ls:
                keep += [False] * (len(P.mean_as_pool(L, (1, 1, 1, 1))) - 1 if L["op"] == "mean" else 0) + [True]   # (the Reshape's tensor is the MEAN's)
            twin = D.twin(G.twin(P.twin_layers(ls, shape), shape[-1]))
            models[key] = (O.Model(tw.build_model(shape, q, twin, elem)), keep)
        return models[key]

    def through(mk, t):
        m, keep = mk
        per = [m.run_quantized(v, layers=True)[1] for v in t]
        assert len(per[0]) == len(keep)
        return [np.stack([p[i].reshape(-1) for p in per]) for i in range(len(keep)) if keep[i]]

    def side(k, outs):
        src = layers[k]["side_of"]
        return through(model(("side", k), shape_of[src], q_of[src], [layers[k]]), outs[src])[0]

    def own(i, L, t, outs, n):
        """operator i, one of OWN, on the running tensor t [n, elems]"""
        shp, qi = before[i]
        img = (n,) + tuple(shp[1:])
        if L["op"] in JOINS:
            s = L["skip"]
            skip, q_skip = outs[s], q_of[s]
            if L["op"] == "add":
                return A.add(skip, t, q_skip, qi, L["out_q"], L.get("act")) if L.get("swap") else A.add(t, skip, qi, q_skip, L["out_q"], L.get("act"))
            t, skip = t.reshape(n, -1, shp[-1]), skip.reshape(n, -1, shape_of[s][-1])   # rows of channels
            return K.concat(skip, t, q_skip, qi, L["out_q"]) if L.get("swap") else K.concat(t, skip, qi, q_skip, L["out_q"])
        if L["op"] == "max_pool_2d":
            c0, c1 = R.pool_constants(qi[0], qi[1], L["out_q"][0], L["out_q"][1])
            return R.max_pool_2d(t.reshape(img), L["filter"], L["strides"], L["padding"], L["out_shape"][1:3], c0, c1, L.get("act"), L["out_q"][0], L["out_q"][1])
        if L["op"] == "pad":
            return P.pad(t.reshape(img), L["pads"], qi[1])
        if L["op"] == "resize_nearest_neighbor":
            return Z.resize(t.reshape(img), L["out_shape"][1] // shp[1], L["out_shape"][2] // shp[2])
        assert L["op"] == "transpose_conv"
        N = L["out_shape"][-1]
        bias = np.zeros(N, np.int32) if L.get("bias") is None else np.asarray(L["bias"], np.int32)
        c0 = (F(L["bscale"]) / F(L["out_q"][0])) * (bias - np.asarray(L["bzp"], np.int32)).astype(F)
        c1 = (F(qi[0]) * F(L["fscale"])) / F(L["out_q"][0])
        return T.transpose_conv(t.reshape(img), np.asarray(L["filters"], t.dtype), qi[1], np.asarray(L["fzp"]), L["strides"], L["out_shape"][1:3],
                                c0, c1, L["out_q"][1], L["out_q"][0], L.get("act"))

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
            elif L["op"] in OWN:
                outs[i] = np.asarray(own(i, L, outs[cur], outs, n)).reshape(n, -1)
                cur, i = i, i + 1
            else:  # a run of reference operators on the main chain, up to the next operator of OWN (side operators stepped over)
                idx, j = [], i
                while j < len(layers) and ("side_of" in layers[j] or layers[j]["op"] not in OWN):
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
