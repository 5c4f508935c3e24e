"""Grouped conv_2d by the contract's equivalent statement (include/microflow_amd.h): the dense conv_2d whose filter is block-diagonal,
every element outside a channel's own group holding that channel's filter zero point.  tests/dilated_ref.conv on expand() is the reference."""
import numpy as np


def expand(w, wzp, G, C):
    """w: [N, KH, KW, C / G], wzp: [N] or [1] -> the dense twin [N, KH, KW, C]"""
    w = np.asarray(w)
    N, Cg = w.shape[0], w.shape[3]
    assert Cg * G == C and N % G == 0, (w.shape, G, C)
    d = np.empty(w.shape[:3] + (C,), w.dtype)
    d[:] = np.broadcast_to(np.asarray(wzp).reshape(-1), (N,)).astype(w.dtype).reshape(N, 1, 1, 1)
    for n in range(N):
        g = n // (N // G)
        d[n, :, :, g * Cg:(g + 1) * Cg] = w[n]
    return d


def twin(layers, C_in):
    """tflite_writer layer dicts (C_in: the model input's channels), every grouped Conv2D as its dense twin, which the CPU oracle can run"""
    out, chans, run = [], [], -1   # run: the layer whose output is the running tensor (a side operator does not move it)
    for L in layers:
        if L["op"] == "conv_2d":
            src = L.get("side_of", run)
            C = C_in if src < 0 else chans[src]
            f = np.asarray(L["filters"])
            if f.shape[3] != C:
                L = dict(L, filters=expand(f, L["fzp"], C // f.shape[3], C))
        if "side_of" not in L:
            run = len(out)
        out.append(L)
        chans.append(L["out_shape"][-1])
    return out
