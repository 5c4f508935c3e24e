#!/usr/bin/env python3
"""Writes small .tflite models made of the six operators MicroFlow supports
(microflow-macros/src/lib.rs:138-148), MaxPool2D, ADD (identity and projection shortcuts), CONCATENATION (fire modules and
identity skips), PAD and MEAN, for randomized model-level tests: parser + constant
preparation + kernel routing + run, product vs oracle.  Only the fields the MicroFlow front
end reads are written (tflite.fbs field ids as used by microflow-macros/src/ops/*.rs).

    layers = [dict(op="depthwise_conv_2d", ...), dict(op="conv_2d", ...), ...]
    blob = build_model(input_shape, input_q, layers)

Each layer dict (all quantization parameters are given, nothing is derived):
    conv_2d           filters int8 [N,KH,KW,C], fscale [N or 1], fzp [N or 1], bias int32 [N],
                      bscale [N or 1], bzp [N or 1], padding "same"|"valid", strides (h,w), act,
                      out_shape (1,OH,OW,N), out_q (scale, zp).  side_of = a layer index (-1: the model input): the convolution reads
                      that layer's output instead of the running tensor and does not become the running tensor (a projection
                      shortcut: a later add names this layer as its skip)
    depthwise_conv_2d weights int8 [1,KH,KW,C] + the same fields
    average_pool_2d   filter (h,w), padding, strides, act, out_shape, out_q
    max_pool_2d       the same fields
    fully_connected   weights int8 [N,K], wscale, wzp, bias int32 [N], bscale, bzp, act, out_shape (M,N), out_q
    add               skip (the layer whose output is the second operand; -1: the model input), swap (False: inputs [running, skip];
                      True: [skip, running]), act, out_shape, out_q.  Negative tests place the inputs by hand: inputs = a list of
                      "cur", a layer index (-1: the model input) or dict(shape, q, type=, data=) for a fresh tensor
    concatenation     skip, swap and inputs as add's (the join is along `axis`, default -1: the last), out_shape, out_q; act (a file that
                      loads carries none)
    reshape           out_shape
    softmax           out_shape, out_q
    pad               pads ((top, bottom), (left, right)), out_shape, out_q (the input's, for a model that loads).  Negative tests:
                      paddings (the whole [4, 2] operand, any shape), pad_type (INT32 | INT64), pad_const=False (the operand has no
                      buffer), code ("padv2" | "mirror_pad": the same operator under another builtin code)
    mean              keep_dims (out_shape (1,1,1,C) or (1,C)), out_shape, out_q; axes (default (1, 2)), axes_const=False, axes_type
"""
import struct

import numpy as np

from make_fc_model import FB, Table, TableVec, Vec, emit, prune_2_4

INT32, UINT8, INT64, INT8 = 2, 3, 4, 9
OPCODES = {"add": 0, "average_pool_2d": 1, "concatenation": 2, "conv_2d": 3, "depthwise_conv_2d": 4, "fully_connected": 9, "max_pool_2d": 17, "reshape": 22,
           "softmax": 25, "pad": 34, "mean": 40, "padv2": 60, "mirror_pad": 100}
# BuiltinOptions union type ids (tflite.fbs)
OPT_TYPE = {"add": 11, "concatenation": 10, "conv_2d": 1, "depthwise_conv_2d": 2, "average_pool_2d": 5, "max_pool_2d": 5, "fully_connected": 8, "softmax": 9,
            "reshape": 17, "pad": 22, "mean": 27, "padv2": 43, "mirror_pad": 77}
ACT = {None: 0, "none": 0, "relu": 1, "relu6": 3, 0: 0, 1: 1, 3: 3}
PAD = {"same": 0, "valid": 1, 0: 0, 1: 1}


def _quant(scales, zps):
    # QuantizationParameters { scale:2 zero_point:3 }
    scales, zps = np.atleast_1d(scales), np.atleast_1d(zps)
    return Table({2: ("ref", Vec("<f", [float(np.float32(v)) for v in scales])),
                  3: ("ref", Vec("<q", [int(v) for v in zps], align=8))})


def _tensor(shape, ttype, buffer, scales, zps):
    # Tensor { shape:0 type:1 buffer:2 quantization:4 }
    return Table({0: ("ref", Vec("<i", [int(v) for v in shape])), 1: ("i8", ttype), 2: ("u32", buffer),
                  4: ("ref", _quant(scales, zps))})


def build_model(input_shape, input_q, layers, elem=INT8):
    tensors, buffers, operators = [], [Table({})], []
    used_ops = []

    def add_buffer(arr):
        buffers.append(Table({0: ("ref", Vec(None, np.ascontiguousarray(arr).tobytes(), align=16))}))
        return len(buffers) - 1

    def add_tensor(shape, ttype, buf, scales, zps):
        tensors.append(_tensor(shape, ttype, buf, scales, zps))
        return len(tensors) - 1

    cur = add_tensor(input_shape, elem, 0, input_q[0], input_q[1])
    first = cur
    outs = []  # every layer's output tensor index (an ADD names its second operand by layer)
    wdt = np.uint8 if elem == UINT8 else np.int8
    for L in layers:
        op = L["op"]
        code = L.get("code", op)  # (negative tests: the layer written under another builtin code)
        if "detach_input" in L:  # negative tests: this operator reads a fresh tensor instead of the running one
            cur = add_tensor(L["detach_input"], elem, 0, input_q[0], input_q[1])
        if code not in used_ops:
            used_ops.append(code)
        oc = used_ops.index(code)
        if op in ("conv_2d", "depthwise_conv_2d"):
            w = np.asarray(L["filters" if op == "conv_2d" else "weights"], wdt)
            tw = add_tensor(w.shape, elem, add_buffer(w), L["fscale"], L["fzp"])
            tb = add_tensor((w.shape[0] if op == "conv_2d" else w.shape[3],), INT32,
                            add_buffer(np.asarray(L["bias"], np.int32)), L["bscale"], L["bzp"])
            out = add_tensor(L["out_shape"], L.get("out_type", elem), 0, *L["out_q"])  # (out_type: negative tests)
            if op == "conv_2d":  # Conv2DOptions { padding:0 stride_w:1 stride_h:2 act:3 }
                opts = Table({0: ("i8", PAD[L["padding"]]), 1: ("i32", L["strides"][1]), 2: ("i32", L["strides"][0]),
                              3: ("i8", ACT[L.get("act")])})
            else:                # DepthwiseConv2DOptions { padding:0 stride_w:1 stride_h:2 depth_multiplier:3 act:4 }
                opts = Table({0: ("i8", PAD[L["padding"]]), 1: ("i32", L["strides"][1]), 2: ("i32", L["strides"][0]),
                              3: ("i32", L.get("depth_multiplier", 1)), 4: ("i8", ACT[L.get("act")])})
            ins = [cur, tw, tb]
            if "side_of" in L:
                ins[0] = first if L["side_of"] < 0 else outs[L["side_of"]]
        elif op in ("average_pool_2d", "max_pool_2d"):
            out = add_tensor(L["out_shape"], elem, 0, *L["out_q"])
            # Pool2DOptions { padding:0 stride_w:1 stride_h:2 filter_width:3 filter_height:4 act:5 }
            opts = Table({0: ("i8", PAD[L["padding"]]), 1: ("i32", L["strides"][1]), 2: ("i32", L["strides"][0]),
                          3: ("i32", L["filter"][1]), 4: ("i32", L["filter"][0]), 5: ("i8", ACT[L.get("act")])})
            ins = [cur]
        elif op == "fully_connected":
            w = np.asarray(L["weights"], wdt)
            tw = add_tensor(w.shape, elem, add_buffer(w), L["wscale"], L["wzp"])
            tb = add_tensor((w.shape[0],), INT32, add_buffer(np.asarray(L["bias"], np.int32)), L["bscale"], L["bzp"])
            out = add_tensor(L["out_shape"], elem, 0, *L["out_q"])
            opts = Table({0: ("i8", ACT[L.get("act")])})
            ins = [cur, tw, tb]
        elif op == "reshape":
            src_q = L.get("out_q")
            out = add_tensor(L["out_shape"], elem, 0, *(src_q or (1.0, 0)))
            shp = add_tensor((len(L["out_shape"]),), INT32, add_buffer(np.asarray(L["out_shape"], np.int32)), 1.0, 0)
            opts = Table({0: ("ref", Vec("<i", [int(v) for v in L["out_shape"]]))})
            ins = [cur, shp]
        elif op == "softmax":
            out = add_tensor(L["out_shape"], elem, 0, *L["out_q"])
            opts = Table({0: ("f32", 1.0)})
            ins = [cur]
        elif op in ("add", "concatenation"):
            def place(item):
                if isinstance(item, dict):
                    data = item.get("data")
                    return add_tensor(item["shape"], item.get("type", elem), 0 if data is None else add_buffer(data), *item["q"])
                return cur if item == "cur" else first if item < 0 else outs[item]
            if "inputs" in L:
                ins = [place(i) for i in L["inputs"]]
            else:
                ins = [place(L["skip"]), cur] if L.get("swap") else [cur, place(L["skip"])]
            out = add_tensor(L["out_shape"], L.get("out_type", elem), 0, *L["out_q"])
            if op == "add":
                opts = Table({0: ("i8", ACT[L.get("act")])})  # AddOptions { fused_activation_function:0 }
            else:            # ConcatenationOptions { axis:0 fused_activation_function:1 }
                opts = Table({0: ("i32", int(L.get("axis", -1))), 1: ("i8", ACT[L.get("act")])})
        elif op == "pad":
            pv = np.asarray(L["paddings"] if "paddings" in L else ((0, 0),) + tuple(tuple(p) for p in L["pads"]) + ((0, 0),))
            ptype = L.get("pad_type", INT32)
            pbuf = add_buffer(pv.astype(np.int64 if ptype == INT64 else np.int32)) if L.get("pad_const", True) else 0
            tp = add_tensor(pv.shape, ptype, pbuf, 1.0, 0)
            out = add_tensor(L["out_shape"], L.get("out_type", elem), 0, *L["out_q"])
            opts = Table({})  # PadOptions {}
            ins = [cur, tp]
        elif op == "mean":
            ax = np.asarray(L.get("axes", (1, 2)), np.int32)
            ta = add_tensor(ax.shape, L.get("axes_type", INT32), add_buffer(ax) if L.get("axes_const", True) else 0, 1.0, 0)
            out = add_tensor(L["out_shape"], elem, 0, *L["out_q"])
            opts = Table({0: ("u8", int(bool(L.get("keep_dims", False))))})  # ReducerOptions { keep_dims:0 }
            ins = [cur, ta]
        else:
            raise ValueError(op)
        # Operator { opcode_index:0 inputs:1 outputs:2 builtin_options_type:3 builtin_options:4 }
        operators.append(Table({0: ("u32", oc), 1: ("ref", Vec("<i", ins)), 2: ("ref", Vec("<i", [out])),
                                3: ("u8", OPT_TYPE[code]), 4: ("ref", opts)}))
        if "side_of" not in L:
            cur = out
        outs.append(out)
    subgraph = Table({0: ("ref", TableVec(tensors)), 1: ("ref", Vec("<i", [first])), 2: ("ref", Vec("<i", [cur])),
                      3: ("ref", TableVec(operators))})
    # OperatorCode { deprecated_builtin_code:0 builtin_code:3 }
    codes = TableVec([Table({0: ("i8", OPCODES[o]), 3: ("i32", OPCODES[o])}) for o in used_ops])
    model = Table({0: ("u32", 3), 1: ("ref", codes), 2: ("ref", TableVec([subgraph])), 4: ("ref", TableVec(buffers))})
    fb = FB()
    fb.buf += bytes(4) + b"TFL3"
    root = emit(fb, model)
    struct.pack_into("<I", fb.buf, 0, root)
    return bytes(fb.buf)


def random_cnn(rng, elem=INT8, per_channel=True, wzp_nonzero=False, tail="fc"):
    """A random small network touching every operator: conv (KxK) -> depthwise -> conv 1x1 ->
    average pool -> reshape -> fully connected -> softmax (or conv 1x1 head + reshape + softmax)."""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    mid = (lo + hi) // 2
    H, W, C = int(rng.integers(7, 13)), int(rng.integers(7, 13)), int(rng.integers(1, 4))

    def q(scale_lo=0.02, scale_hi=0.08, relu=False):
        return (float(np.float32(rng.uniform(scale_lo, scale_hi))), int(lo if relu else rng.integers(lo + 20, hi - 20)))

    def wq(n):
        sc = rng.uniform(0.002, 0.01, n if per_channel else 1).astype(np.float32)
        zp = rng.integers(mid - 10, mid + 10, n if per_channel else 1) if wzp_nonzero else np.full(n if per_channel else 1, mid)
        return sc, zp

    def conv_like(op, in_shape, n, kh, kw, strides, padding, act, in_scale):
        _, h, w, c = in_shape
        if padding == "same":
            oh, ow = -(-h // strides[0]), -(-w // strides[1])
        else:
            oh, ow = (h - kh) // strides[0] + 1, (w - kw) // strides[1] + 1
        sc, zp = wq(n)
        shape = (n, kh, kw, c) if op == "conv_2d" else (1, kh, kw, n)
        wts = rng.integers(lo, hi, shape)
        bias = rng.integers(-500, 500, n)
        bscale = (sc * np.float32(in_scale)).astype(np.float32)
        d = dict(op=op, fscale=sc, fzp=zp, bias=bias, bscale=bscale, bzp=np.zeros_like(zp), padding=padding,
                 strides=strides, act=act, out_shape=(1, oh, ow, n), out_q=q(0.05, 0.2, relu=act in ("relu", "relu6")))
        d["filters" if op == "conv_2d" else "weights"] = wts
        return d

    in_q = q()
    layers = []
    L = conv_like("conv_2d", (1, H, W, C), int(rng.integers(2, 9)), int(rng.integers(1, 4)), int(rng.integers(1, 4)),
                  (int(rng.integers(1, 3)), int(rng.integers(1, 3))), str(rng.choice(["same", "valid"])),
                  str(rng.choice(["none", "relu", "relu6"])), in_q[0])
    layers.append(L)
    shp = L["out_shape"]
    L = conv_like("depthwise_conv_2d", shp, shp[3], int(rng.integers(1, 4)), int(rng.integers(1, 4)), (1, 1), "same",
                  str(rng.choice(["none", "relu6"])), layers[-1]["out_q"][0])
    layers.append(L)
    shp = L["out_shape"]
    L = conv_like("conv_2d", shp, int(rng.integers(2, 7)), 1, 1, (1, 1), "same", "relu", layers[-1]["out_q"][0])
    layers.append(L)
    shp = L["out_shape"]
    fh, fw = min(2, shp[1]), min(2, shp[2])
    pool_out = (1, (shp[1] - fh) // fh + 1, (shp[2] - fw) // fw + 1, shp[3])
    layers.append(dict(op="average_pool_2d", filter=(fh, fw), padding="valid", strides=(fh, fw), act="none",
                       out_shape=pool_out, out_q=q(0.05, 0.2)))
    flat = int(np.prod(pool_out))
    classes = int(rng.integers(2, 6))
    if tail == "fc":
        layers.append(dict(op="reshape", out_shape=(1, flat), out_q=layers[-1]["out_q"]))
        sc, zp = wq(1)
        layers.append(dict(op="fully_connected", weights=rng.integers(lo, hi, (classes, flat)), wscale=sc[:1], wzp=zp[:1],
                           bias=rng.integers(-300, 300, classes), bscale=sc[:1] * np.float32(layers[-1]["out_q"][0]),
                           bzp=[0], act="none", out_shape=(1, classes), out_q=q(0.1, 0.3)))
    else:
        L = conv_like("conv_2d", pool_out, classes, 1, 1, (1, 1), "same", "none", layers[-1]["out_q"][0])
        layers.append(L)
        layers.append(dict(op="reshape", out_shape=(1, int(np.prod(L["out_shape"]))), out_q=L["out_q"]))
        classes = int(np.prod(L["out_shape"]))
    layers.append(dict(op="softmax", out_shape=(1, classes), out_q=(1.0 / 256.0, lo)))
    return build_model((1, H, W, C), in_q, layers, elem)


def speech_like(rng, elem=INT8, fc_wzp=0, per_channel=True, act="relu"):
    """The layer structure and shapes of speech.tflite (TinyConv: Reshape -> DepthwiseConv2D 10x8 stride 2 SAME with one
    input channel and 8 output channels -> FullyConnected 4000 -> 4 -> Softmax) with random weights and quantization,
    incl. a non-zero FullyConnected weight zero point, which the shipped model does not have."""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    mid = (lo + hi) // 2
    in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo, lo + 40)))
    dsc = rng.uniform(0.002, 0.01, 8 if per_channel else 1).astype(np.float32)
    dzp = np.full(8 if per_channel else 1, mid)
    dw_out = (float(np.float32(rng.uniform(0.05, 0.2))), int(lo if act in ("relu", "relu6") else rng.integers(lo + 20, hi - 20)))
    layers = [dict(op="reshape", out_shape=(1, 49, 40, 1), out_q=in_q),
              dict(op="depthwise_conv_2d", weights=rng.integers(lo, hi, (1, 10, 8, 8)), fscale=dsc, fzp=dzp,
                   bias=rng.integers(-2000, 2000, 8), bscale=(dsc * np.float32(in_q[0])).astype(np.float32),
                   bzp=np.zeros_like(dzp), padding="same", strides=(2, 2), act=act, out_shape=(1, 25, 20, 8), out_q=dw_out)]
    fsc = np.float32(rng.uniform(0.001, 0.004))
    layers.append(dict(op="fully_connected", weights=rng.integers(lo, hi, (4, 4000)), wscale=[fsc], wzp=[mid + fc_wzp],
                       bias=rng.integers(-3000, 3000, 4), bscale=[fsc * np.float32(dw_out[0])], bzp=[0], act="none",
                       out_shape=(1, 4), out_q=(float(np.float32(rng.uniform(0.3, 0.9))), int(rng.integers(lo + 60, hi - 60)))))
    layers.append(dict(op="softmax", out_shape=(1, 4), out_q=(1.0 / 256.0, lo)))
    return build_model((1, 1960), in_q, layers, elem)


def kws_like(rng, shape, stem, classes, elem=INT8, fc_wzp=0, softmax=True, wmax=None, act="relu", stem_wzp=False, reshape=True):
    """TensorFlow's keyword-spotting "tiny_conv" family at any geometry: input [1, H, W, 1] (shape = (H, W)) -> a one-channel
    convolution -> Reshape -> FullyConnected(classes) -> optionally a Softmax.  stem = (kind, N, KH, KW, (sh, sw), padding) gives the
    convolution in full: kind "dw" (DepthwiseConv2D with depth multiplier N, what the converter writes) or "conv" (Conv2D with N
    filters), padding "same" or "valid".  Per-channel filter quantization with the zero points at the type's middle (stem_wzp:
    off it), one FullyConnected weight zero point at middle + fc_wzp.  `wmax`: convolution and FullyConnected weights within
    +-wmax of the middle (None: the full range); the scales keep both operators' outputs spread over the range."""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    mid = (lo + hi) // 2
    H, W = (int(v) for v in shape)
    kind, N, KH, KW, (sh, sw), padding = stem
    N, KH, KW = int(N), int(KH), int(KW)
    if padding == "same":
        OH, OW = -(-H // sh), -(-W // sw)
    else:
        OH, OW = (H - KH) // sh + 1, (W - KW) // sw + 1
    wm = 128 if wmax is None else int(wmax)

    def weights(shp):
        return rng.integers(lo, hi, shp) if wmax is None else rng.integers(mid - wm, mid + wm + 1, shp)

    in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo, lo + 40)))
    sc = rng.uniform(0.002, 0.01, N).astype(np.float32)
    zp = rng.integers(mid - 10, mid + 11, N) if stem_wzp else np.full(N, mid)
    if stem_wzp and not np.any(zp != mid):
        zp[0] = mid + 3
    relu = act in ("relu", "relu6")
    c_out = (float(np.float32(in_q[0] * float(sc.mean()) * 50.0 * np.sqrt(KH * KW) * wm / 128.0)),
             int(lo if relu else rng.integers(lo + 20, hi - 20)))
    d = dict(op="depthwise_conv_2d" if kind == "dw" else "conv_2d", fscale=sc, fzp=zp, bias=rng.integers(-2000, 2000, N),
             bscale=(sc * np.float32(in_q[0])).astype(np.float32), bzp=np.zeros(N, np.int64), padding=padding, strides=(sh, sw), act=act,
             out_shape=(1, OH, OW, N), out_q=c_out)
    if kind == "dw":
        d["weights"], d["depth_multiplier"] = weights((1, KH, KW, N)), N
    else:
        d["filters"] = weights((N, KH, KW, 1))
    layers = [d]
    K = OH * OW * N
    if reshape:
        layers.append(dict(op="reshape", out_shape=(1, K), out_q=c_out))
    fsc = np.float32(rng.uniform(0.001, 0.004))
    f_out = (float(np.float32(c_out[0] * fsc * 40.0 * np.sqrt(K) * wm / 128.0)), int(rng.integers(lo + 60, hi - 60)))
    layers.append(dict(op="fully_connected", weights=weights((int(classes), K)), wscale=[fsc], wzp=[mid + fc_wzp],
                       bias=rng.integers(-3000, 3000, int(classes)), bscale=[fsc * np.float32(c_out[0])], bzp=[0], act="none",
                       out_shape=(1, int(classes)), out_q=f_out))
    if softmax:
        layers.append(dict(op="softmax", out_shape=(1, int(classes)), out_q=(1.0 / 256.0, lo)))
    return build_model((1, H, W, 1), in_q, layers, elem)


def mlp(rng, sizes, elem=INT8, wzp_nonzero=False, softmax=False, act="relu", sparse24=()):
    """A FullyConnected-only network: sizes = (K, N1, N2, ...) gives the layers K -> N1 -> N2 ...; every hidden layer has
    the activation `act`, the last one none, optionally followed by a Softmax.  Per-tensor weight quantization (what
    FullyConnected has), random scales and zero points; wzp_nonzero gives every layer a weight zero point off the middle.
    sparse24: indices of layers whose weights are pruned to 2:4 sparsity along K in the int8 domain (make_fc_model.prune_2_4;
    the same random draws as without it)."""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    mid = (lo + hi) // 2
    q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, hi - 20)))
    in_q, layers = q, []
    for i in range(len(sizes) - 1):
        K, N = int(sizes[i]), int(sizes[i + 1])
        last = i == len(sizes) - 2
        a = "none" if last else act
        wsc = np.float32(rng.uniform(0.002, 0.02))
        wzp = mid + (int(rng.integers(-20, 21)) or 7 if wzp_nonzero else 0)
        # output scale chosen so that the layer's outputs spread over the int8 range instead of saturating
        osc = float(np.float32(q[0] * wsc * 120.0 * np.sqrt(K)))
        ozp = lo if a in ("relu", "relu6") else int(rng.integers(lo + 20, hi - 20))
        w = rng.integers(lo, hi, (N, K))
        if i in sparse24:
            w = prune_2_4((w - (lo + 128)).astype(np.int8)).astype(np.int64) + (lo + 128)
        layers.append(dict(op="fully_connected", weights=w, wscale=[wsc], wzp=[wzp],
                           bias=rng.integers(-2000, 2000, N), bscale=[np.float32(q[0]) * wsc], bzp=[0], act=a,
                           out_shape=(1, N), out_q=(osc, ozp)))
        q = (osc, ozp)
    if softmax:
        layers.append(dict(op="softmax", out_shape=(1, int(sizes[-1])), out_q=(1.0 / 256.0, lo)))
    return build_model((1, int(sizes[0])), in_q, layers, elem)


def pool_head(rng, shape, sizes, elem=INT8, wzp_nonzero=False, softmax=False, same_q=False):
    """The usual classifier head alone: input [1, H, W, C] (shape = (H, W, C)) -> AveragePool2D over the whole image -> Reshape
    -> FullyConnected layers C -> sizes[0] -> sizes[1] ... (relu between them, none after the last) -> optionally a Softmax.
    Per-tensor weight quantization as in mlp; wzp_nonzero gives every layer a weight zero point off the middle.  same_q: the pool's
    output has its input's scale and zero point, so that the pooled value is the plain mean and lands on .5 ties (H W even)."""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    mid = (lo + hi) // 2
    H, W, C = (int(v) for v in shape)
    in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, hi - 20)))
    # (a mean of uniform bytes has 1 / sqrt(H W) of their spread: a finer output scale keeps the pooled values spread out)
    q = in_q if same_q else (float(np.float32(in_q[0] * rng.uniform(0.8, 1.2) / np.sqrt(np.sqrt(H * W)))), int(rng.integers(lo + 20, hi - 20)))
    layers = [dict(op="average_pool_2d", filter=(H, W), padding="valid", strides=(H, W), act="none", out_shape=(1, 1, 1, C), out_q=q),
              dict(op="reshape", out_shape=(1, C), out_q=q)]
    K = C
    for i, N in enumerate(int(v) for v in sizes):
        last = i == len(sizes) - 1
        a = "none" if last else "relu"
        wsc = np.float32(rng.uniform(0.002, 0.02))
        wzp = mid + (int(rng.integers(-20, 21)) or 7 if wzp_nonzero else 0)
        osc = float(np.float32(q[0] * wsc * (60.0 if i == 0 else 120.0) * np.sqrt(K)))
        ozp = lo if a == "relu" else int(rng.integers(lo + 20, hi - 20))
        layers.append(dict(op="fully_connected", weights=rng.integers(lo, hi, (N, K)), wscale=[wsc], wzp=[wzp],
                           bias=rng.integers(-2000, 2000, N), bscale=[np.float32(q[0]) * wsc], bzp=[0], act=a,
                           out_shape=(1, N), out_q=(osc, ozp)))
        q, K = (osc, ozp), N
    if softmax:
        layers.append(dict(op="softmax", out_shape=(1, K), out_q=(1.0 / 256.0, lo)))
    return build_model((1, H, W, C), in_q, layers, elem)


def conv_net(rng, input_shape, convs, elem=INT8, wzp_nonzero=False, head=None, wmax=None, in_zp=None, act_scale=None):
    """A convolution stack: input_shape = (H, W, C); convs = [(op, N, K, stride), ...] with op "conv" (KxK Conv2D to N channels)
    or "dw" (KxK depthwise, N ignored), all SAME, relu6; per-channel filter quantization, filter zero points off the middle when
    wzp_nonzero (Conv2D only: the depthwise kernels keep theirs at the middle).  head = classes: AveragePool over the whole
    image, FullyConnected(classes) and Softmax after the stack.  Output scales keep every layer's outputs spread over the range.
    `wmax`: weights within +-wmax of the type's middle (None: the full range, the worst case for the accumulator bounds that decide
    the epilogue form); `in_zp`: the input's zero point (None: a random one; every later tensor's is the type's minimum);
    `act_scale`: every tensor, the input included, has this scale (6 / 255: relu6 is then the type's whole range, as in
    person_detect.tflite) and the filter scales are person_detect_like's, which keep the activations of a deep stack spread over it --
    the default's growing output scales leave relu6 a few dozen levels after a few layers."""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    mid = (lo + hi) // 2
    H, W, C = input_shape
    in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, hi - 20)))
    if in_zp is not None:
        in_q = (in_q[0], int(in_zp))
    if act_scale is not None:
        in_q = (float(np.float32(act_scale)), in_q[1])
    q, layers = in_q, []
    for op, n, k, s in convs:
        d = _conv_layer(rng, (H, W, C), q, op == "dw", n, k, s, elem=elem, wzp="conv" if wzp_nonzero else "none", wmax=wmax, act_scale=act_scale)
        layers.append(d)
        q, (_, H, W, C) = d["out_q"], d["out_shape"]
    if head:
        layers.append(dict(op="average_pool_2d", filter=(H, W), padding="valid", strides=(H, W), act="none",
                           out_shape=(1, 1, 1, C), out_q=q))
        layers.append(dict(op="reshape", out_shape=(1, C), out_q=q))
        wsc = np.float32(rng.uniform(0.002, 0.02))
        osc = float(np.float32(q[0] * wsc * 60.0 * np.sqrt(C)))
        layers.append(dict(op="fully_connected", weights=rng.integers(lo, hi, (head, C)), wscale=[wsc], wzp=[mid],
                           bias=rng.integers(-2000, 2000, head), bscale=[np.float32(q[0]) * wsc], bzp=[0], act="none",
                           out_shape=(1, head), out_q=(osc, int(rng.integers(lo + 20, hi - 20)))))
        layers.append(dict(op="softmax", out_shape=(1, head), out_q=(1.0 / 256.0, lo)))
    return build_model((1,) + tuple(input_shape), in_q, layers, elem)


def _same_or_valid(size, k, s, padding):
    return -(-size // s) if padding == "same" else (size - k) // s + 1


def _conv_layer(rng, shape, q, dw, n, k, stride, padding="same", act="relu6", elem=INT8, wzp="none", wmax=None, act_scale=None):
    """conv_net's per-layer form, one layer dict: a k x k Conv2D to n channels, or (dw) a k x k depthwise, on a tensor shape = (H, W, C)
    of quantisation q; per-channel filter quantisation; the output scale keeps the outputs spread, or is act_scale with
    person_detect_like's filter scales; the output zero point is the type's minimum behind relu / relu6 and a random one without an
    activation.  wzp: filter zero points off the middle -- "conv": Conv2D only, conv_net's draw; "all": the depthwise ones too, both
    with inverted_residual_net's draw, which never lands on the middle."""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    mid = (lo + hi) // 2
    H, W, C = (int(v) for v in shape)
    oh, ow = _same_or_valid(H, k, stride, padding), _same_or_valid(W, k, stride, padding)
    n = C if dw else int(n)
    sc = rng.uniform(0.002, 0.01, n).astype(np.float32)
    if wzp == "all":
        zp = rng.integers(mid - 12, mid + 13, n)
        zp[zp == mid] = mid + 5
    else:
        zp = rng.integers(mid - 10, mid + 11, n) if wzp == "conv" and not dw else np.full(n, mid)
    taps = k * k * (1 if dw else C)
    osc = float(np.float32(q[0] * float(sc.mean()) * 60.0 * np.sqrt(taps)))
    if act_scale is not None:
        sc = (rng.uniform(0.6, 1.4, n) * 2.2 / (74.0 * np.sqrt(taps)) * (128.0 / (wmax or 128))).astype(np.float32)
        osc = float(np.float32(act_scale))
    ozp = lo if act in ("relu", "relu6") else int(rng.integers(lo + 20, hi - 20))
    d = dict(op="depthwise_conv_2d" if dw else "conv_2d", fscale=sc, fzp=zp, bias=rng.integers(-500, 500, n),
             bscale=(sc * np.float32(q[0])).astype(np.float32), bzp=np.zeros(n, np.int64), padding=padding, strides=(stride, stride),
             act=act, out_shape=(1, oh, ow, n), out_q=(osc, ozp))
    wshape = (1, k, k, n) if dw else (n, k, k, C)
    d["weights" if dw else "filters"] = rng.integers(lo, hi, wshape) if wmax is None else rng.integers(mid - wmax, mid + wmax + 1, wshape)
    return d


def _fc_layer(rng, K, N, q, act="none", elem=INT8, wzp_off=0):
    """lenet's FullyConnected form, one layer dict: K -> N on one row, per-tensor weight quantisation with the zero point at the
    middle + wzp_off, an output scale that keeps the outputs spread"""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    mid = (lo + hi) // 2
    wsc = np.float32(rng.uniform(0.002, 0.02))
    osc = float(np.float32(q[0] * wsc * 60.0 * np.sqrt(K)))
    ozp = lo if act in ("relu", "relu6") else int(rng.integers(lo + 20, hi - 20))
    return dict(op="fully_connected", weights=rng.integers(lo, hi, (N, K)), wscale=[wsc], wzp=[mid + wzp_off],
                bias=rng.integers(-2000, 2000, N), bscale=[np.float32(q[0]) * wsc], bzp=[0], act=act, out_shape=(1, N), out_q=(osc, ozp))


def conv_pool_layers(rng, shape, in_q, n, k, stride=1, padding="valid", act="relu", pool=(2, 2), pool_stride=2, pool_padding="valid",
                     pool_act="none", pool_q="same", elem=INT8, wzp_nonzero=False, wmax=None, pool_op="avg"):
    """The two layers of one stage, Conv2D k x k (shape = (H, W, C) -> n channels, per-channel filter quantisation, filter zero points
    off the middle with wzp_nonzero, weights over the full range unless wmax) -> AveragePool2D (pool_op="avg") or MaxPool2D ("max")
    pool[0] x pool[1]; -> (layers, the
    stage's output (H, W, C), its quantisation).  pool_q: "same" -- the pool's output has its input's scale and zero point, so the
    pooled value is the plain mean and lands on .5 ties -- or a factor on the scale (with a random zero point unless the pool has an
    activation, which pins it to the type's minimum).  `pool` is the window; pool="avg" | "max" names the operator instead (as lenet's
    argument does) and leaves the window at 2 x 2 -- with another window the operator goes in pool_op."""
    if isinstance(pool, str):
        pool, pool_op = (2, 2), pool
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    mid = (lo + hi) // 2
    H, W, C = (int(v) for v in shape)
    oh, ow = _same_or_valid(H, k, stride, padding), _same_or_valid(W, k, stride, padding)
    sc = rng.uniform(0.002, 0.01, n).astype(np.float32)
    zp = rng.integers(mid - 10, mid + 11, n) if wzp_nonzero else np.full(n, mid)
    span = 128 if wmax is None else wmax
    osc = float(np.float32(in_q[0] * float(sc.mean()) * 60.0 * np.sqrt(k * k * C) * span / 128.0))
    ozp = lo if act in ("relu", "relu6") else int(rng.integers(lo + 20, hi - 20))
    wshape = (n, k, k, C)
    conv = dict(op="conv_2d", filters=rng.integers(lo, hi, wshape) if wmax is None else rng.integers(mid - wmax, mid + wmax + 1, wshape),
                fscale=sc, fzp=zp, bias=rng.integers(-500, 500, n), bscale=(sc * np.float32(in_q[0])).astype(np.float32),
                bzp=np.zeros(n, np.int64), padding=padding, strides=(stride, stride), act=act, out_shape=(1, oh, ow, n), out_q=(osc, ozp))
    ph, pw = _same_or_valid(oh, pool[0], pool_stride, pool_padding), _same_or_valid(ow, pool[1], pool_stride, pool_padding)
    if pool_q == "same":
        pq = (osc, ozp)
    else:
        pq = (float(np.float32(osc * pool_q)), lo if pool_act in ("relu", "relu6") else int(rng.integers(lo + 20, hi - 20)))
    pl = dict(op={"avg": "average_pool_2d", "max": "max_pool_2d"}[pool_op], filter=tuple(pool), padding=pool_padding, strides=(pool_stride, pool_stride), act=pool_act,
              out_shape=(1, ph, pw, n), out_q=pq)
    return [conv, pl], (ph, pw, n), pq


def conv_pool(rng, shape, n, k, elem=INT8, in_zp=None, **kw):
    """One Conv2D + AveragePool2D (or MaxPool2D: pool="max", or pool_op="max" beside a window) stage as a model of its own
    (conv_pool_layers' geometry arguments)."""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, hi - 20)) if in_zp is None else int(in_zp))
    layers, _, _ = conv_pool_layers(rng, shape, in_q, n, k, elem=elem, **kw)
    return build_model((1,) + tuple(int(v) for v in shape), in_q, layers, elem)


def lenet_layers(rng, shape=(28, 28, 1), convs=((6, 5), (16, 5)), fcs=(120, 84, 10), elem=INT8, wzp_nonzero=False, softmax=True, pool="avg"):
    """lenet's (input shape, input quantisation, layer dicts): what build_model takes, for tests that write parts of the stack as
    models of their own."""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, hi - 20)))
    q, cur, layers = in_q, tuple(int(v) for v in shape), []
    for n, k in convs:
        stage, cur, q = conv_pool_layers(rng, cur, q, int(n), int(k), elem=elem, wzp_nonzero=wzp_nonzero, pool_op=pool)
        layers += stage
    K = cur[0] * cur[1] * cur[2]
    layers.append(dict(op="reshape", out_shape=(1, K), out_q=q))
    for i, N in enumerate(int(v) for v in fcs):
        layers.append(_fc_layer(rng, K, N, q, "none" if i == len(fcs) - 1 else "relu", elem, 7 if wzp_nonzero else 0))
        q, K = layers[-1]["out_q"], N
    if softmax:
        layers.append(dict(op="softmax", out_shape=(1, K), out_q=(1.0 / 256.0, lo)))
    return (1,) + tuple(int(v) for v in shape), in_q, layers


def lenet(rng, shape=(28, 28, 1), convs=((6, 5), (16, 5)), fcs=(120, 84, 10), elem=INT8, wzp_nonzero=False, softmax=True, pool="avg"):
    """LeNet: per (n, k) of convs a stage Conv2D k x k VALID + relu -> AveragePool2D (pool="avg") or MaxPool2D ("max") 2 x 2 stride 2;
    Reshape; FullyConnected layers (relu between them, none after the last); Softmax.  LeNet-5 on 28 x 28 digits by default;
    shape = (32, 32, 3) with wider convs is the CIFAR-style stack.  Quantisation as conv_pool_layers and pool_head."""
    in_shape, in_q, layers = lenet_layers(rng, shape, convs, fcs, elem, wzp_nonzero, softmax, pool)
    return build_model(in_shape, in_q, layers, elem)


def ds_cnn(rng, shape=(49, 10), filters=64, blocks=4, classes=12, stem=(10, 4, (2, 2)), elem=INT8, wzp_nonzero=False):
    """The MLPerf-Tiny keyword spotter's stack (DS-CNN): shape = (frames, coefficients) of ONE channel -- 49 x 10 MFCCs; Conv2D with
    a stem = (KH, KW, strides) filter (conv_net writes square ones only) to `filters` channels, `blocks` x (depthwise 3x3 + 1x1
    Conv2D, `filters` channels, stride 1), all SAME and relu; AveragePool2D over the whole image, FullyConnected(classes), Softmax.
    Per-channel filter quantization; with wzp_nonzero the Conv2D filter zero points sit off the middle (the depthwise kernels keep
    theirs at the middle, as in conv_net).  Every activation tensor has the input's scale and the filter scales keep a deep stack's
    outputs spread over the range (conv_net's act_scale form), so that the Softmax at the end still tells the classes apart."""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    mid = (lo + hi) // 2
    (H, W), C = shape, 1
    in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, hi - 20)))
    q, layers = in_q, []

    def conv(dw, n, kh, kw, strides):
        nonlocal q, H, W, C
        oh, ow = -(-H // strides[0]), -(-W // strides[1])
        taps = kh * kw * (1 if dw else C)
        sc = (rng.uniform(0.6, 1.4, n) * 2.2 / (74.0 * np.sqrt(taps))).astype(np.float32)   # (conv_net's act_scale form)
        zp = rng.integers(mid - 10, mid + 11, n) if wzp_nonzero and not dw else np.full(n, mid)
        d = dict(op="depthwise_conv_2d" if dw else "conv_2d", fscale=sc, fzp=zp, bias=rng.integers(-500, 500, n),
                 bscale=(sc * np.float32(q[0])).astype(np.float32), bzp=np.zeros(n, np.int64), padding="same", strides=tuple(strides),
                 act="relu", out_shape=(1, oh, ow, n), out_q=(q[0], lo))
        d["weights" if dw else "filters"] = rng.integers(lo, hi, (1, kh, kw, n) if dw else (n, kh, kw, C))
        layers.append(d)
        q, H, W, C = d["out_q"], oh, ow, n

    conv(False, filters, stem[0], stem[1], stem[2])
    for _ in range(blocks):
        conv(True, filters, 3, 3, (1, 1))
        conv(False, filters, 1, 1, (1, 1))
    layers.append(dict(op="average_pool_2d", filter=(H, W), padding="valid", strides=(H, W), act="none", out_shape=(1, 1, 1, C), out_q=q))
    layers.append(dict(op="reshape", out_shape=(1, C), out_q=q))
    wsc = np.float32(rng.uniform(0.002, 0.02))
    osc = float(np.float32(q[0] * wsc * 60.0 * np.sqrt(C)))
    layers.append(dict(op="fully_connected", weights=rng.integers(lo, hi, (classes, C)), wscale=[wsc], wzp=[mid],
                       bias=rng.integers(-2000, 2000, classes), bscale=[np.float32(q[0]) * wsc], bzp=[0], act="none",
                       out_shape=(1, classes), out_q=(osc, int(rng.integers(lo + 20, hi - 20)))))
    layers.append(dict(op="softmax", out_shape=(1, classes), out_q=(1.0 / 256.0, lo)))
    return build_model((1, int(shape[0]), int(shape[1]), 1), in_q, layers, elem)


def _add_layer(rng, skip, shape, q_run, q_skip, act="none", elem=INT8, swap=False):
    """one ADD layer dict: the running tensor (q_run) + the output of layer `skip` (q_skip; -1: the model input), an output scale that
    keeps the sum spread over the range"""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    osc = float(np.float32((q_run[0] + q_skip[0]) * rng.uniform(0.55, 0.75)))
    ozp = lo if act in ("relu", "relu6") else int(rng.integers(lo + 40, hi - 40))
    return dict(op="add", skip=int(skip), swap=bool(swap), act=act, out_shape=tuple(shape), out_q=(osc, ozp))


def inverted_residual_net(rng, input_shape, blocks, elem=INT8, wzp_nonzero=False, head=10, residual=False):
    return build_model(*inverted_residual_layers(rng, input_shape, blocks, elem, wzp_nonzero, head, residual), elem)


def inverted_residual_layers(rng, input_shape, blocks, elem=INT8, wzp_nonzero=False, head=10, residual=False):
    """MobileNetV2/V3-style inverted-residual blocks: input_shape = (H, W, C); blocks = [(expand, K, stride, out), ...], each a
    1x1 Conv2D to `expand` channels (relu6) -> KxK depthwise SAME at `stride` (relu6) -> 1x1 Conv2D to `out` channels (no
    activation); then AveragePool over the whole image, FullyConnected(head) and Softmax.  Per-channel filter quantization; with
    wzp_nonzero every filter zero point (the depthwise ones included) sits off the middle, as in classic asymmetric-u8 models.
    residual: an ADD (no activation) of the block's input behind every block with stride 1 and out == its input channels, as
    MobileNet-v2 has them; without it the bytes are the ones written before ADD existed.  -> build_model's arguments"""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    mid = (lo + hi) // 2
    H, W, C = input_shape
    in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, hi - 20)))
    q, layers = in_q, []

    def conv(dw, n, k, s, act):
        nonlocal q, H, W, C
        oh, ow = -(-H // s), -(-W // s)
        sc = rng.uniform(0.002, 0.01, n).astype(np.float32)
        zp = rng.integers(mid - 12, mid + 13, n) if wzp_nonzero else np.full(n, mid)
        if wzp_nonzero:
            zp[zp == mid] = mid + 5
        taps = k * k * (1 if dw else C)
        osc = float(np.float32(q[0] * float(sc.mean()) * 60.0 * np.sqrt(taps)))
        d = dict(op="depthwise_conv_2d" if dw else "conv_2d", fscale=sc, fzp=zp, bias=rng.integers(-500, 500, n),
                 bscale=(sc * np.float32(q[0])).astype(np.float32), bzp=np.zeros(n, np.int64), padding="same", strides=(s, s), act=act,
                 out_shape=(1, oh, ow, n), out_q=(osc, lo if act == "relu6" else int(rng.integers(lo + 20, hi - 20))))
        d["weights" if dw else "filters"] = rng.integers(lo, hi, (1, k, k, n) if dw else (n, k, k, C))
        layers.append(d)
        q, H, W, C = d["out_q"], oh, ow, n

    for expand, k, s, out in blocks:
        skip, q_skip, c_in = len(layers) - 1, q, C  # the block's input: the layer in front of it (-1: the model input)
        conv(False, expand, 1, 1, "relu6")
        conv(True, expand, k, s, "relu6")
        conv(False, out, 1, 1, "none")
        if residual and s == 1 and out == c_in:
            layers.append(_add_layer(rng, skip, (1, H, W, C), q, q_skip, "none", elem))
            q = layers[-1]["out_q"]
    layers.append(dict(op="average_pool_2d", filter=(H, W), padding="valid", strides=(H, W), act="none", out_shape=(1, 1, 1, C), out_q=q))
    layers.append(dict(op="reshape", out_shape=(1, C), out_q=q))
    wsc = np.float32(rng.uniform(0.002, 0.02))
    osc = float(np.float32(q[0] * wsc * 60.0 * np.sqrt(C)))
    layers.append(dict(op="fully_connected", weights=rng.integers(lo, hi, (head, C)), wscale=[wsc], wzp=[mid],
                       bias=rng.integers(-2000, 2000, head), bscale=[np.float32(q[0]) * wsc], bzp=[0], act="none",
                       out_shape=(1, head), out_q=(osc, int(rng.integers(lo + 20, hi - 20)))))
    layers.append(dict(op="softmax", out_shape=(1, head), out_q=(1.0 / 256.0, lo)))
    return (1,) + tuple(input_shape), in_q, layers


def resnet_like_layers(rng, input_shape, blocks, elem=INT8, k=3, swap=(), head=10, side="first", side_wzp="none", side_act="none",
                       add_act="relu", in_q=None, act_scale=None):
    """ResNet-style basic blocks: input_shape = (H, W, C); `blocks` of them (a count: identity blocks), each Conv2D kxk SAME (relu) ->
    Conv2D kxk SAME (no activation) -> ADD with relu onto the block's input; block b's ADD is written [skip, running] when b is in
    `swap`.  `blocks` may also be a list of (stride, width): the block's first convolution has that stride and both have that many
    outputs; a block with stride 2 or a changed width is a projection block, whose ADD reads a 1x1 Conv2D (that stride, no activation
    unless side_act, filter zero points by side_wzp as _conv_layer's wzp) of the block's input instead of the input itself.  `side`
    places that convolution in file order: "first" (directly behind the fork) or "last" (directly in front of the ADD); the operators
    are the same either way.  act_scale: every convolution's output scale (_conv_layer's act_scale: a deep stack keeps its scales),
    else each layer's own spread-keeping one; in_q: the input's quantisation, where a caller puts a stem in front.  Then AveragePool
    over the whole image, FullyConnected(head) and Softmax (head = 0: none of the three).  -> build_model's arguments"""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    H, W, C = (int(v) for v in input_shape)
    in_q = in_q or (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, hi - 20)))  # (given: the tensor in front)
    q, layers = in_q, []
    plan = [(1, C)] * blocks if isinstance(blocks, int) else [(int(s), int(n)) for s, n in blocks]
    assert side in ("first", "last")
    for b, (s, n) in enumerate(plan):
        skip, q_skip = len(layers) - 1, q
        proj = s != 1 or n != C
        sc = None
        if proj:  # (drawn here wherever it stands: both placements write the same operators)
            sc = dict(_conv_layer(rng, (H, W, C), q, False, n, 1, s, "same", side_act, elem, wzp=side_wzp, act_scale=act_scale), side_of=skip)
        if proj and side == "first":
            layers.append(sc)
        layers.append(_conv_layer(rng, (H, W, C), q, False, n, k, s, "same", "relu", elem, act_scale=act_scale))
        oh, ow = layers[-1]["out_shape"][1:3]
        layers.append(_conv_layer(rng, (oh, ow, n), layers[-1]["out_q"], False, n, k, 1, "same", "none", elem, act_scale=act_scale))
        q_run = layers[-1]["out_q"]
        if proj and side == "last":
            layers.append(sc)
        if proj:
            skip = len(layers) - 1 if side == "last" else skip + 1
            q_skip = sc["out_q"]
        H, W, C = oh, ow, n
        layers.append(_add_layer(rng, skip, (1, H, W, C), q_run, q_skip, add_act, elem, swap=b in swap))
        q = layers[-1]["out_q"]
    if head:
        layers.append(dict(op="average_pool_2d", filter=(H, W), padding="valid", strides=(H, W), act="none", out_shape=(1, 1, 1, C), out_q=q))
        layers.append(dict(op="reshape", out_shape=(1, C), out_q=q))
        layers.append(_fc_layer(rng, C, head, q, "none", elem))
        layers.append(dict(op="softmax", out_shape=(1, head), out_q=(1.0 / 256.0, lo)))
    return (1,) + tuple(int(v) for v in input_shape), in_q, layers


def resnet_like(rng, input_shape, blocks, elem=INT8, **kw):
    return build_model(*resnet_like_layers(rng, input_shape, blocks, elem, **kw), elem)


def resnet8_layers(rng, elem=INT8, side="first", input_shape=(32, 32, 3), widths=(16, 32, 64), head=10):
    """MLPerf-Tiny's image classifier: 32x32x3 -> Conv2D 3x3 to 16 (relu) -> an identity block at 16 -> projection blocks to 32 and to 64
    at stride 2 (1x1 stride-2 convolutions on their shortcuts) -> AveragePool over the 8x8 image -> FullyConnected(10) -> Softmax.
    input_shape / widths: a cut-down twin of the same graph.  -> build_model's arguments"""
    lo = 0 if elem == UINT8 else -128
    H, W, C = (int(v) for v in input_shape)
    in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, lo + 236)))
    stem = _conv_layer(rng, (H, W, C), in_q, False, widths[0], 3, 1, "same", "relu", elem, act_scale=in_q[0])
    blocks = [(1, widths[0])] + [(2, int(n)) for n in widths[1:]]
    _, _, body = resnet_like_layers(rng, (H, W, widths[0]), blocks, elem, head=head, side=side, in_q=stem["out_q"], act_scale=in_q[0])
    for L in body:  # (the body's layer indices are one behind the model's: the stem is layer 0; its "model input" is the stem)
        if "side_of" in L:
            L["side_of"] += 1
        if L["op"] == "add":
            L["skip"] += 1
    return (1, H, W, C), in_q, [stem] + body


def resnet8(rng, elem=INT8, **kw):
    return build_model(*resnet8_layers(rng, elem, **kw), elem)


def _concat_layer(skip, shape, q, swap=False, axis=-1):
    """one CONCATENATION layer dict: the running tensor and the output of layer `skip` (-1: the model input) joined along `axis`
    into `shape` with quantisation q; swap: the skip tensor is input a"""
    return dict(op="concatenation", skip=int(skip), swap=bool(swap), axis=int(axis), out_shape=tuple(int(v) for v in shape),
                out_q=(float(q[0]), int(q[1])))


def fire_layers(rng, shape, q, fire, base=0, elem=INT8, act="relu", e1_first=True, identity=(True, True), side_wzp="none", act_scale=None):
    """One SqueezeNet fire module on a tensor shape = (H, W, C) of quantisation q, whose producer is layer base - 1 of the model:
    fire = (S, E1, E3[, stride[, order]]) -- a squeeze 1x1 Conv2D to S channels, then two expands that both read it, 1x1 to E1 and
    3x3 SAME to E3 channels (both at `stride`, 1 or 2), then the CONCATENATION of the two along the channels.  order: "13" writes the
    1x1 expand first, which makes it the side operator and the 3x3 the main chain; "31" the other way round.  e1_first: the join
    reads [e1, e3], else [e3, e1].  identity = (e1, e3): a slice that carries the join's output quantisation, as the converter
    writes both; a slice that does not gets a scale 0.5 .. 1.4 times the output's.  -> (layers, (H, W, C), q) of the output"""
    S, E1, E3 = (int(v) for v in fire[:3])
    stride = int(fire[3]) if len(fire) > 3 else 1
    order = fire[4] if len(fire) > 4 else "13"
    assert order in ("13", "31")
    H, W, C = (int(v) for v in shape)
    sq = _conv_layer(rng, (H, W, C), q, False, S, 1, 1, "same", act, elem, act_scale=act_scale)
    qs = sq["out_q"]
    e1 = _conv_layer(rng, (H, W, S), qs, False, E1, 1, stride, "same", act, elem, wzp=side_wzp if order == "13" else "none", act_scale=act_scale)
    e3 = _conv_layer(rng, (H, W, S), qs, False, E3, 3, stride, "same", act, elem, wzp=side_wzp if order == "31" else "none", act_scale=act_scale)
    oh, ow = e1["out_shape"][1:3]
    q0 = e1["out_q"]
    for e, same in ((e1, identity[0]), (e3, identity[1])):
        e["out_q"] = q0 if same else (float(np.float32(q0[0] * rng.uniform(0.5, 1.4))), e["out_q"][1])
    qo = q0 if (identity[0] or identity[1]) else (float(np.float32(q0[0] * rng.uniform(0.8, 1.2))), q0[1])
    first, second = (e1, e3) if order == "13" else (e3, e1)
    first["side_of"] = base  # (the squeeze is layer `base`; the first expand in the file is the side operator)
    swap = (order == "13") == bool(e1_first)  # the skip tensor -- the side operator's -- is input a
    cat = _concat_layer(base + 1, (1, oh, ow, E1 + E3), qo, swap=swap)
    return [sq, first, second, cat], (oh, ow, E1 + E3), qo


def fire_net(rng, input_shape, fires, elem=INT8, head=0, in_q=None, **kw):
    """Fire modules one behind the other on input_shape = (H, W, C) (fire_layers' arguments), then, with head, AveragePool over the
    whole image, FullyConnected(head) and Softmax."""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    H, W, C = (int(v) for v in input_shape)
    in_q = in_q or (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, hi - 20)))
    q, layers, shape = in_q, [], (H, W, C)
    for fire in fires:
        ls, shape, q = fire_layers(rng, shape, q, fire, base=len(layers), elem=elem, **kw)
        layers += ls
    if head:
        H2, W2, C2 = shape
        layers.append(dict(op="average_pool_2d", filter=(H2, W2), padding="valid", strides=(H2, W2), act="none", out_shape=(1, 1, 1, C2), out_q=q))
        layers.append(dict(op="reshape", out_shape=(1, C2), out_q=q))
        layers.append(_fc_layer(rng, C2, head, q, "none", elem))
        layers.append(dict(op="softmax", out_shape=(1, head), out_q=(1.0 / 256.0, lo)))
    return build_model((1, H, W, C), in_q, layers, elem)


def dense_net_layers(rng, input_shape, growths, elem=INT8, k=3, swap=(), head=0):
    """DenseNet-style single-level blocks on input_shape = (H, W, C): block b is a Conv2D k x k SAME (relu) to growths[b] channels on
    the block's input x and the CONCATENATION concat(x, conv(x)) -- an identity skip; written [conv(x), x] when b is in `swap`.  The
    join carries x's quantisation, so x's slice is copied and the convolution's is requantised wherever their zero points differ.
    -> build_model's arguments"""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    H, W, C = (int(v) for v in input_shape)
    in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, hi - 20)))
    q, layers = in_q, []
    for b, g in enumerate(growths):
        skip = len(layers) - 1
        layers.append(_conv_layer(rng, (H, W, C), q, False, int(g), k, 1, "same", "relu", elem, act_scale=q[0]))
        C += int(g)
        layers.append(_concat_layer(skip, (1, H, W, C), q, swap=b not in swap))  # (swap: the skip tensor x is input a)
    if head:
        layers.append(dict(op="average_pool_2d", filter=(H, W), padding="valid", strides=(H, W), act="none", out_shape=(1, 1, 1, C), out_q=q))
        layers.append(dict(op="reshape", out_shape=(1, C), out_q=q))
        layers.append(_fc_layer(rng, C, head, q, "none", elem))
        layers.append(dict(op="softmax", out_shape=(1, head), out_q=(1.0 / 256.0, lo)))
    return (1,) + tuple(int(v) for v in input_shape), in_q, layers


def dense_net(rng, input_shape, growths, elem=INT8, **kw):
    return build_model(*dense_net_layers(rng, input_shape, growths, elem, **kw), elem)


def squeezenet_layers(rng, side=64, classes=10, elem=INT8, order="13", fires=None):
    """SqueezeNet 1.1's layer list at a reduced input side x side x 3: Conv2D 3x3 stride 2 to 64 (relu) -> MaxPool 3x3 stride 2 ->
    fires (16,64,64) x 2 -> MaxPool -> (32,128,128) x 2 -> MaxPool -> (48,192,192) x 2, (64,256,256) x 2 -> Conv2D 1x1 to `classes`
    (relu) -> AveragePool over the whole image -> Softmax.  Every convolution carries one output scale (a deep stack keeps its
    scales), so both slices of every join are copies, as in converter-written files.  fires: another list of stages, each a list of
    (S, E1, E3), with a MaxPool behind every stage but the last two.  -> build_model's arguments"""
    lo = 0 if elem == UINT8 else -128
    in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, lo + 236)))
    stages = fires or [[(16, 64, 64)] * 2, [(32, 128, 128)] * 2, [(48, 192, 192)] * 2, [(64, 256, 256)] * 2]
    layers = [_conv_layer(rng, (side, side, 3), in_q, False, 64, 3, 2, "same", "relu", elem, act_scale=in_q[0])]
    q, (H, W, C) = layers[0]["out_q"], layers[0]["out_shape"][1:]

    def pool():
        nonlocal H, W
        H, W = _same_or_valid(H, 3, 2, "valid"), _same_or_valid(W, 3, 2, "valid")
        layers.append(dict(op="max_pool_2d", filter=(3, 3), padding="valid", strides=(2, 2), act="none", out_shape=(1, H, W, C), out_q=q))

    pool()
    for si, stage in enumerate(stages):
        for fire in stage:
            ls, (H, W, C), q = fire_layers(rng, (H, W, C), q, tuple(fire) + (1, order), base=len(layers), elem=elem, act_scale=in_q[0])
            layers += ls
        if si + 2 < len(stages):
            pool()
    layers.append(_conv_layer(rng, (H, W, C), q, False, classes, 1, 1, "same", "relu", elem, act_scale=in_q[0]))
    q = layers[-1]["out_q"]
    layers.append(dict(op="average_pool_2d", filter=(H, W), padding="valid", strides=(H, W), act="none", out_shape=(1, 1, 1, classes), out_q=q))
    layers.append(dict(op="reshape", out_shape=(1, classes), out_q=q))
    layers.append(dict(op="softmax", out_shape=(1, classes), out_q=(1.0 / 256.0, lo)))
    return (1, side, side, 3), in_q, layers


def squeezenet(rng, side=64, classes=10, elem=INT8, **kw):
    return build_model(*squeezenet_layers(rng, side, classes, elem, **kw), elem)


# person_detect_like(quant=...): the head's effective multiplier in_scale * fscale / out_scale (256 products of a byte
# around the zero point with a full-range weight: accumulators of some 1e5, so about +-100 output steps)
HEAD_MULT = 1e-3
PD_SCALES = (0.0235294122, 0.03, 0.02, 0.033, 0.026, 0.0285)


def pd_quant_plan(name, elem=INT8, n_stage=5):
    """The named activation-quantisation plans for person_detect_like(quant=...): one (activation, output scale, output
    zero point) per conv-like layer (0 = the stem, 1 .. 2 (8 + n_stage) = the pairs, the last = the 1x1 head).
      shifted  every tensor (0.03, lo + 7), relu6: every clamp is [lo + 7, lo + 207]
      varied   by layer i: relu6 / relu / none (i % 3), the scale PD_SCALES[i % 6], the zero point lo + (0, 5, 17, 30, 9)[i % 5]
               behind relu / relu6 and mid + (-6, 4, 11)[(i // 3) % 3] behind none (the activation has period 3, so the
               index of the third table advances once per period): the periods 6, 5 and 9 leave no two operators of one
               launch with the same input zero point and clamp
      stage    as varied, but every input of a pair of the 6x6x128 run (the outputs of ops 12 .. 12 + 2 n_stage - 1) has the
               zero point lo + 9 and the run alternates relu6 (at a scale of its own per pair) with relu: relu6 then relu in the even
               pairs, relu then relu6 in the odd ones, so that every pair has its own clamps in one phase or the other
      one_odd  the shipped quantisation, but ops 3, 7, 10, 17, 25 are relu6 at scale 0.03 (upper bound lo + 200)."""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    mid = (lo + hi) // 2
    n = 2 * (8 + n_stage) + 2
    shipped = [("relu6", PD_SCALES[0], lo)] * (n - 1) + [("none", 0.0125187514, mid - 1)]

    def varied(i):
        act = ("relu6", "relu", "none")[i % 3]
        zp = mid + (-6, 4, 11)[(i // 3) % 3] if act == "none" else lo + (0, 5, 17, 30, 9)[i % 5]
        return (act, PD_SCALES[i % 6], zp)

    if name == "shifted":
        return [("relu6", 0.03, lo + 7)] * n
    if name == "varied":
        return [varied(i) for i in range(n)]
    if name == "stage":
        plan = [varied(i) for i in range(n)]
        run_scales = (0.03, 0.033, 0.026, 0.0285, 0.031, 0.0275, 0.0295, 0.0325)
        plan[12] = plan[12][:2] + (lo + 9,)
        for i in range(13, 12 + 2 * n_stage):
            j = (i - 13) // 2   # relu6 in the depthwise operator of the even pairs and the 1x1 one of the odd pairs
            plan[i] = ("relu6", run_scales[j % 8], lo + 9) if (i % 2 == 1) == (j % 2 == 0) else ("relu", PD_SCALES[i % 6], lo + 9)
        return plan
    if name == "one_odd":
        return [("relu6", 0.03, lo) if i in (3, 7, 10, 17, 25) else q for i, q in enumerate(shipped)]
    raise ValueError(name)


def person_detect_like(rng, side=96, width=1.0, elem=INT8, wzp_nonzero=False, n_stage=5, classes=2, wmax=None, quant=None, in_q=None):
    """The layer structure of person_detect.tflite (MobileNet-v1 0.25, grey input: a one-channel 3x3 stride-2 stem, then
    depthwise 3x3 + 1x1 pairs with strides 1 2 1 2 1 2 [1 x n_stage] 2 1, AveragePool2D over what is left, a 1x1 head,
    Reshape, Softmax) at another input size / channel width / run length, with random weights.  Activations keep the
    shipped model's quantization (scale 6/255, zero point = the type's minimum, relu6), weights are per-channel.
    `wmax`: weights within +-wmax of the type's middle (trained networks have small weights; None = the full range, the worst
    case for the accumulator bounds that decide the epilogue form); a dict {layer index: wmax} narrows single layers and scales
    their filter scales up by 128 / wmax, so that their outputs stay as spread as their neighbours'.

    `quant` (a list, or a callable over the index of the conv-like layer: 0 = the stem ... the last = the 1x1 head; see
    pd_quant_plan) gives every conv-like layer its own (activation, output scale, output zero point); the next layer's input
    quantisation follows from it, and the filter scales are today's draws times out_scale / in_scale: every pair keeps the shipped
    path's effective multiplier in_scale * fscale / out_scale, so the tensors stay spread; the stem, whose shipped input scale is
    a third of its output scale, gets three times the shipped one, with which its output reaches both clamp bounds.  The pool
    keeps its input's zero point, and the head's filter scale is one that leaves its output spread.  `in_q` overrides the model's
    input quantisation.  This is how the fused table launches, which exist for side 96 and width 1.0 only, are exercised under
    clamps and zero points the shipped quantisation never has (tests/test_gpu_pd_quant.py, tests/test_pd_quant_host.py).
    With both None the file is what it always was, byte for byte."""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    mid = (lo + hi) // 2
    act_q = (0.0235294122, lo)
    in_q0 = (0.00784313772, mid - 1)
    in_q = in_q0 if in_q is None else (float(np.float32(in_q[0])), int(in_q[1]))
    ch = lambda c: max(4, int(round(c * width / 4.0)) * 4)  # noqa: E731
    layers = []

    def planned(i, act, out_q):  # layer i's (activation, output quantisation)
        if quant is None:
            return act, out_q
        a, s, z = quant(i) if callable(quant) else quant[i]
        return a, (float(np.float32(s)), int(z))

    def conv(op, in_shape, n, k, stride, act, in_scale, out_q, rescale=None):
        _, h, w, c = in_shape
        oh, ow = -(-h // stride), -(-w // stride)
        fan = k * k * (1 if op == "depthwise_conv_2d" else c)
        sc = (rng.uniform(0.6, 1.4, n) * 2.2 / (74.0 * np.sqrt(fan))).astype(np.float32)   # keeps the activations spread
        wm = wmax.get(len(layers)) if isinstance(wmax, dict) else wmax
        if isinstance(wmax, dict) and wm is not None:   # (narrower weights, the same spread of the outputs)
            rescale = (rescale or 1.0) * 128.0 / wm
        if rescale is not None:
            sc = (sc * np.float32(rescale)).astype(np.float32)
        zp = rng.integers(mid - 12, mid + 12, n) if wzp_nonzero else np.full(n, mid)
        shape = (n, k, k, c) if op == "conv_2d" else (1, k, k, n)
        d = dict(op=op, fscale=sc, fzp=zp, bias=rng.integers(-300, 300, n), bscale=(sc * np.float32(in_scale)).astype(np.float32),
                 bzp=np.zeros(n, np.int64), padding="same", strides=(stride, stride), act=act, out_shape=(1, oh, ow, n), out_q=out_q)
        d["filters" if op == "conv_2d" else "weights"] = rng.integers(lo, hi, shape) if wm is None else rng.integers(mid - wm, mid + wm + 1, shape)
        layers.append(d)
        return d["out_shape"]

    def layer(op, in_shape, n, k, stride, cur, shipped_in_scale):
        act, out_q = planned(len(layers), "relu6", act_q)
        rescale = None
        if quant is not None:   # today's draw times out_scale / in_scale
            rescale = out_q[0] / cur[0]
        elif cur[0] != shipped_in_scale:   # (in_q alone: the shipped multiplier in_scale * fscale / out_scale)
            rescale = shipped_in_scale / cur[0]
        return conv(op, in_shape, n, k, stride, act, cur[0], out_q, rescale), out_q

    shp, cur = layer("depthwise_conv_2d", (1, side, side, 1), ch(8), 3, 2, in_q, in_q0[0])
    plan = [(1, 16), (2, 32), (1, 32), (2, 64), (1, 64), (2, 128)] + [(1, 128)] * n_stage + [(2, 256), (1, 256)]
    for stride, n in plan:
        shp, cur = layer("depthwise_conv_2d", shp, shp[3], 3, stride, cur, act_q[0])
        shp, cur = layer("conv_2d", shp, ch(n), 1, 1, cur, act_q[0])
    pool_q = (0.0186093301, lo)
    if quant is not None:
        pool_q = (float(np.float32(cur[0] * (0.0186093301 / 0.0235294122))), cur[1])
    layers.append(dict(op="average_pool_2d", filter=(shp[1], shp[2]), padding="valid", strides=(2, 2), act="none",
                       out_shape=(1, 1, 1, shp[3]), out_q=pool_q))
    shp = (1, 1, 1, shp[3])
    head_act, head_q = planned(len(layers) - 1, "none", (0.0125187514, mid - 1))
    # (0.002 saturates the head on random weights; the quant path's scale leaves its accumulators a few dozen output steps wide)
    head_fs = 0.002 if quant is None else HEAD_MULT * head_q[0] / pool_q[0]
    sc = (rng.uniform(0.6, 1.4, classes) * head_fs).astype(np.float32)
    zp = rng.integers(mid - 12, mid + 12, classes) if wzp_nonzero else np.full(classes, mid)
    layers.append(dict(op="conv_2d", filters=rng.integers(lo, hi, (classes, 1, 1, shp[3])), fscale=sc, fzp=zp,
                       bias=rng.integers(-300, 300, classes), bscale=(sc * np.float32(pool_q[0])).astype(np.float32),
                       bzp=np.zeros(classes, np.int64), padding="same", strides=(1, 1), act=head_act,
                       out_shape=(1, 1, 1, classes), out_q=head_q))
    layers.append(dict(op="reshape", out_shape=(1, classes), out_q=head_q))
    layers.append(dict(op="softmax", out_shape=(1, classes), out_q=(1.0 / 256.0, lo)))
    return build_model((1, side, side, 1), in_q, layers, elem)


def stack_layers(rng, input_shape, segments, elem=INT8, wzp="none", act_scale=None):
    """A model written segment by segment, for compositions no generator above has; -> (input shape, input quantisation, layer
    dicts), what build_model takes.  input_shape = (H, W, C); a segment is one of
        ("conv", N, K, stride, padding="same", act="relu6")     Conv2D K x K
        ("dw", K, stride, act="relu6")                          depthwise K x K SAME
        ("avgpool" | "maxpool", window, stride, padding="valid")  the pool (window: one side, or (h, w))
        ("gap",)                                                AveragePool2D over the whole image + Reshape to (1, C)
        ("flatten",)                                            Reshape to (1, H W C)
        ("fc", N, act="none")                                   FullyConnected, one row
        ("softmax",)
    Per-channel filter quantisation, per-tensor FullyConnected; conv_net's output scales, or its act_scale form (every activation
    tensor at that scale) with act_scale; the output zero point behind relu / relu6 is the type's minimum; a pool keeps its input's
    quantisation.  A Conv2D directly followed by a pool is conv_pool_layers' stage (without act_scale, which that form does not have).
    wzp: "none"; "conv" -- Conv2D filter zero points off the middle; "all" -- depthwise and FullyConnected ones too, as
    inverted_residual_net(wzp_nonzero=True) and mlp(wzp_nonzero=True) draw them."""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    if wzp not in ("none", "conv", "all"):
        raise ValueError(wzp)
    H, W, C = (int(v) for v in input_shape)
    in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, hi - 20)))
    if act_scale is not None:
        in_q = (float(np.float32(act_scale)), in_q[1])
    q, layers, flat = in_q, [], None       # flat: the row length once the tensor is [1, K]
    segs = [tuple(s) for s in segments]

    def pool_args(seg):
        kind, window, stride = seg[:3]
        return (window, window) if np.isscalar(window) else tuple(window), int(stride), seg[3] if len(seg) > 3 else "valid"

    def image():
        if flat is not None:
            raise ValueError("a %s segment behind a flatten / gap" % segs[i][0])

    i = 0
    while i < len(segs):
        seg = segs[i]
        kind = seg[0]
        nxt = segs[i + 1] if i + 1 < len(segs) else None
        if kind == "conv":
            image()
            n, k, stride = seg[1:4]
            padding, act = (seg[4] if len(seg) > 4 else "same"), (seg[5] if len(seg) > 5 else "relu6")
            if nxt and nxt[0] in ("avgpool", "maxpool") and act_scale is None:
                window, pstride, ppad = pool_args(nxt)
                stage, (H, W, C), q = conv_pool_layers(rng, (H, W, C), q, int(n), int(k), stride=int(stride), padding=padding, act=act, pool=window,
                                                       pool_stride=pstride, pool_padding=ppad, elem=elem, wzp_nonzero=wzp != "none",
                                                       pool_op=nxt[0][:3])
                layers += stage
                i += 2
                continue
            d = _conv_layer(rng, (H, W, C), q, False, n, int(k), int(stride), padding, act, elem, wzp, act_scale=act_scale)
            layers.append(d)
            q, (_, H, W, C) = d["out_q"], d["out_shape"]
        elif kind == "dw":
            image()
            k, stride = seg[1:3]
            d = _conv_layer(rng, (H, W, C), q, True, C, int(k), int(stride), "same", seg[3] if len(seg) > 3 else "relu6", elem,
                            wzp if wzp == "all" else "none", act_scale=act_scale)
            layers.append(d)
            q, (_, H, W, C) = d["out_q"], d["out_shape"]
        elif kind in ("avgpool", "maxpool"):
            image()
            window, stride, padding = pool_args(seg)
            oh, ow = _same_or_valid(H, window[0], stride, padding), _same_or_valid(W, window[1], stride, padding)
            layers.append(dict(op={"avgpool": "average_pool_2d", "maxpool": "max_pool_2d"}[kind], filter=window, padding=padding,
                               strides=(stride, stride), act="none", out_shape=(1, oh, ow, C), out_q=q))
            H, W = oh, ow
        elif kind == "gap":
            image()
            layers.append(dict(op="average_pool_2d", filter=(H, W), padding="valid", strides=(H, W), act="none", out_shape=(1, 1, 1, C), out_q=q))
            layers.append(dict(op="reshape", out_shape=(1, C), out_q=q))
            H, W, flat = 1, 1, C
        elif kind == "flatten":
            image()
            flat = H * W * C
            layers.append(dict(op="reshape", out_shape=(1, flat), out_q=q))
        elif kind == "fc":
            if flat is None:
                raise ValueError("an fc segment needs a flatten or a gap in front of it")
            off = (int(rng.integers(-20, 21)) or 7) if wzp == "all" else 0
            d = _fc_layer(rng, flat, int(seg[1]), q, seg[2] if len(seg) > 2 else "none", elem, off)
            layers.append(d)
            q, flat = d["out_q"], int(seg[1])
        elif kind == "softmax":
            if flat is None:
                raise ValueError("a softmax segment needs a flatten or a gap in front of it")
            layers.append(dict(op="softmax", out_shape=(1, flat), out_q=(1.0 / 256.0, lo)))
            q = layers[-1]["out_q"]
        else:
            raise ValueError(kind)
        if min(H, W) < 1:
            raise ValueError("segment %d (%s) leaves no pixel" % (i, kind))
        i += 1
    return (1,) + tuple(int(v) for v in input_shape), in_q, layers


def stack(rng, input_shape, segments, elem=INT8, wzp="none", act_scale=None):
    """stack_layers' model as a flatbuffer"""
    in_shape, in_q, layers = stack_layers(rng, input_shape, segments, elem, wzp, act_scale)
    return build_model(in_shape, in_q, layers, elem)


def _pad_layer(shape, q, pads):
    """one PAD layer dict on a tensor shape = (H, W, C) of quantisation q (which its output keeps); pads ((top, bottom), (left, right))"""
    H, W, C = (int(v) for v in shape)
    (t, b), (l, r) = pads
    return dict(op="pad", pads=((int(t), int(b)), (int(l), int(r))), out_shape=(1, H + t + b, W + l + r, C), out_q=q)


def keras_pad_for(size, k, stride):
    """the ZeroPadding2D Keras' MobileNets write in front of a stride-2 k x k VALID convolution (correct_pad): (k // 2 - 1, k // 2) on
    an even side, (k // 2, k // 2) on an odd one"""
    return (k // 2 - (1 - size % 2), k // 2)


def keras_mobilenet_v2_layers(rng, side=32, width=0.25, elem=INT8, classes=10, blocks=None, keep_dims=False, wzp="none", last=None):
    """MobileNet-v2 as the TFLite converter writes it from Keras: the 3x3 stride-2 stem and every stride-2 depthwise as
    ZeroPadding2D (PAD) + a VALID convolution, stride-1 depthwise SAME, an ADD behind every stride-1 block that keeps its channel
    count, a 1x1 Conv2D, GlobalAveragePooling2D as MEAN over {1, 2}, FullyConnected and Softmax.  blocks = [(t, c, n, s), ...] as in
    the paper (expansion, channels at width 1, repeats, first stride); the default is the paper's, cut where the image reaches one
    pixel.  Channels are c * width rounded to a multiple of 8 (at least 8); last: the channels of the 1x1 in front of the pool (the
    paper's 1280, which widths below 1 keep).  -> build_model's arguments"""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    mid = (lo + hi) // 2
    if blocks is None:
        blocks = [(1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1)]

    def ch(c):
        return max(8, int(c * width + 4) // 8 * 8)

    H = W = int(side)
    C = 3
    in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, hi - 20)))
    q, layers = in_q, []

    def conv(dw, n, k, s, act):
        nonlocal q, H, W, C
        if s == 2:  # Keras: ZeroPadding2D + VALID
            pt, pl = keras_pad_for(H, k, s), keras_pad_for(W, k, s)
            layers.append(_pad_layer((H, W, C), q, (pt, pl)))
            H, W = H + sum(pt), W + sum(pl)
        d = _conv_layer(rng, (H, W, C), q, dw, n, k, s, "valid" if s == 2 else "same", act, elem, wzp)
        layers.append(d)
        q, (_, H, W, C) = d["out_q"], d["out_shape"]

    conv(False, ch(32), 3, 2, "relu6")
    for t, c, n, s in blocks:
        for r in range(n):
            stride = s if r == 0 else 1
            if stride == 2 and min(H, W) < 2:
                stride = 1
            skip, q_skip, c_in = len(layers) - 1, q, C
            if t != 1:
                conv(False, c_in * t, 1, 1, "relu6")
            conv(True, C, 3, stride, "relu6")
            conv(False, ch(c), 1, 1, "none")
            if stride == 1 and C == c_in:
                layers.append(_add_layer(rng, skip, (1, H, W, C), q, q_skip, "none", elem))
                q = layers[-1]["out_q"]
    conv(False, int(last) if last else (ch(1280) if width > 1.0 else 1280), 1, 1, "relu6")
    layers.append(dict(op="mean", keep_dims=bool(keep_dims), out_shape=(1, 1, 1, C) if keep_dims else (1, C), out_q=q))
    if keep_dims:
        layers.append(dict(op="reshape", out_shape=(1, C), out_q=q))
    layers.append(_fc_layer(rng, C, int(classes), q, "none", elem))
    layers.append(dict(op="softmax", out_shape=(1, int(classes)), out_q=(1.0 / 256.0, lo)))
    return (1, int(side), int(side), 3), in_q, layers


def keras_mobilenet_v2(rng, side=32, width=0.25, elem=INT8, **kw):
    """keras_mobilenet_v2_layers' model as a flatbuffer"""
    in_shape, in_q, layers = keras_mobilenet_v2_layers(rng, side, width, elem, **kw)
    return build_model(in_shape, in_q, layers, elem)


def keras_resnet_stem_layers(rng, side=32, elem=INT8, filters=64):
    """The stem of Keras' ResNets: ZeroPadding2D(3) + Conv2D 7x7 stride 2 VALID (relu) + ZeroPadding2D(1) + MaxPool2D 3x3 stride 2
    VALID, on a side x side x 3 image.  -> build_model's arguments"""
    lo, hi = (0, 256) if elem == UINT8 else (-128, 128)
    in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, hi - 20)))
    H = W = int(side)
    layers = [_pad_layer((H, W, 3), in_q, ((3, 3), (3, 3)))]
    d = _conv_layer(rng, (H + 6, W + 6, 3), in_q, False, int(filters), 7, 2, "valid", "relu", elem)
    layers.append(d)
    q, (_, H, W, C) = d["out_q"], d["out_shape"]
    layers.append(_pad_layer((H, W, C), q, ((1, 1), (1, 1))))
    oh, ow = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    layers.append(dict(op="max_pool_2d", filter=(3, 3), padding="valid", strides=(2, 2), act="none", out_shape=(1, oh, ow, C), out_q=q))
    return (1, int(side), int(side), 3), in_q, layers


def keras_resnet_stem(rng, side=32, elem=INT8, **kw):
    """keras_resnet_stem_layers' model as a flatbuffer"""
    in_shape, in_q, layers = keras_resnet_stem_layers(rng, side, elem, **kw)
    return build_model(in_shape, in_q, layers, elem)
