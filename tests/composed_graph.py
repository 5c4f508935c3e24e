"""Graph models -- chains with skip edges, side operators, PAD, MEAN, TRANSPOSE_CONV, dilated and grouped convolutions, resizes -- for the
composition suite: the cases of tests/composed.py's shape (its Case, with tests/graph_ref.interpret as interpreter), written with
tools/tflite_writer.stack_layers' graph segments.  Shared by tests/test_composed_graph_host.py (no GPU) and
tests/test_gpu_composed_graph.py, which runs tests/test_gpu_composed.py's checks over every one of them.

What the family tests leave to a composition is the run loop's buffer choice (csrc/model.cpp run_step: fork[0] / fork[1], the side
operator's buffer, final_dst and the f32 exit at a join, input_skip), the splits that keep a fork tensor out of every group
(csrc/model_groups.cpp) and the fork buffers' size (csrc/tflite.cpp parse_join: max_fork_elems).  A curated join is built from the
smallest shape at which its family's own test file asserts the routing, named in its comment; `expect` prefixes are the ones a family
test asserts, an entry without one checks bytes only."""
import numpy as np

from tests import composed as C
from tests import graph_ref

I8, U8, FUSED, ACT6 = C.I8, C.U8, C.FUSED, C.ACT6
FUSED_SIDE = {"add": "(fused into its ADD)", "concatenation": "(fused into its CONCATENATION)"}
KIND = dict(C.KIND, add=0, concatenation=2, pad=34, mean=40, transpose_conv=67, resize_nearest_neighbor=97)


def Case(name, shape, segments, **kw):
    return C.Case(name, shape, segments, interpreter=graph_ref.interpret, **kw)


def _both(name, shape, segments, seeds, **kw):
    """the case in both element types"""
    return [Case(name + "-i8", shape, segments, seed=seeds[0], **kw), Case(name + "-u8", shape, segments, elem=U8, seed=seeds[1], **kw)]


def _res(name, swap=False):
    """an identity residual block behind the mark `name` (test_gpu_residual's "resnet": 3x3 relu, 3x3, ADD relu)"""
    return [("mark", name), ("conv", 16, 3, 1, "same", "relu"), ("conv", 16, 3, 1, "same", "none"), ("add", name, "relu", dict(swap=swap))]


def _side(name, opts, stride, join, src="input"):
    """a side Conv2D `opts` from `src`, a 3x3 main convolution at the same stride, and the join (test_gpu_resnext's side_add form)"""
    k = 3 if "dilation" in opts else 1
    stem = [] if src == "input" else [("conv", 16, 3, 1, "same", "relu"), ("mark", src)]
    tail = [("add", src, "relu")] if join == "add" else [("concat", src)]
    return Case("side-%s-%s" % (name, join), (12, 12, 16), stem + [("side", src, 16, k, stride, "same", "none", opts), ("conv", 16, 3, stride, "same", "none")] + tail,
                seed={"add": 60, "concat": 70}[join] + len(name))


JOINS = (
    # 1. fork-inside-pair: test_gpu_pair_band's chain_rt pair (depthwise 3x3 + 1x1 on 12x12x64; N = 64 so that the ADD has one shape) with
    #    the depthwise output marked: model_groups.cpp's split keeps the fork tensor out of the pair, so no chain_rt anywhere.  -input:
    #    the same model with the model input as skip, where the pair may form (input_skip: no f32 entry)
    [Case("fork-inside-pair", (12, 12, 64), [("dw", 3, 1), ("mark", "d"), ("conv", 64, 1, 1, "same", "none"), ("add", "d", "none")], seed=31, never=("chain_rt<",)),
     Case("fork-inside-pair-input", (12, 12, 64), [("dw", 3, 1), ("conv", 64, 1, 1, "same", "none"), ("add", "input", "none")], seed=32)]
    # 2. join-feeds-join: test_gpu_residual's "resnet" blocks (8x8x16) behind a stem, three in a row: each ADD's result is the next skip,
    #    so run_step's `forks` destination alternates fork[0], fork[1], fork[0]; -swap: the middle ADD reads [skip, running]
    + _both("join-feeds-join", (8, 8, 16), [("conv", 16, 3, 1, "same", "relu")] + _res("a") + _res("b") + _res("c"), seeds=(33, 553))
    + [Case("join-feeds-join-swap", (8, 8, 16), [("conv", 16, 3, 1, "same", "relu")] + _res("a") + _res("b", True) + _res("c"), seed=34)]
    # 3. concat-of-join: a CONCATENATION whose skip is an ADD's result, then an ADD whose skip is that CONCATENATION's result (test_gpu_concat's
    #    dense block on the residual block's 8x8x16)
    + _both("concat-of-join", (8, 8, 16), [("conv", 16, 3, 1, "same", "relu")] + _res("a") + [("mark", "b"), ("conv", 8, 3, 1, "same", "relu"), ("concat", "b"),
                                           ("mark", "c"), ("conv", 24, 3, 1, "same", "none"), ("add", "c", "relu")], seeds=(95, 555))
    # 4. large-fork: the fork tensor is a resize / TRANSPOSE_CONV output, larger than anything in front of it (parse_join: max_fork_elems
    #    from the skip tensor's own size).  test_gpu_upconv's unet1 widths on its 16x16 image, the factor 4 from a 4x4 one
    + [Case("large-fork-resize2", (16, 16, 4), [("conv", 8, 3, 2, "same", "relu"), ("resize", 2, 2), ("mark", "r"), ("conv", 8, 3, 1, "same", "relu"),
                                                ("conv", 8, 3, 1, "same", "relu"), ("concat", "r"), ("conv", 4, 3, 1, "same", "none")], seed=36),
       Case("large-fork-resize4", (8, 8, 8), [("conv", 8, 3, 2, "same", "relu"), ("resize", 4, 4), ("mark", "r"), ("conv", 8, 3, 1, "same", "relu"),
                                              ("conv", 8, 3, 1, "same", "relu"), ("concat", "r", dict(swap=True)), ("conv", 4, 3, 1, "same", "none")], elem=U8, seed=37),
       Case("large-fork-tconv", (8, 8, 8), [("tconv", 16, 3, 2), ("mark", "t"), ("conv", 8, 3, 1, "same", "relu"), ("conv", 8, 3, 1, "same", "relu"),
                                            ("concat", "t"), ("conv", 4, 3, 1, "same", "none")], seed=38)]
    # 5. resize-group-split: resize x4 + Conv2D 3x3 on 4x4x16, the stage of test_gpu_upconv's autoencoder-x4 for which rule (0r) forms
    #    resize+upconv_rt<4x4>.  With the resize output marked and read by a later concat the group must not form; -control: no mark
    + [Case("resize-group-split", (4, 4, 16), [("resize", 4, 4), ("mark", "r"), ("conv", 8, 3, 1, "same", "relu"), ("concat", "r"), ("conv", 4, 3, 1, "same", "none")],
            seed=39, never=("resize+",)),
       Case("resize-group-control", (4, 4, 16), [("resize", 4, 4), ("conv", 8, 3, 1, "same", "relu"), ("conv", 4, 3, 1, "same", "none")],
            seed=60, expect=[(0, "resize+upconv_rt<4x4>")])]
    # 6. input-skip-f32: TRANSPOSE_CONV stride 2 (test_gpu_tconv's autoencoder stage), AveragePool 2x2 back down, ADD with the model input:
    #    input_skip is set, so predict takes the quantise launch (f32_entry: none); the run ends at the join (final_dst, no f32 exit)
    + _both("input-skip-f32", (8, 8, 8), [("tconv", 8, 3, 2), ("avgpool", 2, 2), ("add", "input", "none")], seeds=(41, 561))
    # 7. side-variants: a grouped side Conv2D (G = 4, test_gpu_resnext's side_add on 12x12x16), a dilated 3x3 one (test_gpu_tcn's pass-by
    #    factors 3 x 3) and a stride-2 one under a stride-2 main path (test_gpu_resnet8's projection), each joined by ADD and by
    #    CONCATENATION; the last two from a stem's output instead of the model input
    + [_side("grouped", dict(groups=4), 1, j) for j in ("add", "concat")]
    + [_side("dilated", dict(dilation=(3, 3)), 1, j, "s") for j in ("add", "concat")]
    + [_side("stride2", {}, 2, j, "s") for j in ("add", "concat")]
    # 8. side-concat-into-fork: a side operator joined by a CONCATENATION whose own result is marked for a later ADD: the join writes a
    #    fork buffer, which is the one run_step would give the side operator's result (`s_buf == dst`).  A 3x3 side (test_gpu_squeezenet's
    #    "31" order: no fused side_concat launch) and a 1x1 one
    + [Case("side3-concat-into-fork", (8, 8, 16), [("conv", 16, 3, 1, "same", "relu"), ("mark", "a"), ("side", "a", 8, 3, 1, "same", "relu"), ("conv", 16, 1, 1, "same", "relu"),
                                                   ("concat", "a"), ("mark", "b"), ("conv", 24, 3, 1, "same", "none"), ("add", "b", "relu")], seed=42),
       Case("side1-concat-into-fork", (8, 8, 16), [("conv", 16, 3, 1, "same", "relu"), ("mark", "a"), ("conv", 16, 3, 1, "same", "relu"), ("conv", 16, 1, 1, "same", "relu"),
                                                   ("side", "a", 8, 1, 1, "same", "relu"), ("concat", "a", dict(swap=True)), ("mark", "b"), ("conv", 24, 3, 1, "same", "none"), ("add", "b", "relu")], elem=U8, seed=43)]
    # 9. pad-dilated-maxpool: test_gpu_tcn's block at d = 4 (40 steps of 16 channels, causal PAD of 8, 1x3 VALID: pad+conv_dil_rt<d1x4>),
    #    then MaxPool2D, MEAN and FullyConnected
    + [Case("pad-dilated-maxpool", (1, 40, 16), [("pad", ((0, 0), (8, 0))), ("conv", 16, (1, 3), 1, "valid", "relu", dict(dilation=(1, 4))), ("maxpool", (1, 2), 2),
                                                 ("mean",), ("fc", 6)], seed=44, expect=[(0, "pad+conv_dil_rt<d1x4>")])]
    # 10. grouped-behind-concat: test_gpu_squeezenet's smallest fire (16, 64, 64; the 1x1 expand the side operator: side_concat_rt), a
    #     grouped 3x3 Conv2D with G = 2 over the joined channels, gap + fc + softmax.  u8.  On 4x4x32
    + [Case("grouped-behind-concat", (4, 4, 32), [("conv", 16, 1, 1, "same", "relu"), ("mark", "s"), ("side", "s", 64, 1, 1, "same", "relu"), ("conv", 64, 3, 1, "same", "relu"),
                                                  ("concat", "s", dict(swap=True)), ("conv", 32, 3, 1, "same", "relu", dict(groups=2)), ("gap",), ("fc", 10), ("softmax",)],
            elem=U8, seed=45, expect=[(1, FUSED_SIDE["concatenation"]), (3, "side_concat_rt<16,64,64>")])]
    # 11. ends-at-side / ends-at-join: the last operator is a join with its side operator directly in front of it (the every-operator sweep
    #     ends at the side operator too), and a join of an identity skip
    + [Case("ends-at-side-add", (8, 8, 16), [("conv", 16, 3, 1, "same", "relu"), ("mark", "a"), ("conv", 32, 3, 2, "same", "relu"), ("conv", 32, 3, 1, "same", "none"),
                                             ("side", "a", 32, 1, 2), ("add", "a", "relu")], seed=46),
       Case("ends-at-side-concat", (8, 8, 16), [("conv", 16, 3, 1, "same", "relu"), ("mark", "a"), ("conv", 16, 3, 1, "same", "relu"), ("conv", 16, 1, 1, "same", "relu"), ("side", "a", 8, 1, 1, "same", "relu"),
                                                ("concat", "a")], elem=U8, seed=47),
       Case("ends-at-join-concat", (8, 8, 16), [("conv", 16, 3, 1, "same", "relu"), ("mark", "a"), ("conv", 8, 3, 1, "same", "relu"), ("concat", "a", dict(swap=True))], seed=48)]
)
BY_NAME = {c.name: c for c in JOINS}
assert len(BY_NAME) == len(JOINS)

# ---- the grammar -------------------------------------------------------------------------------------------------------------------
# 24 of the first 200 seeds: among those whose expected tensors meet tests/test_composed_host.py's spread condition with room to spare
# (at least 10 distinct values, at most 70 % at the ends), the ones with joins that together cover what
# tests/test_composed_graph_host.py lists; chosen on the CPU from the reference alone.  A seed that saturates is swapped for another
# seed, the bound stays
SEEDS = (20, 21, 23, 24, 25, 27, 28, 37, 55, 65, 72, 76, 99, 106, 107, 119, 148, 156, 162, 184, 186, 193, 195, 199)

_grammar = {}


def graph_grammar(seed):
    """a seeded random graph: an image of at most 16 x 16 with a channel count of composed.CHANNELS; 3 .. 8 operators of
    composed.grammar's vocabulary plus dilated and grouped convolutions, TRANSPOSE_CONV, resize, PAD and joins; at most one skip alive at a
    time (a new mark only once the last one is joined: tflite.cpp parse_join's liveness refusals), every marked tensor joined exactly once
    ("a fork tensor is used twice"), at most one side Conv2D per join; one of composed.grammar's four endings (MEAN in place of the global
    pool for some); a random element type and zero-point mode.  Never what the parser refuses: joins have equal shapes (ADD) or equal
    images (CONCATENATION), PAD pads rows and columns only, resizes have integer factors; and no image grows beyond 16 x 16"""
    if seed in _grammar:
        return _grammar[seed]
    rng = np.random.default_rng(737300 + seed)
    h, w, c = int(rng.integers(4, 13)), int(rng.integers(4, 13)), int(rng.choice(C.CHANNELS[2:]))
    shape, segs = (h, w, c), []
    n_ops = int(rng.integers(3, 9))
    mark = ("input", (h, w, c)) if rng.integers(0, 3) == 0 else None      # the live skip: (name, its shape)
    n_marks, ops, since = 0, 0, 0                                          # since: main operators behind the mark (a join needs one: no tensor joins itself)

    def conv_to(n, k, stride, act, opts=None):
        nonlocal h, w, c
        segs.append(("conv", n, k, stride, "same", act) + ((opts,) if opts else ()))
        h, w, c = -(-h // stride), -(-w // stride), n

    def new_mark():
        nonlocal mark, n_marks, since
        n_marks += 1
        mark, since = ("m%d" % n_marks, (h, w, c)), 0
        segs.append(("mark", mark[0]))

    while ops < n_ops:
        if mark is not None and since >= 1 and rng.integers(0, 2):        # close the skip
            name, (mh, mw, mc) = mark
            join = str(rng.choice(["add", "concat"]))
            stride = 1 if (h, w) == (mh, mw) else 2                        # (the main path strode once: only a side operator at that stride can follow)
            side = stride == 2 or bool(rng.integers(0, 2))
            n = c if join == "add" else int(rng.choice(C.CHANNELS[2:6]))
            if side:
                kind = int(rng.integers(0, 3))
                opts = dict(groups=2) if kind == 1 else dict(dilation=(2, 2)) if kind == 2 and stride == 1 else {}
                seg = ("side", name, n, 3 if "dilation" in opts else 1, stride, "same", str(rng.choice(["none", "relu"])), opts)
                # in front of the join, or directly behind the fork.  (Behind a single main operator the parser could not tell the two
                # apart: of two operators that read the fork tensor and that only the join reads, the first in the file is the side one)
                at = len(segs) if since >= 2 and rng.integers(0, 2) else 0 if name == "input" else segs.index(("mark", name)) + 1
                segs.insert(at, seg)
                ops += 1
            elif join == "add" and c != mc:
                conv_to(mc, 1, 1, "none")
                ops += 1
            swap = dict(swap=bool(rng.integers(0, 2)))
            segs.append(("add", name, str(rng.choice(["none", "relu"])), swap) if join == "add" else ("concat", name, swap))
            if join == "concat":
                c += n if side else mc
            ops += 1
            mark = None
            if rng.integers(0, 2):                                        # the join's result is the next skip
                new_mark()
            continue
        if mark is None and segs and rng.integers(0, 3) == 0:
            new_mark()
            continue
        small = min(h, w) < 4
        strode = mark is not None and (h, w) != mark[1][:2]
        kinds = ["conv", "conv", "dil", "grp", "dw", "dwdil"] + ([] if small else ["avgpool", "maxpool"])
        if mark is None:                                                   # (what changes the image otherwise than by one stride of 2: no join could follow)
            kinds += ["pad"] + (["tconv", "resize"] if max(h, w) <= 8 else [])
        kind = str(rng.choice(kinds))
        stride = 1 if small or strode else int(rng.integers(1, 3))
        act = str(rng.choice(["relu6", "relu", "none"], p=[0.5, 0.3, 0.2]))
        if kind == "conv":
            conv_to(int(rng.choice(C.CHANNELS[2:])), int(rng.choice([k for k in (1, 3, 5) if k <= min(h, w)])), stride, act)
        elif kind == "dil":
            conv_to(int(rng.choice(C.CHANNELS[2:])), 3, 1, act, dict(dilation=(int(rng.integers(1, 4)), int(rng.integers(2, 4)))))
        elif kind == "grp":
            conv_to(int(rng.choice([8, 16, 32])), int(rng.choice([1, 3])), stride, act, dict(groups=int(rng.choice([2, 4]))))
        elif kind == "dwdil":
            segs.append(("dw", 3, 1, "relu6", dict(dilation=(2, 2))))
        elif kind == "dw":
            segs.append(("dw", int(rng.choice([3, 5])), stride, "relu6"))
            h, w = -(-h // stride), -(-w // stride)
        elif kind == "pad":
            pads = ((int(rng.integers(0, 3)), int(rng.integers(0, 3))), (int(rng.integers(0, 3)), int(rng.integers(1, 3))))
            if max(h + sum(pads[0]), w + sum(pads[1])) > 16:
                continue
            segs.append(("pad", pads))
            h, w = h + sum(pads[0]), w + sum(pads[1])
        elif kind in ("avgpool", "maxpool"):
            segs.append((kind, int(rng.choice([2, 3])), stride, "same"))
            h, w = -(-h // stride), -(-w // stride)
        elif kind == "tconv":
            n, s = int(rng.choice(C.CHANNELS[2:6])), int(rng.integers(1, 3))
            segs.append(("tconv", n, int(rng.choice([2, 3])), s, "same", str(rng.choice(["relu", "none"]))))
            h, w, c = h * s, w * s, n
        else:
            sy, sx = int(rng.integers(1, 3)), 2
            segs.append(("resize", sy, sx))
            h, w = h * sy, w * sx
        ops, since = ops + 1, since + 1
    joined = {s[1] for s in segs if s[0] in ("add", "concat")}
    segs = [s for s in segs if s[0] != "mark" or s[1] in joined]          # (a mark that no join reads is no fork)
    ending = int(rng.integers(0, 4))
    if ending == 0:
        segs.append(("mean",) if rng.integers(0, 2) else ("gap",))
        if rng.integers(0, 2):
            segs.append(("fc", int(rng.choice([16, 32, 40])), "relu"))
        segs.append(("fc", int(rng.integers(6, 13))))
        if rng.integers(0, 2):
            segs.append(("softmax",))
    elif ending == 1:
        segs += [("flatten",), ("fc", int(rng.integers(6, 13)))]
        if rng.integers(0, 2):
            segs.append(("softmax",))
    elif ending == 2:
        segs += [("avgpool", (h, w), max(h, w)), ("conv", 8, 1, 1, "same", "none"), ("flatten",), ("softmax",)]
    elem = U8 if rng.integers(0, 2) else I8
    wzp = str(rng.choice(["none", "conv", "all"]))
    _grammar[seed] = Case("gg%02d" % seed, shape, segs, elem=elem, wzp=wzp, act_scale=ACT6 if n_ops >= 5 else None, seed=7000 + seed)
    return _grammar[seed]


def cases():
    """every curated join and every seed's graph"""
    return JOINS + [graph_grammar(s) for s in SEEDS]
