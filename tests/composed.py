"""Models that join fused-group families (tools/tflite_writer.stack_layers), and every operator's expected tensor.

The grouping rules (csrc/model_groups.cpp) each see what the earlier ones took, and the run loop (csrc/model.cpp: stage_at / group_at /
launch_at) picks a stage, a group or the operator's own launch at every operator -- again, differently, for a run that ends inside a
group.  The family test files write one family per model; JOINS writes the compositions, grammar(seed) random ones.  Shared by
tests/test_composed_host.py (no GPU: the writer, the parser, the spread of the expected tensors) and tests/test_gpu_composed.py.

A join is built from the smallest shapes at which its family's own test file asserts the routing; where the tensor between two families
forces another shape the case's comment says which.  `expect` lists (operator index, kernel-name prefix) under default routing; a
CONTESTED join, where two rules may legitimately claim the same operators, has `outcomes` instead: dicts {operator index: prefix}, of
which the report must show one.  `never`: prefixes no operator may report."""
import os
import sys

import numpy as np

from tests import maxpool_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

I8, U8 = 9, 3
FUSED = "(fused into the previous operator)"
ROWS = 5                       # rows 0 and 1 constant at the type's two ends, three random ones
ACT6 = 6.0 / 255.0             # conv_net's act_scale form: what a deep stack needs to stay spread over the range
KIND = {"average_pool_2d": 1, "conv_2d": 3, "depthwise_conv_2d": 4, "fully_connected": 9, "max_pool_2d": 17, "reshape": 22, "softmax": 25}


class Case:
    def __init__(self, name, shape, segments, elem=I8, wzp="none", act_scale=None, seed=0, expect=(), outcomes=(), never=(), front=None, rows=ROWS):
        self.name, self.shape, self.segments, self.elem, self.wzp, self.act_scale = name, tuple(shape), list(segments), elem, wzp, act_scale
        self.seed, self.expect, self.outcomes, self.never, self.front, self.rows = seed, list(expect), list(outcomes), tuple(never), front, rows
        self._model = None

    @property
    def contested(self):
        return not self.expect

    def model(self):
        """(input shape, input quantisation, layer dicts): build_model's arguments.  front = a flat input shape: a Reshape to the
        image is the first operator"""
        if self._model is None:
            import tflite_writer as tw
            in_shape, in_q, layers = tw.stack_layers(np.random.default_rng(self.seed), self.shape, self.segments, self.elem, self.wzp, self.act_scale)
            if self.front:
                layers = [dict(op="reshape", out_shape=in_shape, out_q=in_q)] + layers
                in_shape = tuple(self.front)
            self._model = (in_shape, in_q, layers)
        return self._model

    def blob(self):
        import tflite_writer as tw
        in_shape, in_q, layers = self.model()
        return tw.build_model(in_shape, in_q, layers, self.elem)

    @property
    def dtype(self):
        return np.uint8 if self.elem == U8 else np.int8

    def inputs(self, n=None, seed=1):
        """n rows of the input: row 0 all-minimum, row 1 all-maximum, the rest random"""
        n = self.rows if n is None else n
        lo = 0 if self.elem == U8 else -128
        x = np.random.default_rng(100000 + 31 * self.seed + seed).integers(lo, lo + 256, (n, int(np.prod(self.model()[0]))), dtype=np.int16)
        x[0] = lo
        if n > 1:
            x[1] = lo + 255
        return x.astype(self.dtype)


def expected(case, O, x=None):
    """every operator's tensor [rows, out_elems] for the rows x (the case's own by default): tests/maxpool_ref.segments -- the oracle
    between max pools, the numpy restatement at them"""
    import tflite_writer as tw
    in_shape, in_q, layers = case.model()
    run = R.segments(tw, O, in_shape, in_q, layers, case.elem)
    return run(case.inputs() if x is None else x)


_expected = {}


def expected_once(case, O):
    """expected(case) on the case's five rows (a case that runs fewer uses the first of them), computed once per process and shared;
    callers leave it unchanged"""
    if case.name not in _expected:
        outs = expected(case, O, case.inputs(ROWS))
        for t in outs:
            t.setflags(write=False)
        _expected[case.name] = outs
    return _expected[case.name]


def quantize(x, scale, zp, dt):
    """maxpool_ref.quantize_scalar over an array: as T of roundf(x / scale + zp), each step in f32"""
    F = np.float32
    return R.saturate(R.roundf(np.asarray(x, F) / F(scale) + F(zp)), dt).astype(dt)


def dequantize(O, q, scale, zp, dt):
    """the oracle's dequantize over an array (a table of its 256 answers)"""
    lo = 0 if np.dtype(dt) == np.uint8 else -128
    table = np.array([O.dequantize(v, scale, zp, dt) for v in range(lo, lo + 256)], np.float32)
    return table[np.asarray(q).astype(np.int64) - lo]


def spread(case, outs):
    """per operator whose tensor lies in front of a Softmax: (index, distinct values over the three random rows, the share of their
    elements at the type's two ends)"""
    lo = 0 if case.elem == U8 else -128
    res = []
    for i, L in enumerate(case.model()[2]):
        if L["op"] == "softmax":
            break
        t = np.asarray(outs[i])[2:5].astype(np.int64)
        res.append((i, int(np.unique(t).size), float(((t == lo) | (t == lo + 255)).mean())))
    return res


# ---- the curated joins -------------------------------------------------------------------------------------------------------------
STAGE = [("conv", 16, 5, 1, "valid", "relu"), ("maxpool", 2, 2)]                  # on 12x12x6: conv_maxpool_rt<12x12x6-16;5x5;p2x2s2 (test_gpu_maxpool.py)
BLOCK_A = [("conv", 32, 1, 1), ("dw", 3, 1), ("conv", 8, 1, 1, "same", "none")]    # on 6x6x8: test_gpu_expand_block.BLOCKS[0]
BLOCK_S2 = [("conv", 144, 1, 1), ("dw", 3, 2), ("conv", 32, 1, 1, "same", "none")]  # on 10x10x24: BLOCKS[3]
HEAD = [("gap",), ("fc", 10), ("softmax",)]

JOINS = [
    # 1. avg stage -> max stage -> flatten -> fc -> fc -> softmax: LeNet's geometry with three input channels, the second pool a max pool.
    #    The first stage has six output channels and stays two launches (fused_conv_pool_create: N < 16)
    Case("avg-max-fc", (28, 28, 3), [("conv", 6, 5, 1, "valid", "relu"), ("avgpool", 2, 2)] + STAGE + [("flatten",), ("fc", 120, "relu"), ("fc", 10), ("softmax",)],
         seed=11, expect=[(2, "conv_maxpool_rt<12x12x6-16;5x5;p2x2s2"), (3, FUSED), (5, "fc_chain<2>+sm")]),
    # 2. max stage -> pair -> stride-2 pair -> gap -> fc -> softmax.  The 12x12x6 stage leaves 4x4x16, below every pair the chain tests
    #    assert, so the stage is 24x24x16 -> 64 3x3 SAME (test_gpu_maxpool's "w" class at the next size up), which leaves the 12x12x64 -> 32
    #    pair test_gpu_pair_band.py asserts chain_rt for; the head is test_gpu_pool_fc's 64 -> 10 + softmax on 6x6
    Case("max-pairs-head-i8", (24, 24, 16), [("conv", 64, 3, 1, "same", "relu"), ("maxpool", 2, 2), ("dw", 3, 1), ("conv", 32, 1, 1), ("dw", 3, 2), ("conv", 64, 1, 1)] + HEAD,
         act_scale=ACT6, seed=12, expect=[(0, "conv_maxpool_rt<24x24x16-64;3x3;p2x2s2"), (1, FUSED), (2, "chain_rt<12x12x64-32"), (3, FUSED), (4, "chain_rt<12x12x32s2-64"), (5, FUSED), (6, "pool_fc_chain<1>+sm")]),
    Case("max-pairs-head-u8", (24, 24, 16), [("conv", 64, 3, 1, "same", "relu"), ("maxpool", 2, 2), ("dw", 3, 1), ("conv", 32, 1, 1), ("dw", 3, 2), ("conv", 64, 1, 1)] + HEAD,
         elem=U8, act_scale=ACT6, seed=13, expect=[(0, "conv_maxpool_rt<24x24x16-64;3x3;p2x2s2"), (1, FUSED), (2, "chain_rt<12x12x64-32"), (3, FUSED), (4, "chain_rt<12x12x32s2-64"), (5, FUSED), (6, "pool_fc_chain<1>+sm")]),
    # 3. pair -> expand block -> pair -> gap -> fc -> softmax.  CONTESTED: the block's depthwise + project (144 channels, stride 2, -> 32)
    #    is a run-time-geometry pair with another behind it, so (4c) may chain the two and leave (4d) nothing, or (4d) takes the block.
    #    BLOCKS[3] with 16 input channels instead of 24, so that the pair in front (32 -> 16) has whole 16-channel tiles.  (The planner
    #    of (4c) leaves the two pairs a chain_rt group each, and (4d) then lays block_band_rt over the first: the first outcome)
    Case("pair-block-pair", (10, 10, 32), [("dw", 3, 1), ("conv", 16, 1, 1), ("conv", 144, 1, 1), ("dw", 3, 2), ("conv", 32, 1, 1, "same", "none"), ("dw", 3, 1), ("conv", 32, 1, 1)] + HEAD,
         act_scale=ACT6, seed=14, outcomes=[{2: "block_band_rt<", 3: FUSED, 4: FUSED}, {3: "chain_rt<", 4: FUSED, 5: FUSED, 6: FUSED}]),
    # 4. the shortest form of 3, with nothing in front or behind.  CONTESTED likewise
    Case("block-pair-bare", (10, 10, 16), [("conv", 144, 1, 1), ("dw", 3, 2), ("conv", 32, 1, 1, "same", "none"), ("dw", 3, 1), ("conv", 32, 1, 1)],
         act_scale=ACT6, seed=15, outcomes=[{0: "block_band_rt<", 1: FUSED, 2: FUSED}, {1: "chain_rt<", 2: FUSED, 3: FUSED, 4: FUSED}]),
    # 5. block -> stride-2 block -> global pool -> conv 1x1 (N = 8) -> flatten -> softmax: person_detect's tail, rule (2), behind blocks.
    #    BLOCKS[3] as it is; the block in front of it is BLOCKS[1] (E 64 -> 24) on the 10x10 image the second one needs
    Case("blocks-pd-tail", (10, 10, 16), [("conv", 64, 1, 1), ("dw", 3, 1), ("conv", 24, 1, 1, "same", "none")] + BLOCK_S2 +
         [("avgpool", (5, 5), 5), ("conv", 8, 1, 1, "same", "none"), ("flatten",), ("softmax",)],
         act_scale=ACT6, seed=216, expect=[(0, "block_band_rt<10x10x16-64-24"), (3, "block_band_rt<10x10x24-144s2-32"), (6, "tail_pool_head_softmax<8>"), (7, FUSED), (9, FUSED)]),
    # 6. one-channel conv -> flatten -> fc -> fc -> softmax (tests/conv1_fc_cases "g"'s convolution).  CONTESTED: (5a) takes the
    #    convolution and one FullyConnected and (3) the other with the Softmax, or (5a) declines and (6) chains the two
    Case("conv1-fc-fc", (12, 12, 1), [("conv", 4, 3, 1, "valid", "relu"), ("flatten",), ("fc", 16, "relu"), ("fc", 10), ("softmax",)],
         seed=17, outcomes=[{0: "conv1_fc_rt<conv,3x3,4>", 2: FUSED}, {2: "fc_chain<2>"}]),
    # 7a. a 2x2 avgpool as the first operator -> conv -> gap -> fc: the Conv2D in front of a GLOBAL pool is no conv_pool_rt
    Case("pool-first", (16, 16, 16), [("avgpool", 2, 2), ("conv", 32, 3, 1), ("gap",), ("fc", 10)],
         seed=18, expect=[(2, "pool_fc_chain<1>"), (4, FUSED)], never=("conv_pool_rt<", "conv_maxpool_rt<")),
    # 7b. conv -> a maxpool over the whole image -> flatten -> fc -> fc: one output pixel, so no stage, and a max pool is no pool_fc_chain
    Case("global-maxpool", (8, 8, 8), [("conv", 16, 3, 1, "same", "relu"), ("maxpool", (8, 8), 8), ("flatten",), ("fc", 32, "relu"), ("fc", 10)],
         seed=319, expect=[(3, "fc_chain<2>"), (4, FUSED)], never=("conv_pool_rt<", "conv_maxpool_rt<", "pool_fc_chain<")),
    # 8. pairs with every filter zero point off the middle (test_gpu_pair_wz.SHAPES[2]: 8x6x80 -> 64; then 64 -> 16) -> a block with
    #    zero points (BLOCKS[1]'s E 64 on the 8x6 image, -> 32) -> gap -> fc.  block_band_rt takes no filter zero points: the block's
    #    depthwise + project are a third pair_wz_rt group and its expand keeps pw_rt, which the list leaves open
    Case("wz-pairs-block-i8", (8, 6, 80), [("dw", 3, 1), ("conv", 64, 1, 1), ("dw", 3, 1), ("conv", 16, 1, 1), ("conv", 64, 1, 1), ("dw", 3, 1), ("conv", 32, 1, 1, "same", "none"), ("gap",), ("fc", 10)],
         wzp="all", act_scale=ACT6, seed=20, expect=[(0, "pair_wz_rt<"), (1, FUSED), (2, "pair_wz_rt<"), (3, FUSED)]),
    Case("wz-pairs-block-u8", (8, 6, 80), [("dw", 3, 1), ("conv", 64, 1, 1), ("dw", 3, 1), ("conv", 16, 1, 1), ("conv", 64, 1, 1), ("dw", 3, 1), ("conv", 32, 1, 1, "same", "none"), ("gap",), ("fc", 10)],
         elem=U8, wzp="all", act_scale=ACT6, seed=21, expect=[(0, "pair_wz_rt<"), (1, FUSED), (2, "pair_wz_rt<"), (3, FUSED)]),
    # 9. the smallest pair_band_rt image (test_gpu_pair_band.CASES[0]: 36x36x64) -> a pair small enough for chain_rt -> gap -> fc.  Three
    #    rows.  Behind CASES[0]'s 64 output channels no pair has a chain plan (36x36x64 is beyond chain_rt's 150 KiB at either stride, and
    #    so is 36x36x48 at stride 2), so the band pair writes 32 channels and the pair behind it is 36x36x32 -> 32
    Case("band-chain", (36, 36, 64), [("dw", 3, 1), ("conv", 32, 1, 1), ("dw", 3, 1), ("conv", 32, 1, 1), ("gap",), ("fc", 10)],
         seed=22, rows=3, expect=[(0, "pair_band_rt<36x36x64-32"), (1, FUSED), (2, "chain_rt<36x36x32-32"), (3, FUSED), (4, "pool_fc_chain<1>")]),
    # 10. models that END inside a family
    Case("ends-pair-1x1", (12, 12, 64), [("dw", 3, 1), ("conv", 32, 1, 1), ("dw", 3, 2), ("conv", 64, 1, 1)], seed=23, expect=[(0, "chain_rt<"), (1, FUSED)]),
    Case("ends-project", (6, 6, 8), BLOCK_A, seed=24, expect=[(0, "block_band_rt<6x6x8-32-8"), (1, FUSED), (2, FUSED)]),
    Case("ends-max-stage", (12, 12, 6), [("dw", 3, 1)] + STAGE, seed=25, expect=[(1, "conv_maxpool_rt<12x12x6-16;5x5;p2x2s2"), (2, FUSED)]),
    Case("ends-global-pool", (12, 12, 64), [("dw", 3, 1), ("conv", 32, 1, 1), ("avgpool", (12, 12), 12)], seed=26, expect=[(0, "chain_rt<"), (1, FUSED)],
         never=("pool_fc_chain<", "tail_pool_head_softmax<")),
    # 11. models that BEGIN inside a family
    Case("begins-pair-dw", (12, 12, 64), [("dw", 3, 1), ("conv", 32, 1, 1)] + HEAD, seed=27, expect=[(0, "chain_rt<"), (1, FUSED), (2, "pool_fc_chain<1>+sm")]),
    Case("begins-expand", (6, 6, 8), BLOCK_A + [("flatten",), ("fc", 10), ("softmax",)], seed=28, expect=[(0, "block_band_rt<6x6x8-32-8"), (1, FUSED), (2, FUSED)]),
    # (tests/conv1_fc_cases "g": 12x12, conv 4 3x3 VALID, 5 classes, with the Reshape speech.tflite has in front)
    Case("begins-reshape-conv1", (12, 12, 1), [("conv", 4, 3, 1, "valid", "relu"), ("flatten",), ("fc", 5), ("softmax",)], seed=29, front=(1, 144),
         expect=[(1, "conv1_fc_rt<conv,3x3,4>+sm"), (3, FUSED), (4, FUSED)]),
]
BY_NAME = {c.name: c for c in JOINS}
assert len(BY_NAME) == len(JOINS)

# ---- the grammar -------------------------------------------------------------------------------------------------------------------
CHANNELS = (1, 3, 4, 8, 12, 16, 24, 32)
# 24 of the first 37 seeds: the ones whose expected tensors meet tests/test_composed_host.py's spread condition with room to spare (the
# others saturate somewhere: another seed, not a looser bound)
SEEDS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 12, 14, 15, 17, 20, 21, 25, 26, 29, 30, 31, 33, 34, 36)


_grammar = {}


def grammar(seed):
    """a seeded random stack: an image of at most 16 x 16 with a channel count of CHANNELS; 2 .. 7 conv-like operators (conv K of 1, 3, 5
    at stride 1 or 2, SAME or VALID; depthwise 3 or 5 at stride 1 or 2; both pools); one of four endings (gap + fc (+ fc) (+ softmax);
    flatten + fc (+ softmax); global pool + conv 1x1 + flatten + softmax; nothing); a random element type and zero-point mode.  Never
    a geometry the library refuses at create time: a VALID window always fits the image, and nothing strides or pools an image with
    a side below 4"""
    if seed in _grammar:
        return _grammar[seed]
    rng = np.random.default_rng(424200 + seed)
    h, w, c = int(rng.integers(5, 17)), int(rng.integers(5, 17)), int(rng.choice(CHANNELS))
    shape, segs = (h, w, c), []
    n_ops = int(rng.integers(2, 8))
    for _ in range(n_ops):
        small = min(h, w) < 4
        kind = str(rng.choice(["conv", "conv", "dw", "dw", "avgpool", "maxpool"] if not small else ["conv", "dw"]))
        stride = 1 if small else int(rng.integers(1, 3))
        if kind == "conv":
            k = int(rng.choice([k for k in (1, 3, 5) if k <= min(h, w)]))
            padding = str(rng.choice(["same", "valid"]))
            n = int(rng.choice(CHANNELS[2:]))
            segs.append(("conv", n, k, stride, padding, str(rng.choice(["relu6", "relu", "none"], p=[0.6, 0.2, 0.2]))))
            c = n
        elif kind == "dw":
            k = int(rng.choice([3, 5]))
            padding = "same"
            segs.append(("dw", k, stride, str(rng.choice(["relu6", "none"], p=[0.8, 0.2]))))
        else:
            k = int(rng.choice([2, 3]))
            padding = str(rng.choice(["same", "valid"]))
            segs.append((kind, k, stride, padding))
        if padding == "same":
            h, w = -(-h // stride), -(-w // stride)
        else:
            h, w = (h - k) // stride + 1, (w - k) // stride + 1
        assert min(h, w) >= 1
    ending = int(rng.integers(0, 4))
    if ending == 0:
        segs.append(("gap",))
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
    _grammar[seed] = Case("g%02d" % seed, shape, segs, elem=elem, wzp=wzp, act_scale=ACT6 if n_ops >= 4 else None, seed=5000 + seed)
    return _grammar[seed]


def cases():
    """every join and every seed's stack"""
    return JOINS + [grammar(s) for s in SEEDS]
