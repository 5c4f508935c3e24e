"""DepthwiseConv2D 3x3 + Conv2D 1x1 pairs whose filters carry zero points as one pair_wz_rt launch (k_pair_wz.hip): routing,
bit-exactness against the CPU oracle on every image, against the operators' own launches and against the shape-generic kernels, the
largest accumulators the members' bounds allow, the bytes around the output, run_until / hipGraph / the MF_NO_PAIR_WZ switch, whole
person_detect-shaped models with zero points everywhere, and the pairs that must keep the launches they have."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests.conftest import ROOT, ROUTING_SWITCHED

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))

FUSED = "(fused into the previous operator)"
LABEL = "pair_wz_rt<"
# (H, W, C), stride, N: what each covers
SHAPES = [
    ((5, 7, 16), 1, 16),        # odd width: one column per unit, sixteen images per column grid
    ((8, 8, 48), 2, 32),        # one padded k step; three channel groups: no swizzle
    ((8, 6, 80), 1, 64),        # two k steps, the second mostly padding
    ((6, 6, 128), 1, 128),      # two full k steps
    ((12, 12, 64), 2, 128),     # several units per wave
    ((4, 4, 256), 1, 256),      # four k steps
    ((3, 3, 192), 1, 64),       # twelve channel groups: not a power of two
]
WHICH = ["dw", "pw", "both"]    # the member(s) whose filter zero points are off the middle
ACTS = [("relu6", "none"), ("relu", "relu6"), ("none", "relu")]    # (depthwise, 1x1): TFLite activations 3, 0, 1 on either member
GRID = [(si, wi) for si in range(len(SHAPES)) for wi in range(len(WHICH))]


def _elem(idx):
    import tflite_writer as tw
    return tw.UINT8 if idx % 2 else tw.INT8


def _grid_id(c):
    (H, W, C), S, N = SHAPES[c[0]]
    idx = 3 * c[0] + c[1]
    return "%dx%dx%d%s-%d-%s-%s" % (H, W, C, "s2" if S == 2 else "", N, WHICH[c[1]], "u8" if idx % 2 else "i8")


def pair_blob(rng, shape, S, N, elem, which, acts=("relu6", "relu6"), zp_ends=False, w_end=None, in_zp=None, osc=(None, None), pw_out_scale=None):
    """one depthwise 3x3 SAME + 1x1 pair (tools/tflite_writer.build_model; conv_net keeps depthwise zero points at the middle), per-channel
    filter quantisation.  `which`: the member(s) with filter zero points off the middle (never AT the middle on any channel), "none" for a
    plain pair.  zp_ends: those zero points sit at the two ends of the type's range, alternating over the channels; w_end = "opposite":
    every weight at the end opposite to its channel's zero point.  in_zp: the input's zero point.  osc: output scales (None: conv_net's)."""
    import tflite_writer as tw
    lo, hi = (0, 256) if elem == tw.UINT8 else (-128, 128)
    mid = (lo + hi) // 2
    H, W, C = shape
    OH, OW = -(-H // S), -(-W // S)
    in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, hi - 20)) if in_zp is None else int(in_zp))
    q = in_q
    layers = []
    for dw, n, taps, s, act, oshape, o in ((True, C, 9, S, acts[0], (1, OH, OW, C), osc[0]), (False, N, C, 1, acts[1], (1, OH, OW, N), osc[1])):
        sc = rng.uniform(0.002, 0.01, n).astype(np.float32)
        zp = np.full(n, mid)
        if which in ("both", "dw" if dw else "pw"):
            zp = rng.integers(mid - 12, mid + 13, n)
            zp[zp == mid] = mid + 5
            if zp_ends:
                zp = np.where(np.arange(n) % 2 == 0, lo, hi - 1)
        o = float(np.float32(q[0] * float(sc.mean()) * 60.0 * np.sqrt(taps))) if o is None else float(np.float32(o))
        ozp = lo if act == "relu6" else int(rng.integers(lo + 20, hi - 20))
        wshape = (1, 3, 3, n) if dw else (n, 1, 1, C)
        w = rng.integers(lo, hi, wshape)
        if w_end == "opposite":
            opp = np.where(zp <= mid, hi - 1, lo)          # per output channel
            w = np.broadcast_to(opp.reshape((1, 1, 1, n) if dw else (n, 1, 1, 1)), wshape).copy()
        d = dict(op="depthwise_conv_2d" if dw else "conv_2d", fscale=sc, fzp=zp, bias=rng.integers(-500, 500, n),
                 bscale=(sc * np.float32(q[0])).astype(np.float32), bzp=np.zeros(n, np.int64), padding="same", strides=(s, s), act=act,
                 out_shape=oshape, out_q=(o, ozp))
        d["weights" if dw else "filters"] = w
        layers.append(d)
        q = d["out_q"]
    if pw_out_scale is not None:
        layers[1]["out_q"] = (float(pw_out_scale), layers[1]["out_q"][1])
    return tw.build_model((1,) + tuple(shape), in_q, layers, elem)


def _inputs(m, n, seed):
    """n images: image 0 all-minimum, image 1 all-maximum, the rest random"""
    lo, hi = (0, 256) if m.dtype == np.uint8 else (-128, 128)
    x = np.random.default_rng(seed).integers(lo, hi, (n, m.input_elems), dtype=np.int16).astype(m.dtype)
    x[0] = lo
    if n > 1:
        x[1] = hi - 1
    return x


def _names(m):
    return [m.op(i)["kernel"] for i in range(m.num_ops)]


class Case:
    """one model of the grid: prepared once, its oracle result computed once and shared"""
    def __init__(self, O, blob, n, seed):
        import microflow_rs_amd as mf
        self.blob = blob
        self.m = mf.Model(blob)
        self.m.prepare(1)
        self.om = O.Model(blob)
        self.x = _inputs(self.m, n, seed)
        self.want = self.om.run_quantized_batch(self.x).reshape(n, -1)


_cases = {}


def _grid_case(O, c):
    if c not in _cases:
        shape, S, N = SHAPES[c[0]]
        idx = 3 * c[0] + c[1]
        blob = pair_blob(np.random.default_rng(900 + idx), shape, S, N, _elem(idx), WHICH[c[1]], ACTS[idx % 3])
        _cases[c] = Case(O, blob, 37, 1900 + idx)
    return _cases[c]


def _assert_wz_group(m):
    if not ROUTING_SWITCHED:
        names = _names(m)
        assert names[0].startswith(LABEL) and names[1] == FUSED, names


def _same(got, want):
    for i in range(want.shape[0]):                       # every image
        bad = np.flatnonzero(got[i] != want[i])
        assert bad.size == 0, (i, bad.size, bad[:8], got[i][bad[:8]], want[i][bad[:8]])


# ---- 1. the grid ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GRID, ids=_grid_id)
def test_pair_is_one_zero_point_launch_and_equals_the_oracle(O, c):
    case = _grid_case(O, c)
    m = case.m
    _assert_wz_group(m)                                  # (what fails without the route: the pair is two launches there)
    _same(m.run_quantized(case.x).reshape(37, -1), case.want)                  # batch 37: ragged last step for every G
    assert np.array_equal(m.run_quantized(case.x[2:3]).reshape(-1), case.want[2])   # batch 1
    m.set_fusion(False)
    try:
        off = m.run_quantized(case.x).reshape(37, -1)
        if not ROUTING_SWITCHED:
            assert not any(k.startswith(LABEL) or k == FUSED for k in _names(m)), _names(m)
    finally:
        m.set_fusion(True)
    _same(off, case.want)
    m.set_generic(True)
    try:
        gen = m.run_quantized(case.x).reshape(37, -1)
    finally:
        m.set_generic(False)
    _same(gen, case.want)
    _assert_wz_group(m)


def test_the_grid_covers_both_element_types_and_every_activation(O):
    import tflite_writer as tw
    seen = {(_elem(3 * si + wi), ACTS[(3 * si + wi) % 3]) for si, wi in GRID}
    assert {e for e, _ in seen} == {tw.INT8, tw.UINT8}
    assert {a for _, (a, _) in seen} == {"none", "relu", "relu6"} == {a for _, (_, a) in seen}


def test_persistent_workgroups_walk_many_ragged_steps(O):
    """the smallest shape at batch 4100: more steps than resident workgroups, a ragged last one, every image against the oracle"""
    shape, S, N = SHAPES[0]
    import tflite_writer as tw
    for elem, which in ((tw.INT8, "both"), (tw.UINT8, "dw")):
        case = Case(O, pair_blob(np.random.default_rng(41), shape, S, N, elem, which), 4100, 42)
        _assert_wz_group(case.m)
        _same(case.m.run_quantized(case.x).reshape(4100, -1), case.want)


# ---- 2. extremes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
@pytest.mark.parametrize("shape,N", [((4, 4, 256), 256), ((3, 3, 16), 16)], ids=["4x4x256", "3x3x16-border"])
def test_extreme_zero_points_weights_and_images(O, shape, N, u8):
    """filter zero points at both ends of the range (alternating over the channels), every weight at the opposite end, the input zero
    point at an end, images constant at either end: the largest |acc| the members' bounds allow -- at 256 input channels
    256 * 255 * 255 > 2^22, so the launch must be the v_cvt instance (mode 0); at 3x3x16 every pixel is a border pixel and
    halo x zero point is the dominant term"""
    import tflite_writer as tw
    elem = tw.UINT8 if u8 else tw.INT8
    lo, hi = (0, 256) if u8 else (-128, 128)
    C = shape[2]
    for in_zp in (lo, hi - 1):
        # output scales that keep the extreme accumulators (9 * 255 * 255, C * 255 * 255) a hundred output steps wide
        sc_in, fs = 0.05, 0.006
        osc0 = sc_in * fs * 9 * 255 * 255 / 100.0
        osc = (osc0, osc0 * fs * C * 255 * 255 / 100.0)
        blob = pair_blob(np.random.default_rng(77 + in_zp - lo), shape, 1, N, elem, "both", ("none", "none"), zp_ends=True, w_end="opposite", in_zp=in_zp, osc=osc)
        case = Case(O, blob, 6, 78)
        case.x[2], case.x[3] = lo, hi - 1
        case.x[4, ::2], case.x[4, 1::2] = lo, hi - 1
        case.want = case.om.run_quantized_batch(case.x).reshape(6, -1)
        m = case.m
        _assert_wz_group(m)
        if not ROUTING_SWITCHED and C == 256:
            assert m.op_epilogue_mode(0) == 0, m.op_epilogue_mode(0)
        _same(m.run_quantized(case.x).reshape(6, -1), case.want)
        assert len({bytes(w) for w in case.want}) > 1    # (the outputs are not one saturated constant)


# ---- 3. guard bytes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [(0, 2), (1, 0), (6, 1)], ids=_grid_id)
@pytest.mark.parametrize("offset", [16, 48])
def test_nothing_is_written_outside_the_output(O, c, offset):
    import torch
    case = _grid_case(O, c)
    m = case.m
    n, elems = 37, case.want.shape[1]
    x = torch.as_tensor(case.x).cuda()
    dt = torch.uint8 if m.dtype == np.uint8 else torch.int8
    buf = torch.full((offset + n * elems + 4096,), 0x5A, dtype=dt, device="cuda")
    m.run_quantized(x, out=buf[offset:offset + n * elems])
    b = buf.cpu().numpy()
    _same(b[offset:offset + n * elems].reshape(n, -1), case.want)
    assert (b[:offset] == 0x5A).all() and (b[offset + n * elems:] == 0x5A).all()


# ---- 4. controls ----------------------------------------------------------------------------------------------------------------
def test_run_until_the_depthwise_is_the_oracles_layer(O):
    case = _grid_case(O, (4, 2))
    _, layers = case.om.run_quantized(case.x[3], layers=True)
    got = np.asarray(case.m.run_until(case.x[3:4], 0)).reshape(-1)
    assert np.array_equal(got, layers[0].reshape(-1))
    assert np.array_equal(np.asarray(case.m.run_until(case.x[3:4], 1)).reshape(-1), case.want[3])


def test_graph_replay_gives_the_same_bytes(O):
    import torch
    case = _grid_case(O, (3, 2))
    m = case.m
    xd = torch.as_tensor(case.x).cuda()
    m.set_graph(True)
    try:
        out = torch.empty_like(torch.as_tensor(case.want)).cuda()
        for it in range(3):                              # eager, captured + replayed, replayed
            out.zero_()
            m.run_quantized(xd, out=out)
            assert np.array_equal(out.cpu().numpy().reshape(37, -1), case.want), it
    finally:
        m.set_graph(False)


def test_no_pair_wz_switch_goes_back_to_the_operators(O):
    """MF_DEV=1 MF_NO_PAIR_WZ=1 (a child process: the switches are read once per process): the members run dw3x3_rt<S,wzp> and
    pw_rt<K,N,wzp> with the same bytes"""
    case = _grid_case(O, (4, 2))
    code = r'''
import sys, numpy as np
sys.path.insert(0, %r)
import microflow_rs_amd as mf
m = mf.Model(open(sys.argv[1], "rb").read())
m.prepare(1)
x = np.load(sys.argv[2])
print("KERNELS", "|".join(m.op(i)["kernel"] for i in range(m.num_ops)))
np.save(sys.argv[3], m.run_quantized(x).reshape(x.shape[0], -1))
''' % (ROOT,)
    outs, kernels = [], []
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "m.tflite"), "wb").write(case.blob)
        np.save(os.path.join(tmp, "x.npy"), case.x)
        for sw in (None, "1"):
            env = dict(os.environ)
            for k in [k for k in env if k.startswith("MF_")]:
                del env[k]
            if sw:
                env.update(MF_DEV="1", MF_NO_PAIR_WZ="1")
            path = os.path.join(tmp, "out%d.npy" % len(outs))
            r = subprocess.run([sys.executable, "-c", code, os.path.join(tmp, "m.tflite"), os.path.join(tmp, "x.npy"), path], capture_output=True, text=True,
                               timeout=600, env=env, cwd=ROOT)
            assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
            kernels.append([l for l in r.stdout.splitlines() if l.startswith("KERNELS")][0].split(" ", 1)[1].split("|"))
            outs.append(np.load(path))
    on, off = kernels
    assert on[0].startswith(LABEL) and on[1] == FUSED, on
    assert off[0].startswith("dw3x3_rt<") and off[0].endswith(",wzp>") and off[1].startswith("pw_rt<") and off[1].endswith(",wzp>"), off
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], case.want)


# ---- 5. whole models --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side,width,nst,u8", [(80, 1.0, 4, False), (72, 0.5, 5, True)], ids=["80-1.0-4-i8", "72-0.5-5-u8"])
def test_person_detect_shaped_models_with_zero_points_everywhere(O, side, width, nst, u8):
    import microflow_rs_amd as mf
    import tflite_writer as tw
    blob = tw.person_detect_like(np.random.default_rng(side * 7 + nst), side, width, tw.UINT8 if u8 else tw.INT8, True, nst)
    m, om = mf.Model(blob), O.Model(blob)
    m.prepare(1)
    names = _names(m)
    if not ROUTING_SWITCHED:
        groups = [i for i, k in enumerate(names) if k.startswith(LABEL)]
        assert groups and all(names[i + 1] == FUSED for i in groups), names
    x = _inputs(m, 6, side)
    want = om.run_quantized_batch(x).reshape(6, -1)
    _same(m.run_quantized(x).reshape(6, -1), want)
    _, layers = om.run_quantized(x[5], layers=True)
    for k in range(m.num_ops):                           # every layer: a group's depthwise alone runs the pair unfused
        assert np.array_equal(np.asarray(m.run_until(x[5:6], k)).reshape(-1), layers[k].reshape(-1)), (k, names[k])
    m.set_fusion(False)
    try:
        _same(m.run_quantized(x).reshape(6, -1), want)
    finally:
        m.set_fusion(True)


# ---- 6. what must not move ----------------------------------------------------------------------------------------------------------
# (no shape class is excluded on speed grounds: DESIGN 4.15's table)
def _outside(name):
    import tflite_writer as tw
    rng = np.random.default_rng(66)
    if name == "C8-superpixel":
        return pair_blob(rng, (8, 8, 8), 1, 16, tw.INT8, "both")
    if name == "C24":
        return pair_blob(rng, (8, 8, 24), 1, 32, tw.INT8, "both")
    if name == "56x56x128-too-large":
        return pair_blob(rng, (56, 56, 128), 1, 128, tw.INT8, "both")
    if name == "non-finite-constant":
        return pair_blob(rng, (6, 6, 32), 1, 32, tw.INT8, "both", ("relu6", "none"), pw_out_scale=0.0)   # c0, c1 = x / 0
    if name == "N48-three-tiles":
        return pair_blob(rng, (6, 6, 32), 1, 48, tw.INT8, "both")      # chain_plan refuses three output tiles
    if name == "9x9x32s2-odd-width":
        return pair_blob(rng, (9, 9, 32), 2, 32, tw.INT8, "both")
    raise ValueError(name)


@pytest.mark.parametrize("name", ["C8-superpixel", "C24", "56x56x128-too-large", "non-finite-constant", "N48-three-tiles", "9x9x32s2-odd-width"])
def test_zero_point_pairs_outside_the_route_keep_their_launches(O, name):
    import microflow_rs_amd as mf
    blob = _outside(name)
    m = mf.Model(blob)
    m.prepare(1)
    if not ROUTING_SWITCHED:
        names = _names(m)
        assert not any("pair_wz" in k for k in names) and FUSED not in names, names
    n = 2 if name.startswith("56x56") else 5
    x = _inputs(m, n, 67)
    _same(m.run_quantized(x).reshape(n, -1), O.Model(blob).run_quantized_batch(x).reshape(n, -1))


def test_pairs_without_filter_zero_points_keep_their_groups(O):
    """a plain pair is chain_rt's, with or without the new route"""
    import microflow_rs_amd as mf
    import tflite_writer as tw
    blob = pair_blob(np.random.default_rng(5), (12, 12, 64), 1, 32, tw.INT8, "none")
    m = mf.Model(blob)
    m.prepare(1)
    if not ROUTING_SWITCHED:
        names = _names(m)
        assert names[0].startswith("chain_rt<") and names[1] == FUSED, names


def test_a_model_without_filter_zero_points_has_the_same_kernels_with_and_without_the_switch():
    code = r'''
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import microflow_rs_amd as mf
import tflite_writer as tw
m = mf.Model(tw.person_detect_like(np.random.default_rng(453), 64, 1.0, tw.INT8, False, 5))
m.prepare(1)
print("KERNELS", "|".join(m.op(i)["kernel"] for i in range(m.num_ops)))
''' % (ROOT, os.path.join(ROOT, "tools"))
    kernels = []
    for sw in (None, "1"):
        env = dict(os.environ)
        for k in [k for k in env if k.startswith("MF_")]:
            del env[k]
        if sw:
            env.update(MF_DEV="1", MF_NO_PAIR_WZ="1")
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        kernels.append([l for l in r.stdout.splitlines() if l.startswith("KERNELS")][0])
    assert kernels[0] == kernels[1] and "pair_wz" not in kernels[0], kernels
