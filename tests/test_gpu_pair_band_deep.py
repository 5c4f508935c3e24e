"""DepthwiseConv2D 3x3 + Conv2D 1x1 pairs of 256 < C <= 512 input channels as one pair_band_deep_rt launch (k_pair_band_deep.hip: the
band-by-band pair with eight k steps): routing, bit-exactness against the CPU oracle and against the operators' own launches, the
bytes around the output, workgroups that walk many steps, the 512-channel middle of a MobileNet-v1 every way the model can be run,
the pairs that must keep today's launches, the MF_NO_PAIR_BAND switch and an unaligned input pointer."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests.conftest import ROOT, ROUTING_SWITCHED

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))

FUSED = "(fused into the previous operator)"
LABEL = "pair_band_deep_rt<"
GUARD = 4096
# name, (H, W, C), stride, N, u8, conv_net options, the epilogue mode the launch reports.
# The mode is the minimum of the two operators'; the 1x1's input zero point is the type's minimum, so its accumulator bound is
# 255 x the largest sum of |w| over a filter: K = 512 full-range weights give about 512 x 64 x 255 = 8.4e6 > 2^22 (mode 0), weights
# within +-24 at most 512 x 24 x 255 = 3.1e6 and K <= 384 within +-40 at most 384 x 40 x 255 = 3.9e6, both < 2^22 (mode 1: relu6 is
# not the whole range at the default scales).
CASES = [
    ("14x14x512-512", (14, 14, 512), 1, 512, False, dict(wmax=24), 1),         # KS = 8 with 32 channel groups (the swizzle); two bands of 8 rows, the
                                                                               # second ragged (rows 14, 15 never stored); 16 blocks: two passes
    ("8x8x512-528", (8, 8, 512), 1, 528, False, dict(), 0),                    # full-range weights: accumulators leave +-2^22, v_cvt epilogue; 33 tiles,
                                                                               # one per block, five passes; one band that is the whole image
    ("16x16x512s2-1024-u8", (16, 16, 512), 2, 1024, True, dict(wmax=24), 1),   # stride 2; 32 blocks: four passes; two bands of 4 rows
    ("10x10x320-320", (10, 10, 320), 1, 320, False, dict(), 0),                # KS = 5; 20 channel groups, no swizzle; CY = 8: one 16-row band, rows
                                                                               # 10 .. 15 computed and never stored
    ("12x12x272-288", (12, 12, 272), 1, 288, False, dict(wmax=40), 1),         # a fifth k step holding ONE channel group: clamped planes x zero weights
    ("13x7x384-384-u8", (13, 7, 384), 1, 384, True, dict(wmax=40), 1),         # odd H, W and OW: one-column units, one 16-row band
    ("8x8x512-512-sat", (8, 8, 512), 1, 512, False, dict(act_scale=6.0 / 255.0, wmax=40), 2),  # relu6 = the whole range: saturating pack
]
IDS = [c[0] for c in CASES]
# the 512-channel middle of a MobileNet-v1 at 224 x 224 and the pair behind it
MIDDLE = [("dw", 0, 3, 1), ("conv", 512, 1, 1)] * 5 + [("dw", 0, 3, 2), ("conv", 1024, 1, 1)]


def _pair_blob(seed, shape, S, N, u8, **kw):
    import tflite_writer as tw
    return tw.conv_net(np.random.default_rng(seed), shape, [("dw", 0, 3, S), ("conv", N, 1, 1)], elem=tw.UINT8 if u8 else tw.INT8, **kw)


def _inputs(m, n, seed):
    """n images: image 0 all-minimum, image 1 all-maximum, the rest random"""
    lo, hi = (0, 256) if m.dtype == np.uint8 else (-128, 128)
    x = np.random.default_rng(seed).integers(lo, hi, (n, m.input_elems), dtype=np.int16).astype(m.dtype)
    x[0], x[1] = lo, hi - 1
    return x


def _names(m):
    return [m.op(i)["kernel"] for i in range(m.num_ops)]


class Pair:
    def __init__(self, O, case, seed):
        import microflow_rs_amd as mf
        name, shape, S, N, u8, kw, mode = case
        self.blob = _pair_blob(seed, shape, S, N, u8, **kw)
        self.m = mf.Model(self.blob)
        self.m.prepare(1)
        self.om = O.Model(self.blob)
        self.x = _inputs(self.m, 6, seed + 1)
        self.want = self.om.run_quantized_batch(self.x).reshape(6, -1)
        self.mode = mode


_pairs = {}


def _pair(O, i):
    if i not in _pairs:
        _pairs[i] = Pair(O, CASES[i], 900 + 10 * i)
    return _pairs[i]


@pytest.fixture(params=range(len(CASES)), ids=IDS)
def pair(request, O):
    return _pair(O, request.param)


# ---- 1. the pair cases ---------------------------------------------------------------------------------------------------
def test_pair_is_one_deep_band_launch_and_equals_the_oracle(pair):
    import torch
    m = pair.m
    if not ROUTING_SWITCHED:
        names = _names(m)
        assert names[0].startswith(LABEL) and names[1] == FUSED, names
        assert m.op_epilogue_mode(0) == pair.mode, (m.op_epilogue_mode(0), names)
    n, elems = 6, pair.want.shape[1]
    x = torch.as_tensor(pair.x).cuda()
    dt = torch.uint8 if m.dtype == np.uint8 else torch.int8
    buf = torch.full((GUARD + n * elems + GUARD,), 0x5A, dtype=dt, device="cuda")
    out = buf[GUARD:GUARD + n * elems]
    m.run_quantized(x, out=out)
    b = buf.cpu().numpy()
    got = b[GUARD:GUARD + n * elems].reshape(n, -1).copy()
    for i in range(n):                                   # every image against the oracle
        bad = np.flatnonzero(got[i] != pair.want[i])
        assert bad.size == 0, (i, bad.size, bad[:8])
    assert (b[:GUARD] == 0x5A).all() and (b[GUARD + n * elems:] == 0x5A).all()        # the guards untouched
    m.set_fusion(False)
    try:
        off = m.run_quantized(x).cpu().numpy().reshape(n, -1)
        if not ROUTING_SWITCHED:
            assert not any(k.startswith("pair_band") or k == FUSED for k in _names(m)), _names(m)
    finally:
        m.set_fusion(True)
    assert np.array_equal(got, off)                      # the whole batch against the operators' own launches
    buf.fill_(0x5A)
    m.run_quantized(x, out=out)                          # a second launch: identical, guards included
    assert np.array_equal(buf.cpu().numpy(), b)


def test_the_launches_report_every_epilogue_mode(O):
    """what the models report, not what the table above says: together the deep band launches run all three epilogue forms"""
    if ROUTING_SWITCHED:
        return
    ms = [_pair(O, i).m for i in range(len(CASES))]
    seen = {m.op_epilogue_mode(0) for m in ms if _names(m)[0].startswith(LABEL)}
    assert seen == {0, 1, 2}, seen


# ---- 2. several steps per workgroup ---------------------------------------------------------------------------------------
def test_workgroups_that_walk_many_steps(O):
    """more than three steps for the one resident workgroup of every CU: a workgroup goes border band -> next image's border band ...,
    which is where a tile row left over from the step before would show"""
    import torch
    import microflow_rs_amd as mf
    name, shape, S, N, u8, kw, _ = CASES[0]
    blob = _pair_blob(900, shape, S, N, u8, **kw)
    m = mf.Model(blob)
    m.prepare(1)
    label = m.op(0)["kernel"]
    NB = 2                                               # (14 rows in bands of 8: tests/test_pair_band_deep_host.py pins the plan)
    if not ROUTING_SWITCHED:
        assert label.startswith(LABEL), label
        NB = int(re.search(r";NB(\d+)>", label).group(1))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    batch = -(-3 * cus // NB) + 1
    x = _inputs(m, batch, 34)
    xd = torch.as_tensor(x).cuda()
    got = m.run_quantized(xd).cpu().numpy().reshape(batch, -1)
    m.set_fusion(False)
    try:
        off = m.run_quantized(xd).cpu().numpy().reshape(batch, -1)
    finally:
        m.set_fusion(True)
    bad = np.flatnonzero((got != off).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:8])
    pick = sorted({0, 1, batch // 2, batch - 2, batch - 1})
    want = O.Model(blob).run_quantized_batch(x[pick]).reshape(len(pick), -1)
    assert np.array_equal(got[pick], want)


# ---- 3. the 512-channel middle of a MobileNet-v1 ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def middle(O):
    import microflow_rs_amd as mf
    import tflite_writer as tw
    blob = tw.conv_net(np.random.default_rng(512), (14, 14, 512), MIDDLE, act_scale=6.0 / 255.0, wmax=40)
    m = mf.Model(blob)
    m.prepare(1)
    x = _inputs(m, 3, 513)
    return blob, m, O.Model(blob), x


def test_mobilenet_middle_pairs_are_deep_band_groups(middle):
    blob, m, om, x = middle
    if ROUTING_SWITCHED:
        return
    names = _names(m)
    for i in (0, 2, 4, 6, 8):
        assert names[i].startswith(LABEL + "14x14x512-512;") and names[i + 1] == FUSED, names
    # 14x14x512 s2 -> 1024: OW = 7 forces 16-row bands, whose tile does not fit: two operators
    assert names[11] != FUSED and not names[10].startswith("pair_band"), names


def test_mobilenet_middle_equals_the_oracle_every_way(middle):
    import torch
    blob, m, om, x = middle
    got = m.run_quantized(x).reshape(3, -1)
    want = om.run_quantized_batch(x).reshape(3, -1)
    for i in range(3):
        assert np.array_equal(got[i], want[i]), i
    _, layers = om.run_quantized(x[2], layers=True)
    for k in (2, 3, 8, 9, 10):                           # 2, 8: a group's depthwise alone (the pair runs unfused); 3, 9: whole groups
        g = np.asarray(m.run_until(x[2:3], k)).reshape(-1)
        assert np.array_equal(g, layers[k].reshape(-1)), k
    m.set_fusion(False)
    try:
        assert np.array_equal(m.run_quantized(x).reshape(3, -1), got)
    finally:
        m.set_fusion(True)
    m.set_generic(True)
    try:
        assert np.array_equal(m.run_quantized(x).reshape(3, -1), got)
    finally:
        m.set_generic(False)
    xd = torch.as_tensor(x).cuda()
    m.set_graph(True)
    try:
        out = torch.empty_like(torch.as_tensor(got)).cuda()
        for it in range(3):                              # eager, captured + replayed, replayed
            out.zero_()
            m.run_quantized(xd, out=out)
            assert np.array_equal(out.cpu().numpy().reshape(3, -1), got), it
    finally:
        m.set_graph(False)


# ---- 4. what must not move --------------------------------------------------------------------------------------------------
# 14x14x512 s2 -> 1024 has no plan (see above); 7x7x1024 -> 1024 and 14x14x528 -> 64 are beyond 512 channels; 14x14x264 is no multiple of 16.
# Excluded on speed grounds (not faster than the operators' own launches by a margin safely above the spread of the repeats):
# at most 256 outputs, where the 1x1 alone runs a weights-in-registers kernel (14x14x512 -> 256 ran x1.12 at a spread of 0.106).
@pytest.mark.parametrize("shape,S,N", [((14, 14, 512), 2, 1024), ((7, 7, 1024), 1, 1024), ((14, 14, 528), 1, 64), ((14, 14, 264), 1, 64),
                                       ((14, 14, 512), 1, 256), ((8, 8, 384), 1, 128)],
                         ids=["14x14x512s2-1024-no-plan", "7x7x1024", "14x14x528", "14x14x264", "14x14x512-256-slower", "8x8x384-128-slower"])
def test_pairs_outside_the_route_keep_their_launches(O, shape, S, N):
    import microflow_rs_amd as mf
    blob = _pair_blob(57, shape, S, N, False)
    m = mf.Model(blob)
    m.prepare(1)
    if not ROUTING_SWITCHED:
        names = _names(m)
        assert not any(k.startswith("pair_band") for k in names) and FUSED not in names, names
    x = _inputs(m, 5, 58)
    assert np.array_equal(m.run_quantized(x).reshape(5, -1), O.Model(blob).run_quantized_batch(x).reshape(5, -1))


# ---- 5. the switch --------------------------------------------------------------------------------------------------------
def test_no_pair_band_switch_goes_back_to_the_operators():
    """MF_DEV=1 MF_NO_PAIR_BAND=1 (a child process: the switches are read once per process): the middle's pairs run their operators'
    own launches with the same bytes as the deep band groups in the other child"""
    code = r'''
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import microflow_rs_amd as mf
import tflite_writer as tw
m = mf.Model(tw.conv_net(np.random.default_rng(512), (14, 14, 512), %r, act_scale=6.0 / 255.0, wmax=40))
m.prepare(1)
x = np.random.default_rng(6).integers(-128, 128, (2, m.input_elems)).astype(np.int8)
print("KERNELS", "|".join(m.op(i)["kernel"] for i in range(m.num_ops)))
np.save(sys.argv[1], m.run_quantized(x).reshape(2, -1))
''' % (ROOT, os.path.join(ROOT, "tools"), MIDDLE)
    outs, kernels = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for sw in (None, "1"):
            env = dict(os.environ)
            for k in [k for k in env if k.startswith("MF_")]:
                del env[k]
            if sw:
                env.update(MF_DEV="1", MF_NO_PAIR_BAND="1")
            path = os.path.join(tmp, "out%d.npy" % len(outs))
            r = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
            assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
            kernels.append([l for l in r.stdout.splitlines() if l.startswith("KERNELS")][0].split(" ", 1)[1].split("|"))
            outs.append(np.load(path))
    assert np.array_equal(outs[0], outs[1])
    on, off = kernels
    assert all(on[i].startswith(LABEL) and on[i + 1] == FUSED for i in (0, 2, 4, 6, 8)), on
    assert FUSED not in off and not any(k.startswith("pair_band") for k in off), off
    assert off[10:] == on[10:]


# ---- 6. an input pointer that is not 16-byte aligned ----------------------------------------------------------------------------
def test_input_view_offset_by_four_bytes(pair):
    """a caller's device pointer that is not 16-byte aligned gives the same bytes: the deep band launch (whose LDS-DMA reads 16-byte
    words) never sees it -- the pair's input goes through the model's own aligned buffer or the operators' own launches"""
    import torch
    m = pair.m
    flat = pair.x.reshape(-1)
    buf = torch.zeros(flat.size + 64, dtype=torch.uint8 if m.dtype == np.uint8 else torch.int8, device="cuda")
    view = buf[4:4 + flat.size]
    view.copy_(torch.as_tensor(flat))
    assert view.data_ptr() % 16 == 4
    got = m.run_quantized(view).cpu().numpy().reshape(6, -1)
    assert np.array_equal(got, pair.want)
