"""Conv2D 1x1 expand + DepthwiseConv2D 3x3 + Conv2D 1x1 project blocks with 320 <= E <= 1024 as one block_slice_rt launch
(k_block_slice.hip): routing, bit-exactness against the CPU oracle and against the operators' own launches and the generic kernels on a
ragged batch, every operator of the block through run_until, and workgroups that walk several steps."""
import os
import sys

import numpy as np
import pytest

from tests.conftest import ROOT, ROUTING_SWITCHED

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))

FUSED = "(fused into the previous operator)"
BATCH = 37
# (H, W, C), E, S, N: what each is the smallest case of
BLOCKS = [
    ((6, 6, 8), 320, 1, 8),          # one band, K padded from 8, N below one tile, five slices
    ((9, 7, 16), 384, 1, 24),        # odd H and W: ragged chunks in all GEMM phases, 1.5 output tiles
    ((10, 10, 24), 320, 2, 32),      # stride 2
    ((14, 14, 96), 576, 1, 96),      # two k steps of C, 14 chunks x 6 tiles of accumulators
    ((7, 7, 160), 960, 1, 320),      # three k steps of C, fifteen slices, twenty N tiles: the most accumulators per wave
    ((40, 40, 16), 320, 1, 16),      # does not fit as one band: NB >= 2, border and interior bands, halo rows expanded twice
    # the first two keep their launches (KEPT below); these are their edges on routed blocks
    ((10, 10, 8), 320, 2, 8),        # K padded from 8, N below one tile: the store mask, the padded constants and filter rows
    ((9, 7, 96), 384, 1, 24),        # odd H and W, 1.5 output tiles, two units per wave
    ((9, 7, 96), 384, 1, 40),        # 2.5 output tiles, four units per wave
    ((3, 3, 160), 960, 1, 160),      # less than one chunk per image; one launch up to 256 images
]
# name, builder ("ir": inverted_residual_net; "cn": conv_net with wmax = 40 and act_scale = 6 / 255, the saturating pack), block, u8
CASES = [("%dx%dx%d-%d%s-%d-%s" % (s + (E, "s2" if S == 2 else "", N, "u8" if u8 else "i8")), "ir", (s, E, S, N), u8)
         for i, (s, E, S, N) in enumerate(BLOCKS) for u8 in ((False, True) if i in (0, 2, 4, 6) else (False,))]
CASES += [("10x10x24-320s2-32-sat", "cn", BLOCKS[2], False)]
PICK = [0, 1, 2, BATCH - 1]
# one k step of C at stride 1 with the image in one band is a class measured no faster than its three launches: it keeps them
KEPT = (BLOCKS[0], BLOCKS[1])


def _blob(kind, block, u8, seed=7):
    import tflite_writer as tw
    shape, E, S, N = block
    elem = tw.UINT8 if u8 else tw.INT8
    rng = np.random.default_rng(seed)
    if kind == "ir":
        return tw.inverted_residual_net(rng, shape, [(E, 3, S, N)], elem=elem, head=10)
    return tw.conv_net(rng, shape, [("conv", E, 1, 1), ("dw", 0, 3, S), ("conv", N, 1, 1)], elem=elem, wmax=40, act_scale=6.0 / 255.0)


def _inputs(m, n, seed):
    """n images: image 0 all-minimum, image 1 all-maximum, the rest random"""
    lo, hi = (0, 256) if m.dtype == np.uint8 else (-128, 128)
    x = np.random.default_rng(seed).integers(lo, hi, (n, m.input_elems), dtype=np.int16).astype(m.dtype)
    x[0], x[1] = lo, hi - 1
    return x


_names = lambda m: [m.op(i)["kernel"] for i in range(m.num_ops)]


@pytest.mark.parametrize("name,kind,block,u8", CASES, ids=[c[0] for c in CASES])
def test_block_is_one_launch_and_equals_the_oracle_every_way(O, name, kind, block, u8):
    import microflow_rs_amd as mf
    blob = _blob(kind, block, u8)
    m = mf.Model(blob)
    m.prepare(1)
    if not ROUTING_SWITCHED:
        names = _names(m)
        if block in KEPT:
            assert not any(k.startswith("block_slice_rt") for k in names), names
        else:
            assert names[0].startswith("block_slice_rt<") and names[1] == FUSED and names[2] == FUSED, names
    om = O.Model(blob)
    x = _inputs(m, BATCH, 11)
    layers = [om.run_quantized(x[i], layers=True)[1] for i in PICK]
    want = om.run_quantized_batch(x[PICK]).reshape(len(PICK), -1)
    got_blk = np.asarray(m.run_until(x, 2)).reshape(BATCH, -1)
    got = np.asarray(m.run_quantized(x)).reshape(BATCH, -1)
    for j, i in enumerate(PICK):                         # the oracle, byte for byte
        assert np.array_equal(got[i], want[j]), i
        assert np.array_equal(got_blk[i], np.asarray(layers[j][2]).reshape(-1)), i
    for setter in (m.set_fusion, m.set_generic):         # fusion off, then every operator generic: every image
        setter(setter == m.set_generic)
        try:
            if setter == m.set_fusion and not ROUTING_SWITCHED:
                assert not any(k.startswith("block_slice_rt") or k == FUSED for k in _names(m)[:3]), _names(m)
            other_blk = np.asarray(m.run_until(x, 2)).reshape(BATCH, -1)
            other = np.asarray(m.run_quantized(x)).reshape(BATCH, -1)
        finally:
            setter(setter != m.set_generic)
        bad = np.flatnonzero((got_blk != other_blk).any(axis=1))
        assert bad.size == 0, (setter.__name__, bad.size, bad[:8])
        assert np.array_equal(got, other), setter.__name__
    for k in range(3):                                   # run_until at each operator of the block
        g = np.asarray(m.run_until(x[PICK[2:]], k)).reshape(2, -1)
        for j in (2, 3):
            assert np.array_equal(g[j - 2], np.asarray(layers[j][k]).reshape(-1)), (k, j)


def test_above_256_images_a_3x3_block_runs_the_launches_it_had():
    """images below one 16-pixel chunk win as one launch only while three launches cannot fill the chip"""
    import torch
    import microflow_rs_amd as mf
    m = mf.Model(_blob("ir", BLOCKS[9], False))
    m.prepare(1)
    x = torch.as_tensor(_inputs(m, 257, 5)).cuda()
    before = m.device_ops()
    a = m.run_until(x[:256], 2).cpu().numpy().reshape(256, -1)
    mid = m.device_ops()
    b = m.run_until(x, 2).cpu().numpy().reshape(257, -1)
    assert ROUTING_SWITCHED or m.device_ops() - mid == mid - before + 2     # two launches more, the same bytes
    assert np.array_equal(b[:256], a)


def test_workgroups_that_walk_several_steps():
    """more steps than the resident workgroups (512 at two per CU): every workgroup walks several, changing between border and interior bands"""
    import re
    import torch
    import microflow_rs_amd as mf
    m = mf.Model(_blob("ir", BLOCKS[5], False))
    m.prepare(1)
    label = m.op(0)["kernel"]
    NB = 4
    if not ROUTING_SWITCHED:
        assert label.startswith("block_slice_rt<"), label
        NB = int(re.search(r";NB(\d+)>", label).group(1))
        assert NB >= 2, label
    batch = -(-1600 // NB) + 3
    xd = torch.as_tensor(_inputs(m, batch, 33)).cuda()
    got = m.run_until(xd, 2).cpu().numpy().reshape(batch, -1)
    m.set_fusion(False)
    try:
        off = m.run_until(xd, 2).cpu().numpy().reshape(batch, -1)
    finally:
        m.set_fusion(True)
    bad = np.flatnonzero((got != off).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:8])
