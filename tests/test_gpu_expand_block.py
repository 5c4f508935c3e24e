"""Conv2D 1x1 expand + DepthwiseConv2D 3x3 + Conv2D 1x1 project blocks (the tensor inside the widest) as one block_band_rt launch
(k_block_band.hip): routing, bit-exactness against the CPU oracle and against the operators' own launches and the generic kernels on
a ragged batch, every operator of the block through run_until, the bytes around the output, an unaligned input pointer, hipGraph
replay, workgroups that walk many steps, the batch limit of the small blocks, a four-block model, the blocks that must keep their
launches and the MF_NO_EXPAND_BLOCK switch.  The inputs are checked too (on the oracle's layers): a block whose inner tensors are constant would pass whatever runs."""
import ctypes
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
GUARD = 64
BATCH = 37
# (H, W, C), E, S, N: what each is the smallest case of
BLOCKS = [
    ((6, 6, 8), 32, 1, 8),        # one band, one k step, K padded from 8, N below one tile
    ((9, 7, 16), 64, 1, 24),      # odd H and W: ragged 16-pixel chunks in both GEMM phases, CX = 1; 1.5 output tiles
    ((13, 11, 12), 48, 1, 20),    # C and N that are only multiples of 4; an unaligned image size
    ((10, 10, 24), 144, 2, 32),   # stride 2, three k steps of E on the four-k-step instance
    ((40, 40, 16), 96, 1, 16),    # does not fit as one band: NB >= 2, the halo rows computed twice, border and interior bands
    ((34, 30, 32), 256, 2, 64),   # E at the limit, stride 2 with bands, two output tiles per block
]
# name, builder ("ir": inverted_residual_net; "cn": conv_net with wmax = 40 and act_scale = 6 / 255, the saturating-pack epilogue), block, u8
CASES = [("%dx%dx%d-%d%s-%d-%s" % (s + (E, "s2" if S == 2 else "", N, "u8" if u8 else "i8")), "ir", (s, E, S, N), u8) for (s, E, S, N) in BLOCKS for u8 in (False, True)]
CASES += [("10x10x24-144s2-32-sat", "cn", BLOCKS[3], False), ("40x40x16-96-16-sat", "cn", BLOCKS[4], False)]
IDS = [c[0] for c in CASES]
WHOLE = [op for (E, S, N) in ((96, 1, 24), (144, 2, 32), (192, 1, 32), (192, 2, 64)) for op in (("conv", E, 1, 1), ("dw", 0, 3, S), ("conv", N, 1, 1))]


def _block_blob(kind, block, u8, seed=7):
    import tflite_writer as tw
    shape, E, S, N = block
    elem = tw.UINT8 if u8 else tw.INT8
    rng = np.random.default_rng(seed)
    if kind == "ir":
        return tw.inverted_residual_net(rng, shape, [(E, 3, S, N)], elem=elem, head=10)
    return tw.conv_net(rng, shape, [("conv", E, 1, 1), ("dw", 0, 3, S), ("conv", N, 1, 1)], elem=elem, wmax=40, act_scale=6.0 / 255.0)


def _whole_blob(u8, seed=7):
    import tflite_writer as tw
    return tw.conv_net(np.random.default_rng(seed), (28, 28, 16), WHOLE, elem=tw.UINT8 if u8 else tw.INT8, head=10, act_scale=6.0 / 255.0)


def _inputs(m, n, seed):
    """n images: image 0 all-minimum, image 1 all-maximum, the rest random"""
    lo, hi = (0, 256) if m.dtype == np.uint8 else (-128, 128)
    x = np.random.default_rng(seed).integers(lo, hi, (n, m.input_elems), dtype=np.int16).astype(m.dtype)
    x[0], x[1] = lo, hi - 1
    return x


def _names(m):
    return [m.op(i)["kernel"] for i in range(m.num_ops)]


def _until_into(m, xd, last_op, out):
    """mf_model_run_until with the caller's device pointers (Model.run_until allocates its own output)"""
    import torch
    from microflow_rs_amd import _lib
    _lib.check(_lib.lib().mf_model_set_stream(m._h, torch.cuda.current_stream().cuda_stream))
    _lib.check(_lib.lib().mf_model_run_until(m._h, ctypes.c_void_p(xd.data_ptr()), xd.numel() // m.input_elems, int(last_op), ctypes.c_void_p(out.data_ptr()),
                                             _lib.MF_MEM_DEVICE))
    torch.cuda.synchronize()


def _spread(t):
    """distinct byte values of a tensor, and the share of its bytes at its minimum or maximum"""
    t = np.asarray(t).reshape(-1)
    return np.unique(t).size, float(((t == t.min()) | (t == t.max())).mean())


PICK = [0, 1, 2, BATCH - 1]


class Case:
    def __init__(self, O, blob, nblocks):
        import microflow_rs_amd as mf
        self.blob = blob
        self.m = mf.Model(blob)
        self.m.prepare(1)
        self.om = O.Model(blob)
        self.x = _inputs(self.m, BATCH, 11)
        self.last = 3 * nblocks - 1                      # the last block's project
        self.layers = [self.om.run_quantized(self.x[i], layers=True)[1] for i in PICK]   # computed once, never changed
        self.want = self.om.run_quantized_batch(self.x[PICK]).reshape(len(PICK), -1)


_cases = {}


@pytest.fixture(params=range(len(CASES)), ids=IDS)
def case(request, O):
    i = request.param
    if i not in _cases:
        name, kind, block, u8 = CASES[i]
        _cases[i] = Case(O, _block_blob(kind, block, u8), 1)
    return _cases[i]


_wholes = {}


@pytest.fixture(params=[False, True], ids=["i8", "u8"])
def whole(request, O):
    if request.param not in _wholes:
        _wholes[request.param] = Case(O, _whole_blob(request.param), 4)
    return _wholes[request.param]


def _check_inputs(c, nblocks):
    """the oracle's expand, depthwise and project tensors of each of the two random images: at least 32 distinct byte values and at most
    0.80 of the bytes at the minimum or maximum, each tensor"""
    for k in range(3 * nblocks):
        for j in (2, 3):
            distinct, share = _spread(c.layers[j][k])
            assert distinct >= 32 and share <= 0.80, (k, j, distinct, share)


def _check_every_way(c, first_ops):
    """the ragged batch: default routing == fusion off == all-generic on every image, at the last block's output and at the model's;
    the oracle on images 0 (all lo), 1 (all hi - 1), 2 and the last; run_until at every operator of every block"""
    m = c.m
    got_blk = np.asarray(m.run_until(c.x, c.last)).reshape(BATCH, -1)
    got = np.asarray(m.run_quantized(c.x)).reshape(BATCH, -1)
    for j, i in enumerate(PICK):
        assert np.array_equal(got[i], c.want[j]), i
        assert np.array_equal(got_blk[i], np.asarray(c.layers[j][c.last]).reshape(-1)), i
    for setter in (m.set_fusion, m.set_generic):
        setter(setter == m.set_generic)
        try:
            if setter == m.set_fusion and not ROUTING_SWITCHED:
                assert not any(k.startswith("block_band_rt") or k == FUSED for k in _names(m)[:c.last + 1]), _names(m)
            other_blk = np.asarray(m.run_until(c.x, c.last)).reshape(BATCH, -1)
            other = np.asarray(m.run_quantized(c.x)).reshape(BATCH, -1)
        finally:
            setter(setter != m.set_generic)
        bad = np.flatnonzero((got_blk != other_blk).any(axis=1))
        assert bad.size == 0, (setter.__name__, bad.size, bad[:8])
        assert np.array_equal(got, other), setter.__name__
    for k in range(c.last + 1):                          # the expand and the depthwise run the lower level; the project the block
        g = np.asarray(m.run_until(c.x[PICK[2:]], k)).reshape(2, -1)
        for j in (2, 3):
            assert np.array_equal(g[j - 2], np.asarray(c.layers[j][k]).reshape(-1)), (k, j)


# ---- 1. the single blocks ---------------------------------------------------------------------------------------------------
def test_block_is_one_launch_and_equals_the_oracle_every_way(case):
    if not ROUTING_SWITCHED:
        names = _names(case.m)
        assert names[0].startswith("block_band_rt<") and names[1] == FUSED and names[2] == FUSED, names
    _check_inputs(case, 1)
    _check_every_way(case, [0])


def test_block_output_guards_unaligned_input_and_graph_replay(case):
    import torch
    m, c = case.m, case
    n = 6
    x = torch.as_tensor(c.x[:n]).cuda()
    elems = m.op(2)["out_elems"]
    dt = torch.uint8 if m.dtype == np.uint8 else torch.int8
    want = np.asarray(m.run_until(c.x[:n], 2)).reshape(-1)
    buf = torch.full((GUARD + n * elems + GUARD,), 0x5A, dtype=dt, device="cuda")
    out = buf[GUARD:GUARD + n * elems]
    _until_into(m, x, 2, out)
    b = buf.cpu().numpy()
    assert np.array_equal(b[GUARD:GUARD + n * elems], want)
    assert (b[:GUARD] == 0x5A).all() and (b[GUARD + n * elems:] == 0x5A).all()     # 64 bytes in front and behind: untouched
    # an input view offset by four bytes: the same bytes
    flat = c.x[:n].reshape(-1)
    raw = torch.zeros(flat.size + 64, dtype=dt, device="cuda")
    view = raw[4:4 + flat.size]
    view.copy_(torch.as_tensor(flat))
    assert view.data_ptr() % 16 == 4
    buf.fill_(0x5A)
    _until_into(m, view, 2, out)
    assert np.array_equal(buf.cpu().numpy(), b)
    # hipGraph: eager, captured + replayed, replayed -- each into a zeroed output
    m.set_graph(True)
    try:
        before = m.graph_launches
        for it in range(3):
            out.zero_()
            _until_into(m, x, 2, out)
            assert np.array_equal(out.cpu().numpy(), want), it
        assert m.graph_launches - before == 2
    finally:
        m.set_graph(False)


def test_the_cases_report_both_epilogue_modes(O):
    """what the models report, not what the table says: the inverted_residual_net blocks run the v_med3 epilogue (relu6 inside the
    range), the conv_net ones the saturating pack (relu6 = the whole range)"""
    if ROUTING_SWITCHED:
        return
    for i in range(len(CASES)):
        if i not in _cases:
            _cases[i] = Case(O, _block_blob(CASES[i][1], CASES[i][2], CASES[i][3]), 1)
    seen = {_cases[i].m.op_epilogue_mode(0) for i in range(len(CASES)) if _names(_cases[i].m)[0].startswith("block_band_rt<")}
    assert {1, 2} <= seen, seen


def test_above_its_batch_limit_a_small_block_runs_the_launches_it_had(O):
    """One k step of E is a class in which the one launch wins only while three launches cannot fill the chip: up to
    512 / NB images it runs, above that the operators' own launches do -- two launches more, the same bytes."""
    import torch
    import microflow_rs_amd as mf
    blob = _block_blob("ir", BLOCKS[0], False)
    m = mf.Model(blob)
    m.prepare(1)
    x = torch.as_tensor(_inputs(m, 513, 5)).cuda()
    counts, outs = [], []
    for n in (512, 513):
        before = m.device_ops()
        outs.append(m.run_until(x[:n], 2).cpu().numpy().reshape(n, -1))
        counts.append(m.device_ops() - before)
    if not ROUTING_SWITCHED:
        assert _names(m)[0].startswith("block_band_rt<6x6x8-32-8;RB8;NB1>"), _names(m)
        assert counts[1] == counts[0] + 2, counts
    assert np.array_equal(outs[1][:512], outs[0])
    m.set_fusion(False)
    try:
        assert np.array_equal(m.run_until(x, 2).cpu().numpy().reshape(513, -1), outs[1])
    finally:
        m.set_fusion(True)


# ---- 2. several steps per workgroup ---------------------------------------------------------------------------------------
def test_workgroups_that_walk_many_steps(O):
    """more steps than the 512 workgroups two per CU can launch: every workgroup changes between border and interior bands, which is
    where a tile row left over from the step before would show"""
    import torch
    import microflow_rs_amd as mf
    blob = _block_blob("ir", BLOCKS[4], False)
    m = mf.Model(blob)
    m.prepare(1)
    label = m.op(0)["kernel"]
    NB = 2
    if not ROUTING_SWITCHED:
        assert label.startswith("block_band_rt<"), label
        NB = int(re.search(r";NB(\d+)>", label).group(1))
        assert NB >= 2, label
    batch = -(-1100 // NB) + 3
    x = _inputs(m, batch, 33)
    xd = torch.as_tensor(x).cuda()
    got = m.run_until(xd, 2).cpu().numpy().reshape(batch, -1)
    m.set_fusion(False)
    try:
        off = m.run_until(xd, 2).cpu().numpy().reshape(batch, -1)
    finally:
        m.set_fusion(True)
    bad = np.flatnonzero((got != off).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:8])


# ---- 3. a model of four blocks ----------------------------------------------------------------------------------------------
def test_whole_model_is_four_block_launches_and_equals_the_oracle_every_way(whole):
    if not ROUTING_SWITCHED:
        names = _names(whole.m)
        for i in (0, 3, 6, 9):
            assert names[i].startswith("block_band_rt<") and names[i + 1] == FUSED and names[i + 2] == FUSED, names
        assert sum(k.startswith("block_band_rt<") for k in names) == 4, names
    _check_inputs(whole, 4)
    _check_every_way(whole, [0, 3, 6, 9])


# ---- 4. what must not move, and the switch ------------------------------------------------------------------------------------
# name -> python expression of the blob (tw = tflite_writer, rng = a fresh default_rng(7)).  None of these is a block of this route:
# E = N, E no multiple of 16, E beyond 256, a 5x5 depthwise, filter zero points, an odd width at stride 2, a MobileNet-v1-shaped
# model (channel counts never shrink), and the two classes measured no faster as one launch.
KEEP = {
    "E=N": "tw.inverted_residual_net(rng, (12, 12, 16), [(64, 3, 1, 64)])",
    "E=36": "tw.inverted_residual_net(rng, (12, 12, 12), [(36, 3, 1, 12)])",
    "E=272": "tw.inverted_residual_net(rng, (12, 12, 16), [(272, 3, 1, 16)])",
    "dw5x5": "tw.inverted_residual_net(rng, (12, 12, 16), [(64, 5, 1, 16)])",
    "wzp": "tw.inverted_residual_net(rng, (12, 12, 16), [(64, 3, 1, 16)], wzp_nonzero=True)",
    "9x9x16-64s2-16": "tw.inverted_residual_net(rng, (9, 9, 16), [(64, 3, 2, 16)])",
    "person_detect_like": "tw.person_detect_like(rng, 96, 0.75)",
    # excluded on speed grounds (not faster than the launches they replace by more than the spread of the repeats)
    "56x56x24-144-24-slower": "tw.conv_net(rng, (56, 56, 24), [('conv', 144, 1, 1), ('dw', 0, 3, 1), ('conv', 24, 1, 1)], act_scale=6.0 / 255.0)",
    "6x6x32-192s2-64-slower": "tw.conv_net(rng, (6, 6, 32), [('conv', 192, 1, 1), ('dw', 0, 3, 2), ('conv', 64, 1, 1)], act_scale=6.0 / 255.0)",
}
CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import microflow_rs_amd as mf
import tflite_writer as tw
KEEP, WHOLE = %r, %r
for name in sorted(KEEP):
    rng = np.random.default_rng(7)
    m = mf.Model(eval(KEEP[name]))
    m.prepare(1)
    print("KERNELS", name, "|".join(m.op(i)["kernel"] for i in range(m.num_ops)))
m = mf.Model(tw.conv_net(np.random.default_rng(7), (28, 28, 16), WHOLE, head=10, act_scale=6.0 / 255.0))
m.prepare(1)
print("KERNELS", "whole", "|".join(m.op(i)["kernel"] for i in range(m.num_ops)))
x = np.random.default_rng(6).integers(-128, 128, (5, m.input_elems)).astype(np.int8)
np.save(sys.argv[1], np.concatenate([np.asarray(m.run_until(x, 11)).reshape(5, -1), np.asarray(m.run_quantized(x)).reshape(5, -1)], axis=1))
'''


@pytest.fixture(scope="module")
def children():
    """the same models in two child processes (the switches are read once per process): default routing, and MF_DEV=1 MF_NO_EXPAND_BLOCK=1"""
    code = CHILD % (ROOT, os.path.join(ROOT, "tools"), KEEP, WHOLE)
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        for sw in (None, "1"):
            env = dict(os.environ)
            for k in [k for k in env if k.startswith("MF_")]:
                del env[k]
            if sw:
                env.update(MF_DEV="1", MF_NO_EXPAND_BLOCK="1")
            path = os.path.join(tmp, "out%d.npy" % len(res))
            r = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
            assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
            names = {}
            for l in r.stdout.splitlines():
                if l.startswith("KERNELS "):
                    _, name, ks = l.split(" ", 2)
                    names[name] = ks.split("|")
            res.append((names, np.load(path)))
    return res


@pytest.mark.parametrize("name", sorted(KEEP))
def test_blocks_outside_the_route_keep_their_launches(children, name):
    (on, _), (off, _) = children
    assert on[name] == off[name], (on[name], off[name])
    assert not any(k.startswith("block_band_rt") for k in on[name]), on[name]


def test_no_expand_block_switch_goes_back_to_the_operators(children):
    (on, out_on), (off, out_off) = children
    assert sum(k.startswith("block_band_rt<") for k in on["whole"]) == 4, on["whole"]
    assert not any(k.startswith("block_band_rt") for k in off["whole"]), off["whole"]
    assert on["whole"][12:] == off["whole"][12:]
    assert np.array_equal(out_on, out_off)
