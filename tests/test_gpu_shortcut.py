"""shortcut_add_rt (k_side_join.hip) on the device: one projection block per case -- a 1x1 Conv2D on the skip edge, two 3x3 main
convolutions, the ADD -- written without a head, so the launch's bytes are the model's output.  Expected tensors: tests/shortcut_ref.py
(the oracle for the convolutions, tests/add_ref.add for the ADD), computed once per case at the largest batch and left unchanged.  Every
case names the kernel that ran: the fused launch where the class is taken, the two launches where it is not -- a silent fallback cannot
pass for the fused kernel.  Comparisons are bit-exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import shortcut_ref as S
from tests.conftest import ROOT, ROUTING_SWITCHED

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))

I8, U8 = 9, 3
BATCHES = (1, 3, 67, 300)       # ragged against the 16-pixel chunk; 300 images are more than one workgroup at every shape
FUSED_SIDE = "(fused into its ADD)"   # the side operator's report; the launch is named at the ADD, where it runs
ADD_ALONE = ("add_c16", "add_c16<fma>")
# (H, W, C, stride, N, in the class)
SHAPES = {
    "8x8x16s2-32": (8, 8, 16, 2, 32, True),
    "7x9x16s2-32": (7, 9, 16, 2, 32, True),      # odd sizes: the last sampled row and column are the image's last
    "6x6x32s1-64": (6, 6, 32, 1, 64, True),
    "4x4x48s2-80": (4, 4, 48, 2, 80, True),      # K not a power of two (one k step, 16 padded bytes); N: a second wave block with one tile
    "2x2x64s2-128": (2, 2, 64, 2, 128, True),
    "8x8x24s2-32": (8, 8, 24, 2, 32, False),     # C outside whole sixteens: two launches
    "8x8x16s2-32wzp": (8, 8, 16, 2, 32, False),  # non-zero filter zero points: two launches
    # the wide end of the class: more than one k step, N split over four waves
    "2x2x128s2-256": (2, 2, 128, 2, 256, True),  # two k steps; four wave blocks of four tiles (ResNet-18's 128 -> 256 shortcut)
    "2x2x192s1-176": (2, 2, 192, 1, 176, True),  # three k steps in the four-step instance; three wave blocks, the fourth wave idle,
                                                 # the third block with three live tiles of four
    "2x2x256s2-144": (2, 2, 256, 2, 144, True),  # four k steps; three wave blocks, the third with one live tile
}
# (swap: the ADD written [side, running]; the ADD's activation; the side convolution's activation)
VARIANTS = [(sw, aa, ca) for sw in (False, True) for aa in ("none", "relu", "relu6") for ca in ("none", "relu")]


def _cases():
    out = []
    for si, name in enumerate(SHAPES):
        for elem in (I8, U8):
            # every variant on the first shape; on the others a walk through them, so that every shape meets both orders, every ADD
            # activation and both convolution activations in one element type or the other
            vs = VARIANTS if si == 0 else [VARIANTS[(5 * si + 7 * k + (elem == U8)) % 12] for k in range(3)]
            for v in vs:
                out.append((name, elem) + v)
    return out


CASES = _cases()
IDS = ["%s-%s-%s-%s-c%s" % (n, "u8" if e == U8 else "i8", "swap" if sw else "plain", aa, ca) for n, e, sw, aa, ca in CASES]


class Block:
    def __init__(self, O, name, elem, swap, add_act, conv_act, side="first"):
        import microflow_rs_amd as mf
        import tflite_writer as tw
        H, W, C, s, N, self.in_class = SHAPES[name]
        self.elem, self.dtype = elem, (np.uint8 if elem == U8 else np.int8)
        seed = 9000 + 17 * list(SHAPES).index(name) + (elem == U8)
        self.in_shape, self.in_q, self.layers = tw.resnet_like_layers(np.random.default_rng(seed), (H, W, C), [(s, N)], elem, head=0, side=side,
                                                                      swap=(0,) if swap else (), add_act=add_act, side_act=conv_act,
                                                                      side_wzp="conv" if name.endswith("wzp") else "none")
        self.side = [i for i, L in enumerate(self.layers) if "side_of" in L][0]
        self.add = len(self.layers) - 1
        self.blob = tw.build_model(self.in_shape, self.in_q, self.layers, elem)
        self.m = mf.Model(self.blob)
        self.m.prepare(1)
        lo = 0 if elem == U8 else -128
        x = np.random.default_rng(seed + 1).integers(lo, lo + 256, (BATCHES[-1], H * W * C), dtype=np.int16)
        x[0], x[1] = lo, lo + 255          # T all-lowest and all-highest: with full-range weights the convolution's byte saturates
        self.x = x.astype(self.dtype)
        self.lo = lo
        self.outs = S.segments(tw, O, self.in_shape, self.in_q, self.layers, elem)(self.x)
        for t in self.outs:
            t.setflags(write=False)
        self.want = self.outs[-1]


_blocks = {}


def _block(O, *key):
    if key not in _blocks:
        _blocks[key] = Block(O, *key)
    return _blocks[key]


def names(m):
    return [m.op(i)["kernel"] for i in range(m.num_ops)]


def _check_names(b):
    ns = names(b.m)
    if ROUTING_SWITCHED:
        return ns
    if b.in_class:
        assert ns[b.add].startswith("shortcut_add_rt<") and ns[b.side] == FUSED_SIDE, ns
    else:
        assert ns[b.side] not in ("", FUSED_SIDE) and not ns[b.side].startswith("shortcut_add_rt") and ns[b.add] in ADD_ALONE, ns
    return ns


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_block_matches_at_every_batch(O, case):
    import torch
    b = _block(O, *case)
    assert b.m.op_source(b.side) == -1 and b.m.op_skip(b.add) == (b.side, 1 if case[2] else 0)
    ns = _check_names(b)
    for n in BATCHES:
        x = torch.as_tensor(b.x[:n]).cuda()
        got = b.m.run_quantized(x).cpu().numpy().reshape(n, -1)
        bad = np.argwhere(got != b.want[:n])
        assert bad.shape[0] == 0, (n, ns, int(bad.shape[0]), bad[:6].tolist())
    # ... the side operator's own tensor (run_until at its index: computed from the model input) and the main chain behind it
    for i in range(b.m.num_ops):
        got = np.asarray(b.m.run_until(b.x[:3], i)).reshape(3, -1)
        assert np.array_equal(got, b.outs[i][:3]), ("run_until", i, ns)


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_convolution_saturates_on_the_extreme_rows(O, name):
    """what the first two rows are for: the expected side tensor of the all-lowest / all-highest input has bytes at BOTH ends of the
    type, so the ADD meets operands that saturated in the convolution"""
    b = _block(O, name, I8, False, "none", "none")
    s = np.asarray(b.outs[b.side][:2]).astype(np.int64)
    assert (s == b.lo).any() and (s == b.lo + 255).any(), ((s == b.lo).mean(), (s == b.lo + 255).mean())


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("side", ["first", "last"])
def test_side_position_fusion_off_and_generic(O, name, side):
    """the side convolution first and last in file order give the same bytes; so do the two launches (fusion off) and the generic kernels"""
    b = _block(O, name, I8, True, "relu", "none", side)
    first = _block(O, name, I8, True, "relu", "none", "first")
    assert np.array_equal(b.want, first.want)
    _check_names(b)
    n = 67
    got = np.asarray(b.m.run_quantized(b.x[:n])).reshape(n, -1)
    assert np.array_equal(got, b.want[:n])
    for mode in ("set_fusion", "set_generic"):
        getattr(b.m, mode)(mode == "set_generic")
        try:
            ns = names(b.m)
            assert not ns[b.add].startswith("shortcut_add_rt") and ns[b.side] not in ("", FUSED_SIDE), ns
            got = np.asarray(b.m.run_quantized(b.x[:n])).reshape(n, -1)
        finally:
            getattr(b.m, mode)(mode != "set_generic")
        assert np.array_equal(got, b.want[:n]), (mode, ns)


@pytest.mark.parametrize("name", ["7x9x16s2-32", "4x4x48s2-80"])
@pytest.mark.parametrize("n", [1, 67])
def test_guard_bytes_around_the_output_stay(O, name, n):
    """the launch writes the caller's aligned buffer directly (an i8 model): 256 bytes in front of and behind it are as they were"""
    import torch
    b = _block(O, name, I8, False, "relu6", "relu")
    G = 256
    elems = b.m.output_elems
    buf = torch.full((G + n * elems + G,), 0x5A, dtype=torch.int8, device="cuda")
    out = buf[G:G + n * elems].view(n, elems)
    assert out.data_ptr() % 16 == 0
    b.m.run_quantized(torch.as_tensor(b.x[:n]).cuda(), out=out)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:G] == 0x5A).all() and (h[G + n * elems:] == 0x5A).all()
    assert np.array_equal(h[G:G + n * elems].reshape(n, -1), b.want[:n])


CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import microflow_rs_amd as mf
m = mf.Model(open(sys.argv[2], "rb").read())
m.prepare(1)
x = np.load(sys.argv[3])
ns = [m.op(i)["kernel"] for i in range(m.num_ops)]
assert not any(n.startswith("shortcut_add_rt") for n in ns), ns
np.save(sys.argv[4], np.asarray(m.run_quantized(x)).reshape(len(x), -1))
print("|".join(ns))
"""


def test_the_dev_switch_gives_two_launches_and_the_same_bytes(O, tmp_path):
    b = _block(O, "8x8x16s2-32", I8, False, "relu", "none")
    paths = [str(tmp_path / f) for f in ("m.tflite", "x.npy", "y.npy")]
    with open(paths[0], "wb") as f:
        f.write(b.blob)
    np.save(paths[1], b.x[:67])
    env = dict(os.environ, MF_DEV="1", MF_NO_SHORTCUT_ADD="1")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT] + paths, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().split("|")[b.add] in ADD_ALONE, r.stdout
    assert np.array_equal(np.load(paths[2]), b.want[:67])
