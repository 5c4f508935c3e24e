"""side_concat_rt (k_side_join.hip) on the device: one fire module per case -- a squeeze 1x1, the 1x1 expand on the skip edge, the
3x3 expand on the main chain, their CONCATENATION -- written without a head, so the launch's bytes are the model's output.  Expected
tensors: tests/concat_ref.py (the oracle for the convolutions, concat_ref.concat for the join), computed once per case on UNIQUE rows
that the larger batches repeat, and left unchanged.  Every case names the kernel that ran: the fused launch where the class is taken,
the two launches where it is not -- a silent fallback cannot pass for the fused kernel.  Comparisons are bit-exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import concat_ref as CR
from tests.conftest import ROOT, ROUTING_SWITCHED

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))

I8, U8 = 9, 3
BATCHES = (1, 3, 67, 300)       # 3 and 67 leave a ragged last 16-row chunk at every image size used here
UNIQUE = 20                     # distinct inputs; batch row i is unique row i % UNIQUE
FUSED_SIDE = "(fused into its CONCATENATION)"   # the side operator's report; the launch is named at the join, where it runs
CIN = 16                        # the fire's input channels (the squeeze's input)
# C -> N + Cb: the side convolution's input and output channels and the running slice = (squeeze, expand 1x1, expand 3x3)
SHAPES = {
    "16-16+16": (16, 16, 16),       # the minimal case
    "48-192+192": (48, 192, 192),   # one k step, three wave blocks' worth of N
    "64-256+256": (64, 256, 256),   # the widest fire
    "128-144+16": (128, 144, 16),   # two k steps, a partly idle last block, a narrow running slice
    "192-176+80": (192, 176, 80),   # three k steps
    "256-32+240": (256, 32, 240),   # four k steps, an 8-byte-per-lane store
}
IMAGES = {"2x2": (2, 1), "3x3": (3, 1), "4x4s2": (4, 2)}   # (side, the expands' stride)
# (the join reads [e1, e3]; the convolutions' activation; which slices carry the join's output quantisation (e1, e3))
VARIANTS = [(f, a, i) for f in (True, False) for a in ("relu", "relu6", "none") for i in ((True, True), (False, True), (True, False), (False, False))]


def _cases():
    out = []
    for si, name in enumerate(SHAPES):
        for ii, img in enumerate(IMAGES):
            for elem in (I8, U8):
                # every variant on the minimal shape at 2x2; elsewhere a walk through them, so that every shape meets both operand
                # orders, every activation and every identity pattern in one element type or image or the other
                vs = VARIANTS if (si == 0 and ii == 0) else [VARIANTS[(5 * si + 7 * ii + 11 * (elem == U8)) % len(VARIANTS)]]
                for v in vs:
                    out.append((name, img, elem) + v)
    return out


CASES = _cases()
IDS = ["%s-%s-%s-%s-%s-%s" % (n, img, "u8" if e == U8 else "i8", "e1first" if f else "e3first", a, "".join("ir"[not k] for k in i))
       for n, img, e, f, a, i in CASES]


class Fire:
    def __init__(self, O, name, img, elem, e1_first, act, identity):
        import microflow_rs_amd as mf
        import tflite_writer as tw
        S, E1, E3 = SHAPES[name]
        side, stride = IMAGES[img]
        self.elem, self.dtype = elem, (np.uint8 if elem == U8 else np.int8)
        lo = 0 if elem == U8 else -128
        seed = 12000 + 37 * list(SHAPES).index(name) + 5 * list(IMAGES).index(img) + (elem == U8)
        rng = np.random.default_rng(seed)
        self.in_shape = (1, side, side, CIN)
        self.in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(lo + 20, lo + 236)))
        self.layers, out_shape, _ = tw.fire_layers(rng, (side, side, CIN), self.in_q, (S, E1, E3, stride, "13"), elem=elem, act=act,
                                                   e1_first=e1_first, identity=identity)
        self.sq, self.side, self.main, self.join = 0, 1, 2, 3
        self.want_name = "side_concat_rt<%d,%d,%d%s>" % (S, E1, E3, ",s2" if stride == 2 else "")
        self.blob = tw.build_model(self.in_shape, self.in_q, self.layers, elem)
        self.m = mf.Model(self.blob)
        self.m.prepare(1)
        assert self.m.output_shape == (1,) + tuple(out_shape)
        x = np.random.default_rng(seed + 1).integers(lo, lo + 256, (UNIQUE, side * side * CIN), dtype=np.int16)
        x[0], x[1] = lo, lo + 255          # the input all-lowest and all-highest: with full-range weights the convolutions saturate
        self.x = x.astype(self.dtype)
        self.lo = lo
        self.outs = CR.segments(tw, O, self.in_shape, self.in_q, self.layers, elem)(self.x)
        for t in self.outs:
            t.setflags(write=False)
        self.want = self.outs[-1]

    def rows(self, n):
        idx = np.arange(n) % UNIQUE
        return self.x[idx], self.want[idx]


_fires = {}


def _fire(O, *key):
    if key not in _fires:
        _fires[key] = Fire(O, *key)
    return _fires[key]


def names(m):
    return [m.op(i)["kernel"] for i in range(m.num_ops)]


def _check_names(b):
    ns = names(b.m)
    if not ROUTING_SWITCHED:
        assert ns[b.join] == b.want_name and ns[b.side] == FUSED_SIDE, ns
    return ns


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fire_matches_at_every_batch(O, case):
    import torch
    b = _fire(O, *case)
    assert b.m.op_source(b.side) == 0 and b.m.op_skip(b.join) == (b.side, 1 if case[3] else 0)
    ca, cb = b.m.op_constants(b.join)[:2]
    e1_c, e3_c = (ca[0], cb[0]) if case[3] else (cb[0], ca[0])
    assert (e1_c == 1.0, e3_c == 1.0) == case[5]            # the slices requantise exactly where the case says so
    ns = _check_names(b)
    for n in BATCHES:
        x, want = b.rows(n)
        got = b.m.run_quantized(torch.as_tensor(x).cuda()).cpu().numpy().reshape(n, -1)
        bad = np.argwhere(got != want)
        assert bad.shape[0] == 0, (n, ns, int(bad.shape[0]), bad[:6].tolist())
    # the two launches of the same build: the side convolution's own, then concat_c4 -- and the byte-wise kernels
    x, want = b.rows(67)
    for mode in ("set_fusion", "set_generic"):
        getattr(b.m, mode)(mode == "set_generic")
        try:
            off = names(b.m)
            assert not off[b.join].startswith("side_concat_rt") and off[b.side] not in ("", FUSED_SIDE), off
            assert off[b.join] == ("concat_generic" if mode == "set_generic" else "concat_c4<v16>"), off
            got = np.asarray(b.m.run_quantized(x)).reshape(67, -1)
        finally:
            getattr(b.m, mode)(mode != "set_generic")
        assert np.array_equal(got, want), (mode, off)
    # ... the side operator's own tensor (run_until at its index: computed from the squeeze's output) and every other operator
    for i in range(b.m.num_ops):
        got = np.asarray(b.m.run_until(b.x[:3], i)).reshape(3, -1)
        assert np.array_equal(got, b.outs[i][:3]), ("run_until", i, ns)


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_convolutions_saturate_and_the_join_requantises_inside_the_range(O, name):
    """what the first two rows are for: both expands have bytes at BOTH ends of the type without an activation, so the join meets
    operands that saturated in the convolution"""
    b = _fire(O, name, "2x2", I8, True, "none", (False, False))
    for k in (b.side, b.main):
        s = np.asarray(b.outs[k][:2]).astype(np.int64)
        assert (s == b.lo).any() and (s == b.lo + 255).any(), (k, (s == b.lo).mean(), (s == b.lo + 255).mean())


@pytest.mark.parametrize("name,img", [("16-16+16", "3x3"), ("128-144+16", "4x4s2"), ("256-32+240", "2x2")])
@pytest.mark.parametrize("n", [1, 67])
def test_guard_bytes_around_the_output_stay(O, name, img, n):
    """the launch writes the caller's aligned buffer directly (an i8 model): 256 bytes in front of and behind it are as they were"""
    import torch
    b = _fire(O, name, img, I8, False, "relu", (True, False))
    _check_names(b)
    G = 256
    elems = b.m.output_elems
    x, want = b.rows(n)
    buf = torch.full((G + n * elems + G,), 0x5A, dtype=torch.int8, device="cuda")
    out = buf[G:G + n * elems].view(n, elems)
    assert out.data_ptr() % 16 == 0
    b.m.run_quantized(torch.as_tensor(x).cuda(), out=out)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:G] == 0x5A).all() and (h[G + n * elems:] == 0x5A).all()
    assert np.array_equal(h[G:G + n * elems].reshape(n, -1), want)


@pytest.mark.parametrize("form", ["wzp", "c24", "cb24", "k3"])
def test_outside_the_class_two_launches_run(O, form):
    """filter zero points, channels outside whole sixteens and a 3x3 side convolution load and run the two launches"""
    import microflow_rs_amd as mf
    import tflite_writer as tw
    fire = {"wzp": (16, 32, 48), "c24": (24, 32, 48), "cb24": (16, 32, 24), "k3": (16, 32, 48, 1, "31")}[form]
    rng = np.random.default_rng(77)
    in_q = (0.05, 3)
    ls, _, _ = tw.fire_layers(rng, (3, 3, CIN), in_q, fire, side_wzp="conv" if form == "wzp" else "none")
    m = mf.Model(tw.build_model((1, 3, 3, CIN), in_q, ls, I8))
    m.prepare(1)
    ns = names(m)
    if not ROUTING_SWITCHED:
        assert ns[3] == ("concat_c4<v8>" if form == "cb24" else "concat_c4<v16>") and ns[1] not in ("", FUSED_SIDE), ns
    x = np.random.default_rng(78).integers(-128, 128, (19, 3 * 3 * CIN)).astype(np.int8)
    outs = CR.segments(tw, O, (1, 3, 3, CIN), in_q, ls, I8)(x)
    for i in range(m.num_ops):
        assert np.array_equal(np.asarray(m.run_until(x, i)).reshape(19, -1), outs[i]), (i, ns)


CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import microflow_rs_amd as mf
m = mf.Model(open(sys.argv[2], "rb").read())
m.prepare(1)
x = np.load(sys.argv[3])
ns = [m.op(i)["kernel"] for i in range(m.num_ops)]
assert not any(n.startswith("side_concat_rt") for n in ns), ns
np.save(sys.argv[4], np.asarray(m.run_quantized(x)).reshape(len(x), -1))
print("|".join(ns))
"""


def test_the_dev_switch_gives_two_launches_and_the_same_bytes(O, tmp_path):
    b = _fire(O, "48-192+192", "4x4s2", I8, True, "relu", (True, True))
    paths = [str(tmp_path / f) for f in ("m.tflite", "x.npy", "y.npy")]
    with open(paths[0], "wb") as f:
        f.write(b.blob)
    x, want = b.rows(67)
    np.save(paths[1], x)
    env = dict(os.environ, MF_DEV="1", MF_NO_SIDE_CONCAT="1")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT] + paths, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().split("|")[b.join] == "concat_c4<v16>", r.stdout
    assert np.array_equal(np.load(paths[2]), want)
