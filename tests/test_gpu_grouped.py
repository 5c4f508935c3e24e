"""Grouped Conv2D: conv_grp_rt (k_conv_grp.hip), the block-diagonal twin on the dense routes and conv2d_generic with groups, each byte for
byte against tests/dilated_ref.conv on tests/grouped_ref.expand's dense filter, through ops.prepare_conv_2d.  Every case names what it
can break.  Constants as tests/test_gpu_dilated.py's, c1 from the fan-in of a GROUP (half the outputs inside the clamp); seeds per case."""
import zlib

import numpy as np
import pytest

from tests import dilated_ref as D
from tests import grouped_ref as R
from tests.test_gpu_tconv import mf  # noqa: F401  (the module-scoped fixture: the package on a machine with a GPU)

pytestmark = pytest.mark.gpu
f32 = np.float32

#             H   W   C    N   KH KW  s  G  same  dil batch
SHAPES = {
    "g1":  (7,  7,  16,  16,  3, 3, 1, 4, True,  1, 5),   # four groups packed in one tile, halo on four sides; a ragged last step
    "g2":  (7,  7,  32,  32,  3, 3, 1, 2, True,  1, 2),   # one group per tile, b128 operand
    "g3":  (5,  5,  64,  64,  3, 3, 1, 2, True,  1, 2),   # two tiles per group, two 16-byte chunks per tap
    "g4":  (6,  9,  24,  36,  3, 3, 1, 3, False, 1, 2),   # Ng = 12: dead columns, N % 16 != 0, C % 16 != 0: the dword gather
    "g5":  (6,  6,  8,   40,  3, 3, 1, 2, True,  1, 2),   # Ng = 20: a full and a ragged tile per group
    "g6":  (8,  8,  8,   8,   2, 2, 2, 2, False, 1, 2),   # even filter, K = 16 padded to 64
    "g7":  (5,  6,  32,  64,  1, 1, 1, 8, True,  1, 2),   # the grouped pointwise: K = 4 per group, two groups per tile
    "g8":  (24, 24, 64,  64,  3, 3, 1, 4, True,  1, 3),   # row bands
    "g9":  (4,  4,  256, 256, 3, 3, 1, 2, True,  1, 2),   # N slices
    "g10": (7,  7,  18,  12,  3, 3, 1, 3, True,  1, 2),   # Cg = 6: the twin
    "g11": (7,  7,  16,  16,  3, 3, 1, 4, True,  3, 2),   # dilation with groups: the twin or generic, exact
    "g12": (6,  6,  8,   16,  3, 3, 1, 8, True,  1, 2),   # Cg = 1: the twin
    "g13": (5,  6,  32,  32,  1, 1, 1, 2, True,  1, 2),   # a 1x1 with G <= 3: the twin on the pointwise kernels, measured faster
    "g14": (5,  5,  24,  24,  3, 3, 1, 6, True,  1, 2),   # a ragged packed tile: 4 + 2 groups, the second tile's span reaches past channel C
}
TWIN = ("g10", "g11", "g12", "g13")
PLAN = {"g8": lambda p: p["bands"] > 1, "g9": lambda p: p["slices"] > 1, "g1": lambda p: 1 < p["images"] and 5 % p["images"] != 0}
VARIATIONS = [("worst", dict(worst=True)), ("u8", dict(u8=True)), ("relu", dict(act=1)), ("relu6", dict(act=3)), ("nobias", dict(bias=False)), ("wzp", dict(wz=True))]
CASES = [(k, k, {}) for k in SHAPES] + [("%s-%s" % (k, n), k, v) for k in ("g1", "g3", "g7", "g14") for n, v in VARIATIONS]   # (g1, g3 read b128; g7, g14 the dword gather)


def build(name, key, u8=False, act=0, bias=True, wz=False, worst=False, batch=None):
    """-> (prepare(mf) giving the operator, x, the contract's output)"""
    H, W, C, N, KH, KW, s, G, same, dil, b0 = SHAPES[key]
    batch, Cg = batch or b0, C // G
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    dt, off = (np.uint8, 128) if u8 else (np.int8, 0)
    OH, OW = D.geometry(H, W, KH, KW, (s, s), (dil, dil), same)[:2]
    x = (rng.integers(-128, 128, (batch, H, W, C)) + off).astype(dt)
    w = (rng.integers(-127, 128, (N, KH, KW, Cg)) + off).astype(dt)
    wzp = (np.where(rng.integers(0, 2, N) > 0, 1, -1) * rng.integers(1, 25, N) if wz else np.zeros(N, np.int64)) + off
    izp, ozp, oscale = int(rng.integers(-20, 21)) + off, int(rng.integers(-20, 21)) + off, f32(0.0235294122)
    c0 = rng.uniform(-30, 30, N).astype(f32) if bias else np.zeros(N, f32)
    taps = D.mean_taps(H, W, KH, KW, (s, s), (dil, dil), same)
    c1 = (rng.uniform(0.8, 1.25, N) * 190.0 / (74.0 * 73.3 * np.sqrt(taps * Cg))).astype(f32)   # (the fan-in of a group)
    if worst:   # input all -128, weights all 127, unit constants: the accumulator bound, saturation
        x[:], w[:], izp, c0, c1 = -128, 127, 0, np.zeros(N, f32), np.ones(N, f32)
    want = D.conv(x, R.expand(w, wzp.astype(dt), G, C), izp, wzp, (s, s), (dil, dil), same, c0, c1, ozp, oscale, act)

    def prepare(mf, groups=G, filters=w):
        opts = mf.ops.Conv2DOptions(mf.FusedActivation(act), mf.TensorViewPadding(0 if same else 1), (s, s), (dil, dil), groups)
        return mf.ops.prepare_conv_2d((H, W, C), filters, wzp.astype(dt), izp, oscale, ozp, opts, (c0, c1), (OH, OW))
    return prepare, x, want


@pytest.mark.parametrize("name,key,var", CASES, ids=[c[0] for c in CASES])
def test_a_grouped_convolution_is_the_contract(mf, name, key, var):
    prepare, x, want = build(name, key, **var)
    if not var:
        inside = float(np.mean((want > -128) & (want < 127)))
        assert 0.35 <= inside <= 0.65, inside       # (a property of the test's constants, from the reference alone)
    op, G = prepare(mf), SHAPES[key][7]
    if key in TWIN:
        assert op.kernel.endswith("[g%d]" % G) and "conv_grp" not in op.kernel, op.kernel
    else:
        assert op.kernel == "conv_grp_rt<g%d%s>" % (G, ",wzp" if var.get("wz") else ""), op.kernel
        assert key not in PLAN or PLAN[key](op.tile_plan()), op.tile_plan()
    got = op(x)
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    op.set_generic(True)
    assert op.kernel.startswith("conv2d_generic"), op.kernel
    gen = op(x)
    assert np.array_equal(gen, want), int((gen != want).sum())


def test_a_workgroup_walks_many_steps(mf):
    """More steps than the launch can have workgroups, so every workgroup stages over a tile it has read; a ragged last step."""
    import torch
    batch, unique = 70003, 61
    prepare, x, want = build("steps-g1", "g1", batch=unique)
    idx = torch.arange(batch) % unique
    op = prepare(mf)
    assert op.kernel.startswith("conv_grp_rt") and batch % op.tile_plan()["images"] != 0, (op.kernel, op.tile_plan())
    got = op(torch.as_tensor(x)[idx].cuda())
    bad = (got != torch.as_tensor(want)[idx].cuda()).flatten(1).any(1).nonzero().flatten()
    assert bad.numel() == 0, bad[:8].tolist()


def test_one_group_is_the_old_entry_point_and_bad_group_counts_are_refused(mf):
    """groups = 1 against mf_conv_2d_dilated_create: the same kernel and bytes.  G < 1, C % G != 0 and N % G != 0: MF_ERR_INVALID_ARG."""
    import ctypes as C
    from microflow_rs_amd import _lib, ops as o
    rng = np.random.default_rng(4)
    w = rng.integers(-127, 128, (16, 3, 3, 16)).astype(np.int8)
    z, c0, c1, h = np.zeros(1, np.int8), np.zeros(16, f32), np.full(16, 0.001, f32), C.c_void_p()
    new = o.prepare_conv_2d((9, 9, 16), w, z, 3, 0.1, -5, o.Conv2DOptions(groups=1), (c0, c1), (9, 9))
    _lib.check(_lib.lib().mf_conv_2d_dilated_create(0, 9, 9, 16, 16, 3, 3, o._ptr(w), o._ptr(z), 1, 3, 0.1, -5, 0, 0, 1, 1, 9, 9, o._ptr(c0), o._ptr(c1), 16, 1, 1, C.byref(h)))
    old = o.PreparedOp(h, (9, 9, 16), (9, 9, 16), np.int8)
    x = rng.integers(-128, 128, (2, 9, 9, 16)).astype(np.int8)
    assert old.kernel == new.kernel and "grp" not in new.kernel and np.array_equal(old(x), new(x)), (old.kernel, new.kernel)
    for cin, n, g in ((16, 16, 0), (16, 16, -2), (18, 16, 4), (16, 18, 4)):
        with pytest.raises(_lib.MicroflowError) as e:
            o.prepare_conv_2d((9, 9, cin), np.ones((n, 3, 3, 4), np.int8), z, 0, 0.1, 0, o.Conv2DOptions(groups=g), (np.zeros(n, f32), np.ones(n, f32)), (9, 9))
        assert e.value.status == _lib.MF_ERR_INVALID_ARG, e.value
