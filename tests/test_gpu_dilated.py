"""Conv2D and DepthwiseConv2D with dilation factors: conv_dil_rt (k_conv_dil.hip), dw_gemm_rt's dilated geometry and the two generic
kernels, each byte for byte against tests/dilated_ref.py through ops.prepare_conv_2d / prepare_depthwise_conv_2d.  Every case names
what it can break.  Constants as tests/test_gpu_tconv.py's: inputs over the whole byte range, weights in +-127, c1 near 190 / (74 73.3
sqrt(taps C)) with `taps` the taps inside the image averaged over the output pixels (KH KW where no window reaches the halo; a halo tap
adds exactly 0, so the accumulator's deviation follows the in-image taps): about half the outputs lie strictly inside the clamp
(asserted on the reference's result).  Seeds are fixed per case."""
import zlib

import numpy as np
import pytest

from tests import dilated_ref as D
from tests.test_gpu_tconv import mf  # noqa: F401  (the module-scoped fixture: the package on a machine with a GPU)

pytestmark = pytest.mark.gpu
f32 = np.float32


#              H   W   C    N   KH KW  s  dh dw same batch
CONV = {
    "c1":  (7,  7,  16,  16,  3, 3, 1, 2, 2, True, 2),    # both plane phases, halo on four sides
    "c2":  (6,  9,  4,   12,  3, 3, 1, 1, 3, False, 2),   # W no multiple of dw: planes of unequal length; AL = 4
    "c3":  (9,  5,  16,  8,   3, 3, 1, 3, 1, True, 2),    # row-only dilation: one plane, the LDS-DMA row copy; N < 16
    "c4":  (1,  20, 8,   24,  1, 3, 1, 1, 4, False, 2),   # the TCN shape, H = 1
    "c5":  (8,  8,  20,  10,  2, 2, 1, 2, 2, True, 2),    # even filter: padt = 1 with a bottom / right margin of 1; byte stores
    "c6":  (7,  8,  16,  16,  3, 3, 2, 2, 2, True, 2),    # stride and dilation together: windows start in either phase
    "c7":  (5,  5,  16,  16,  3, 3, 1, 3, 3, True, 2),    # Ke = 7 > H: windows with only the centre tap in bounds
    "c8":  (24, 24, 64,  16,  3, 3, 1, 3, 3, True, 3),    # 30 tile rows of 2128 B exceed the 48 KiB step: row bands, (KH - 1) dh halo rows between them
    "c9":  (4,  4,  128, 128, 3, 3, 1, 3, 3, True, 2),    # 144 KiB of weights: N slices
    "c11": (7,  7,  18,  16,  3, 3, 1, 2, 2, True, 2),    # C % 4 != 0 (and image rows that are no whole dwords): conv2d_generic, still exact
    # c1 - c6 have fewer than 3x the taps in their effective extent and run the stuffed filter on the undilated kernels; the same
    # properties on conv_dil_rt, at factors from 3x on:
    "p1":  (7,  7,  16,  16,  3, 3, 1, 3, 2, True, 5),    # both plane phases, halo on four sides; several images per step, a ragged last one
    "p2":  (6,  11, 4,   12,  3, 3, 1, 2, 3, False, 2),   # W no multiple of dw; AL = 4
    "p3":  (9,  5,  16,  8,   3, 3, 1, 4, 1, True, 2),    # row-only dilation: one plane, the LDS-DMA row copy
    "p5":  (8,  8,  20,  10,  2, 2, 1, 3, 3, True, 2),    # even filter, Ke = 4: padt = 1 with a bottom / right margin of 2; byte stores
    "p6":  (7,  8,  16,  16,  3, 3, 2, 3, 3, True, 2),    # stride and dilation together
}
DEPTHWISE = {  # (N = C)
    "d1":  (7,  7,  16,  16,  3, 3, 1, 2, 2, True, 2),    # C % 16 == 0 with zero filter zero points: dw_gemm_rt, not dw_mm_rt
    "d2":  (6,  10, 20,  20,  3, 3, 1, 1, 3, False, 2),   # AL = 4
    "d3":  (9,  9,  8,   8,   5, 5, 1, 2, 2, True, 2),    # Ke = H; two pixels per 16-row group
    "d4":  (7,  7,  6,   6,   3, 3, 1, 2, 2, True, 2),    # image rows that are no whole dwords: dwconv_generic
    "d5":  (7,  8,  6,   6,   3, 3, 1, 2, 2, True, 2),    # AL = 1
    "d6":  (24, 24, 64,  64,  3, 3, 1, 3, 3, True, 3),    # row bands
    "q1":  (7,  7,  16,  16,  3, 3, 1, 3, 3, True, 2),    # d1 on the dilated dw_gemm_rt (d1, d2, d4, d5 run the stuffed filter)
    "q5":  (7,  8,  6,   6,   3, 3, 1, 3, 3, True, 2),    # AL = 1 there
}
SHAPES = dict(CONV, **DEPTHWISE)
GENERIC = {"c11": "conv2d_generic", "d4": "dwconv_generic"}


def stuffed(key):   # fewer than 3x the taps in the effective extent: the undilated operator with the zero-stuffed filter
    KH, KW, _, dh, dw = SHAPES[key][4:9]
    return ((KH - 1) * dh + 1) * ((KW - 1) * dw + 1) < 3 * KH * KW and key not in GENERIC


def fast_name(key):
    dh, dw = SHAPES[key][7:9]
    return GENERIC.get(key) or ("conv_dil_rt<d%dx%d" % (dh, dw) if key in CONV else "dw_gemm_rt<%dx%d,d%dx%d" % (SHAPES[key][4:6] + (dh, dw)))


#          bands > 1, slices > 1, images per step > 1 -- asserted on the operator's plan, so that a planner change cannot empty the case
PLAN = {"c8": lambda p: p["planes"] == 3 and p["bands"] > 1 and p["rows"] >= p["band_rows"] + 6, "c9": lambda p: p["slices"] > 1,
        "p1": lambda p: p["planes"] == 2 and 1 < p["images"] and 5 % p["images"] != 0, "p3": lambda p: p["planes"] == 1, "d6": lambda p: p["bands"] > 1}


VARIATIONS = [("worst", dict(worst=True)), ("u8", dict(u8=True)), ("relu", dict(act=1)), ("relu6", dict(act=3)), ("nobias", dict(bias=False)), ("wzp", dict(wz=True))]
CASES = [(k, k, {}) for k in SHAPES] + [("%s-%s" % (k, n), k, v) for k in ("p1", "q1") for n, v in VARIATIONS] + [("c1-wzp", "c1", dict(wz=True)), ("d1-u8", "d1", dict(u8=True))]   # (the new kernels; one each through the stuffed filter)


def build(name, key, u8=False, act=0, bias=True, wz=False, worst=False, batch=None):
    """-> (prepare(mf) giving the operator, x, the contract's output)"""
    H, W, C, N, KH, KW, s, dh, dw, same, b0 = SHAPES[key]
    batch, depthwise = batch or b0, key in DEPTHWISE
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    dt, off = (np.uint8, 128) if u8 else (np.int8, 0)
    OH, OW = D.geometry(H, W, KH, KW, (s, s), (dh, dw), same)[:2]
    x = (rng.integers(-128, 128, (batch, H, W, C)) + off).astype(dt)
    w = (rng.integers(-127, 128, (KH, KW, N) if depthwise else (N, KH, KW, C)) + off).astype(dt)
    wzp = (np.where(rng.integers(0, 2, N) > 0, 1, -1) * rng.integers(1, 25, N) if wz else np.zeros(N, np.int64)) + off
    izp, ozp, oscale = int(rng.integers(-20, 21)) + off, int(rng.integers(-20, 21)) + off, f32(0.0235294122)
    c0 = rng.uniform(-30, 30, N).astype(f32) if bias else np.zeros(N, f32)
    taps = D.mean_taps(H, W, KH, KW, (s, s), (dh, dw), same)   # (KH KW where no window reaches the halo)
    c1 = (rng.uniform(0.8, 1.25, N) * 190.0 / (74.0 * 73.3 * np.sqrt(taps * (1 if depthwise else C)))).astype(f32)
    if worst:   # input all -128, weights all 127, unit constants: the accumulator bound, saturation
        x[:], w[:], izp, c0, c1 = -128, 127, 0, np.zeros(N, f32), np.ones(N, f32)
    want = D.conv(x, w, izp, wzp, (s, s), (dh, dw), same, c0, c1, ozp, oscale, act, depthwise)

    def prepare(mf):
        cls, prep = (mf.ops.DepthwiseConv2DOptions, mf.ops.prepare_depthwise_conv_2d) if depthwise else (mf.ops.Conv2DOptions, mf.ops.prepare_conv_2d)
        opts = cls(mf.FusedActivation(act), mf.TensorViewPadding(0 if same else 1), (s, s), (dh, dw))
        return prep((H, W, C), w, wzp.astype(dt), izp, oscale, ozp, opts, (c0, c1), (OH, OW))
    return prepare, x, want


@pytest.mark.parametrize("name,key,var", CASES, ids=[c[0] for c in CASES])
def test_a_dilated_convolution_is_the_contract(mf, name, key, var):
    prepare, x, want = build(name, key, **var)
    if not var.get("worst") and not var.get("act"):
        lo, hi = (0, 255) if want.dtype == np.uint8 else (-128, 127)
        inside = float(np.mean((want > lo) & (want < hi)))
        assert 0.35 <= inside <= 0.65, inside       # (a property of the test's constants, from the reference alone)
    op = prepare(mf)
    dh, dw = SHAPES[key][7:9]
    if stuffed(key):
        assert op.kernel.endswith("[d%dx%d]" % (dh, dw)) and "generic" not in op.kernel and "d%dx%d" % (dh, dw) not in op.kernel[:-6], op.kernel
    else:
        assert op.kernel.startswith(fast_name(key)) and op.kernel.endswith(",wzp>") == bool(var.get("wz") and key not in GENERIC), op.kernel
        assert key not in PLAN or PLAN[key](op.tile_plan()), op.tile_plan()
    got = op(x)
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    op.set_generic(True)
    assert op.kernel in ("conv2d_generic", "dwconv_generic"), op.kernel
    gen = op(x)
    assert np.array_equal(gen, want), int((gen != want).sum())


@pytest.mark.parametrize("key,batch,unique", [("p1", 70003, 61), ("c8", 803, 3), ("q1", 70003, 61)], ids=["conv-whole-images", "conv-bands", "depthwise"])
def test_a_workgroup_walks_many_steps(mf, key, batch, unique):
    """More steps than the launch can have workgroups (at most 2048), so every workgroup stages over a tile it has read: 4376 steps of
    16 whole images with a ragged last one, 1606 bands whose out-of-image halo rows are refilled.  `unique` images repeated."""
    import torch
    prepare, x, want = build("steps-" + key, key, batch=unique)
    idx = torch.arange(batch) % unique
    op = prepare(mf)
    assert op.kernel.startswith(fast_name(key)) and (key != "c8" or op.tile_plan()["bands"] > 1), op.kernel
    got = op(torch.as_tensor(x)[idx].cuda())
    bad = (got != torch.as_tensor(want)[idx].cuda()).flatten(1).any(1).nonzero().flatten()
    assert bad.numel() == 0, bad[:8].tolist()


def test_factors_along_one_tap_and_bad_arguments(mf):
    """A 1 x 1 filter at any factors routes as the undilated operator; factors <= 0 and a size the placement does not give are refused."""
    from microflow_rs_amd import _lib
    o = mf.ops
    w, z, c = np.ones((16, 1, 1, 16), np.int8), np.zeros(1, np.int8), (np.zeros(16, f32), np.ones(16, f32))
    names = [o.prepare_conv_2d((8, 8, 16), w, z, 0, 0.1, 0, o.Conv2DOptions(dilation=d), c, (8, 8)).kernel for d in ((1, 1), (3, 2))]
    assert names[0] == names[1] and not names[0].startswith("conv_dil"), names
    w3 = np.ones((16, 3, 3, 16), np.int8)
    for dil, out_hw in (((0, 1), (8, 8)), ((1, -2), (8, 8)), ((2, 2), (6, 6)), ((2, 2), (8, 7))):   # VALID at 2 x 2 gives 4 x 4
        with pytest.raises(_lib.MicroflowError) as e:
            o.prepare_conv_2d((8, 8, 16), w3, z, 0, 0.1, 0, o.Conv2DOptions(view_padding=mf.TensorViewPadding(1 if out_hw == (6, 6) else 0), dilation=dil), c, out_hw)
        assert e.value.status == _lib.MF_ERR_INVALID_ARG, e.value


def test_the_old_entry_points_are_the_new_ones_at_one(mf):
    """mf_conv_2d_create / mf_depthwise_conv_2d_create against the *_dilated_create calls at (1, 1): the same kernel and the same bytes"""
    import ctypes as C
    from microflow_rs_amd import _lib, ops as o
    rng = np.random.default_rng(4)
    for dw in (False, True):
        w = rng.integers(-127, 128, (3, 3, 16) if dw else (16, 3, 3, 16)).astype(np.int8)
        z, c0, c1, h = np.zeros(1, np.int8), np.zeros(16, f32), np.full(16, 0.001, f32), C.c_void_p()
        new = (o.prepare_depthwise_conv_2d if dw else o.prepare_conv_2d)((9, 9, 16), w, z, 3, 0.1, -5, (o.DepthwiseConv2DOptions if dw else o.Conv2DOptions)(), (c0, c1), (9, 9))
        fn = _lib.lib().mf_depthwise_conv_2d_create if dw else _lib.lib().mf_conv_2d_create
        geo = (9, 9, 16, 3, 3, 16) if dw else (9, 9, 16, 16, 3, 3)
        _lib.check(fn(0, *geo, o._ptr(w), o._ptr(z), 1, 3, 0.1, -5, 0, 0, 1, 1, 9, 9, o._ptr(c0), o._ptr(c1), 16, C.byref(h)))
        old = o.PreparedOp(h, (9, 9, 16), (9, 9, 16), np.int8)
        x = rng.integers(-128, 128, (2, 9, 9, 16)).astype(np.int8)
        assert old.kernel == new.kernel and np.array_equal(old(x), new(x)), (old.kernel, new.kernel)
