"""RESIZE_NEAREST_NEIGHBOR and resize + Conv2D in one launch: upconv_rt (k_upconv.hip) and upconv_generic byte for byte against
tests/dilated_ref.conv on tests/resize_ref.resize's image, through ops.prepare_conv_2d(upsample=...); resize_nn_c4 / resize_nn_generic
against np.repeat; the UpSampling2D models against the composed operators.  Every case names what it can break.  Constants as
tests/test_gpu_grouped.py's, c1 from the taps of the UPSAMPLED geometry (half the outputs inside the clamp); seeds per case."""
import os
import sys
import zlib

import numpy as np
import pytest

from tests import dilated_ref as D
from tests import resize_ref as R
from tests.conftest import ROOT
from tests.test_gpu_tconv import mf  # noqa: F401  (the module-scoped fixture: the package on a machine with a GPU)

sys.path.insert(0, os.path.join(ROOT, "tools"))
import tflite_writer as tw  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32

#            H   W   C    N    KH KW sy sx same  batch      (of the SOURCE)
SHAPES = {
    "u1":  (4,  4,  16,  16,  3, 3, 2, 2, True,  5),   # b128 operand, halo on four sides, ragged last step
    "u2":  (3,  5,  32,  16,  3, 3, 2, 2, True,  2),   # two 16-byte chunks per tap, odd sizes
    "u3":  (5,  4,  8,   24,  3, 3, 2, 2, False, 2),   # dword gather, N % 16 != 0, no halo
    "u4":  (3,  3,  16,  16,  3, 3, 3, 3, True,  2),   # three y phases, d of -1, 0, +1
    "u5":  (4,  6,  16,  32,  5, 5, 2, 2, True,  2),   # pad 2: two halo rows map to one source row
    "u6":  (4,  4,  4,   8,   3, 3, 2, 2, True,  2),   # C = 4: K padded from 12 to 16 per row
    "u7":  (6,  3,  16,  16,  3, 3, 2, 1, True,  2),   # y only, a 3-pixel row: chunks span rows
    "u8":  (3,  6,  16,  16,  1, 1, 2, 2, True,  2),   # 1x1: the tables are all phase-free
    "u9":  (16, 16, 32,  32,  3, 3, 2, 2, True,  3),   # a 32 x 32 output, 18 source rows per image (the planner keeps whole images here)
    "u10": (2,  2,  256, 256, 3, 3, 2, 2, True,  2),   # N slices
    "u11": (3,  3,  16,  16,  2, 2, 4, 4, False, 2),   # even filter, factor 4
    "u12": (5,  5,  12,  10,  3, 3, 1, 2, True,  2),   # x only, N % 4 != 0 byte stores
    "u13": (31, 32, 32,  16,  3, 3, 2, 2, True,  2),   # row bands: starts on multiples of sy, zero-point rows above and below, a ragged last band
}
PLAN = {"u13": lambda p: p["bands"] > 1 and p["band_rows"] % 2 == 0 and 62 % p["band_rows"] != 0, "u10": lambda p: p["slices"] > 1, "u1": lambda p: 1 < p["images"] and 5 % p["images"] != 0}
VARIATIONS = [("worst", dict(worst=True)), ("u8", dict(u8=True)), ("relu6", dict(act=3)), ("nobias", dict(bias=False))]
CASES = [(k, k, {}) for k in SHAPES] + [("%s-%s" % (k, n), k, v) for k in ("u1", "u3", "u4") for n, v in VARIATIONS] + [("u1-wzp", "u1", dict(wz=True))]


def build(name, key, u8=False, act=0, bias=True, wz=False, worst=False, batch=None):
    """-> (prepare(mf) giving the operator, x, the contract's output)"""
    H, W, C, N, KH, KW, sy, sx, same, b0 = SHAPES[key]
    batch = batch or b0
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    dt, off = (np.uint8, 128) if u8 else (np.int8, 0)
    OH, OW = D.geometry(H * sy, W * sx, KH, KW, (1, 1), (1, 1), same)[:2]
    x = (rng.integers(-128, 128, (batch, H, W, C)) + off).astype(dt)
    w = (rng.integers(-127, 128, (N, KH, KW, C)) + off).astype(dt)
    wzp = (np.where(rng.integers(0, 2, N) > 0, 1, -1) * rng.integers(1, 25, N) if wz else np.zeros(N, np.int64)) + off
    izp, ozp, oscale = int(rng.integers(-20, 21)) + off, int(rng.integers(-20, 21)) + off, f32(0.0235294122)
    c0 = rng.uniform(-30, 30, N).astype(f32) if bias else np.zeros(N, f32)
    taps = D.mean_taps(H * sy, W * sx, KH, KW, (1, 1), (1, 1), same)
    c1 = (rng.uniform(0.8, 1.25, N) * 190.0 / (74.0 * 73.3 * np.sqrt(taps * C))).astype(f32)
    if worst:   # input all -128, weights all 127, unit constants: the accumulator bound, saturation
        x[:], w[:], izp, c0, c1 = -128, 127, 0, np.zeros(N, f32), np.ones(N, f32)
    want = D.conv(R.resize(x, sy, sx), w, izp, wzp, (1, 1), (1, 1), same, c0, c1, ozp, oscale, act)

    def prepare(mf):
        opts = mf.ops.Conv2DOptions(mf.FusedActivation(act), mf.TensorViewPadding(0 if same else 1), (1, 1), upsample=(sy, sx))
        return mf.ops.prepare_conv_2d((H, W, C), w, wzp.astype(dt), izp, oscale, ozp, opts, (c0, c1), (OH, OW))
    return prepare, x, want


@pytest.mark.parametrize("name,key,var", CASES, ids=[c[0] for c in CASES])
def test_an_upsampled_convolution_is_the_contract(mf, name, key, var):
    prepare, x, want = build(name, key, **var)
    if not var:
        inside = float(np.mean((want > -128) & (want < 127)))
        assert 0.35 <= inside <= 0.65, inside       # (a property of the test's constants, from the reference alone)
    op, (sy, sx) = prepare(mf), SHAPES[key][6:8]
    assert op.kernel == ("upconv_generic" if var.get("wz") else "upconv_rt<%dx%d>" % (sy, sx)), op.kernel
    assert var or key not in PLAN or PLAN[key](op.tile_plan()), op.tile_plan()
    got = op(x)
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    op.set_generic(True)
    assert op.kernel == "upconv_generic", op.kernel
    gen = op(x)
    assert np.array_equal(gen, want), int((gen != want).sum())


def test_a_workgroup_walks_many_steps(mf):
    """More steps than the launch can have workgroups, so every workgroup stages over a tile it has read; a ragged last step."""
    import torch
    batch, unique = 70003, 61
    prepare, x, want = build("steps-u1", "u1", batch=unique)
    idx = torch.arange(batch) % unique
    op = prepare(mf)
    assert op.kernel.startswith("upconv_rt") and batch % op.tile_plan()["images"] != 0, (op.kernel, op.tile_plan())
    got = op(torch.as_tensor(x)[idx].cuda())
    bad = (got != torch.as_tensor(want)[idx].cuda()).flatten(1).any(1).nonzero().flatten()
    assert bad.numel() == 0, bad[:8].tolist()


def test_factors_of_one_are_the_old_entry_point_and_bad_sizes_are_refused(mf):
    """mf_conv_2d_upsampled_create at (1, 1) against mf_conv_2d_create's route: the same kernel and bytes.  An output size that is not the
    resized image's, and a factor below 1: MF_ERR_INVALID_ARG.  (Creating an operator needs a device, so the check is here and not
    in tests/test_resize_host.py.)"""
    import ctypes as C
    from microflow_rs_amd import _lib, ops as o
    rng = np.random.default_rng(4)
    w = rng.integers(-127, 128, (16, 3, 3, 16)).astype(np.int8)
    z, c0, c1, h = np.zeros(1, np.int8), np.zeros(16, f32), np.full(16, 0.001, f32), C.c_void_p()
    old = o.prepare_conv_2d((8, 8, 16), w, z, 3, 0.1, -5, o.Conv2DOptions(), (c0, c1), (8, 8))
    _lib.check(_lib.lib().mf_conv_2d_upsampled_create(0, 8, 8, 16, 16, 3, 3, o._ptr(w), o._ptr(z), 1, 3, 0.1, -5, 0, 0, 1, 1, 8, 8, o._ptr(c0), o._ptr(c1), 16, 1, 1, C.byref(h)))
    new = o.PreparedOp(h, (8, 8, 16), (8, 8, 16), np.int8)
    x = rng.integers(-128, 128, (2, 8, 8, 16)).astype(np.int8)
    assert old.kernel == new.kernel and "upconv" not in new.kernel and np.array_equal(old(x), new(x)), (old.kernel, new.kernel)
    for up, out in (((2, 2), (4, 4)), ((2, 2), (8, 9)), ((0, 2), (8, 8))):
        with pytest.raises(_lib.MicroflowError) as e:
            o.prepare_conv_2d((4, 4, 16), w, z, 3, 0.1, -5, o.Conv2DOptions(upsample=up), (c0, c1), out)
        assert e.value.status == _lib.MF_ERR_INVALID_ARG, e.value


@pytest.mark.parametrize("shape,factors", [((3, 5, 16), (2, 2)), ((4, 3, 8), (3, 1)), ((2, 7, 5), (2, 3))], ids=["v16", "dwords", "bytes"])
def test_resize_nearest_copies_the_right_bytes_and_nothing_else(mf, shape, factors):
    """resize_nn_c4 on 16-byte and dword pixels, resize_nn_generic where C % 4 != 0 and when forced; guard bytes around the output stay"""
    import torch
    from microflow_rs_amd import _lib
    x = np.random.default_rng(sum(shape)).integers(-128, 128, (3,) + shape).astype(np.int8)
    want = R.resize(x, *factors)
    op = mf.ops.prepare_resize_nearest(shape, factors)
    assert op.kernel == {16: "resize_nn_c4<v16>", 8: "resize_nn_c4", 5: "resize_nn_generic"}[shape[2]], op.kernel
    assert np.array_equal(op(x), want)
    assert np.array_equal(mf.ops.resize_nearest(mf.Tensor4D(x.view(np.uint8), [0.5], [7]), factors).buffer, want.view(np.uint8))
    buf, xt = torch.full((want.size + 512,), 77, dtype=torch.int8, device="cuda"), torch.as_tensor(x).cuda()
    for generic in (False, True):
        op.set_generic(generic)
        assert not generic or op.kernel == "resize_nn_generic"
        _lib.check(_lib.lib().mf_op_run(op._h, xt.data_ptr(), 3, buf.data_ptr() + 256, torch.cuda.current_stream().cuda_stream))
        got = buf.cpu().numpy()
        assert np.array_equal(got[256:-256], want.reshape(-1)) and (got[:256] == 77).all() and (got[-256:] == 77).all()
        buf[256:-256] = 77


@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
@pytest.mark.parametrize("name,kw", [("upsample_autoencoder", {}), ("upsample_autoencoder", dict(factor=4)), ("unet1", {})], ids=["autoencoder", "autoencoder-x4", "unet1"])
def test_the_upsampling_models_run_as_the_composed_operators(mf, name, kw, u8):
    """run_quantized and predict against the composed operators, fused and unfused.  Rule (0r) forms the resize + Conv2D group where it
    measured faster than the convolution alone: factors of 4, or a convolution whose own kernel is conv_gemm_rt; the
    factor-2 stages of these models run convolutions of other kernels and keep their two launches."""
    from oracle import oracle as O
    elem, dt = (tw.UINT8, np.uint8) if u8 else (tw.INT8, np.int8)
    in_q, layers = getattr(tw, name + "_layers")(np.random.default_rng(26), (16, 16, 4), (8, 16), elem=elem, **kw)
    m = mf.model(tw.build_model((1, 16, 16, 4), in_q, layers, elem))
    xq = (np.random.default_rng(5).integers(-128, 128, (5, 16, 16, 4)) + (128 if u8 else 0)).astype(dt)
    want = R.compose(tw, O, (1, 16, 16, 4), in_q, layers, elem, xq)
    got = m.run_quantized(xq).reshape(5, -1)
    assert np.array_equal(got, want), int((got != want).sum())
    xf = ((xq.astype(f32) - f32(in_q[1])) * f32(in_q[0])).astype(f32)   # (exactly representable: predict quantises it back to xq)
    yf = (want.astype(f32) - f32(m.output_zero_point)) * f32(m.output_scale)
    assert np.array_equal(m.predict(xf).reshape(5, -1), yf)
    first = [i for i in range(m.num_ops) if m.op(i)["name"].startswith("resize")]
    fused = [m.op(i)["kernel"] for i in first]
    m.set_fusion(False)
    alone = [(m.op(i)["kernel"], m.op(i + 1)["kernel"]) for i in first]
    assert all(r == ("resize_nn_c4<v16>" if m.op(i)["in_shape"][3] % 16 == 0 else "resize_nn_c4") for i, (r, _) in zip(first, alone)), alone
    f = kw.get("factor", 2)
    assert fused == ["resize+upconv_rt<%dx%d>" % (f, f) if f == 4 or c.startswith("conv_gemm_rt") else r for r, c in alone], (fused, alone)
    assert np.array_equal(m.run_quantized(xq).reshape(5, -1), want)
