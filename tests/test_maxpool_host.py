"""MaxPool2D without a GPU: a LeNet written with max pools loads and reports the operator (kind 17, shapes, the average pool's
constants), the writer's default blobs are byte for byte what they were, geometries with an empty window are refused with the stated
codes, the numpy restatement the GPU tests compare against (tests/maxpool_ref.py) gives a hand-computed known answer, and the
listing of the two layer-wise kernels keeps the house rules."""
import ctypes as C
import hashlib
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests.conftest import ROOT
from tests import maxpool_ref as R

sys.path.insert(0, os.path.join(ROOT, "tools"))

CSRC = os.path.join(ROOT, "microflow_rs_amd", "csrc")
U8 = 3


def test_a_lenet_with_max_pools_loads_and_reports_the_operator():
    """the test that fails without the operator: `unsupported operator: 17`"""
    import microflow_rs_amd as mf
    import tflite_writer as tw
    from microflow_rs_amd import _lib
    for elem in (9, U8):
        shape, in_q, layers = tw.lenet_layers(np.random.default_rng(5), elem=elem, wzp_nonzero=elem == U8, pool="max")
        assert tw.build_model(shape, in_q, layers, elem) == tw.lenet(np.random.default_rng(5), elem=elem, wzp_nonzero=elem == U8, pool="max")
        m = mf.Model(tw.build_model(shape, in_q, layers, elem))
        assert m.num_ops == 9 and [o["kind"] for o in m.ops] == [3, 17, 3, 17, 22, 9, 9, 9, 25]
        assert _lib.MF_OP_MAX_POOL_2D == 17
        for i, (ins, outs) in ((1, ((1, 24, 24, 6), (1, 12, 12, 6))), (3, ((1, 8, 8, 16), (1, 4, 4, 16)))):
            d, L, prev = m.op(i), layers[i], layers[i - 1]
            assert d["name"] == "max_pool_2d" and d["in_shape"] == ins and d["out_shape"] == outs
            assert (d["KH"], d["KW"], d["sh"], d["sw"], d["pad"], d["act"]) == (2, 2, 2, 2, 1, 0)
            assert d["n_c0"] == 1 and d["n_c1"] == 1 and d["out_elems"] == int(np.prod(outs))
            c0, c1, _, _ = m.op_constants(i)
            # ... the average pool's: mf_preprocess_average_pool_2d's own results, and the restatement's
            a, b = C.c_float(), C.c_float()
            fn = _lib.lib().mf_preprocess_average_pool_2d_u8 if elem == U8 else _lib.lib().mf_preprocess_average_pool_2d
            _lib.check(fn(prev["out_q"][0], prev["out_q"][1], L["out_q"][0], L["out_q"][1], C.byref(a), C.byref(b)))
            assert (np.float32(a.value), np.float32(b.value)) == (c0[0], c1[0]) == R.pool_constants(*prev["out_q"], *L["out_q"])


# sha256 of the blobs the writer gave before it knew MaxPool2D (recorded from the parent commit)
PARENT_BLOBS = {
    "lenet": (49160, "c006dc6aa8780c5ecb912ae56815660e85f5d8cb0664d3086b05263a27913efa"),
    "lenet-u8-wzp": (49160, "7389de261572a8c6d8024acc1c9da7457c33b715469f17a12f6cd405eb059d92"),
    "cifar": (173464, "c39477b3b8d3f485619595f6ccfbc070a9ee44e3fb4bc8095796f60c33ac80c3"),
    "stage": (3792, "312b31df36b26a7f8f1430d665ee9de41d974a3e72669d3a0c17d77421ae465d"),
    "stage-u8-pool3x3": (10544, "59032297c48f4256ef3bcb137afc44bc86158594ca4ce0360cc91781414a48f0"),
}


def _default_blobs(tw, **kw):
    rng = np.random.default_rng
    return {
        "lenet": tw.lenet(rng(5), **kw),
        "lenet-u8-wzp": tw.lenet(rng(6), elem=tw.UINT8, wzp_nonzero=True, **kw),
        "cifar": tw.lenet(rng(9), shape=(32, 32, 3), convs=((32, 3), (64, 3)), fcs=(64, 10), **kw),
        "stage": tw.conv_pool(rng(7), (12, 12, 6), 16, 5, **({"pool_op": kw["pool"]} if kw else {})),
        "stage-u8-pool3x3": tw.conv_pool(rng(8), (48, 48, 8), 96, 3, padding="same", pool=(3, 3), pool_padding="same", pool_q=0.8, elem=tw.UINT8,
                                         wzp_nonzero=True, **({"pool_op": kw["pool"]} if kw else {})),
    }


def test_the_default_pool_gives_the_blobs_it_gave():
    import tflite_writer as tw
    for blobs in (_default_blobs(tw), _default_blobs(tw, pool="avg")):
        assert {k: (len(b), hashlib.sha256(b).hexdigest()) for k, b in blobs.items()} == PARENT_BLOBS
    # ... and a max pool differs from them in the operator code alone: the same length, two bytes per code (the deprecated and the new field)
    for k, b in _default_blobs(tw, pool="max").items():
        a = _default_blobs(tw)[k]
        diff = [i for i in range(len(a)) if a[i] != b[i]]
        assert len(a) == len(b) and len(diff) == 2 and {(a[i], b[i]) for i in diff} == {(1, 17)}, (k, diff)
    assert tw.conv_pool(np.random.default_rng(7), (12, 12, 6), 16, 5, pool="max") == _default_blobs(tw, pool="max")["stage"]


def _pool_model(tw, shape, filt, strides, padding, out_hw, elem=9, op="max_pool_2d"):
    q = (0.05, 228 if elem == U8 else 100)
    L = dict(op=op, filter=filt, padding=padding, strides=strides, act="none", out_shape=(1,) + tuple(out_hw) + (shape[2],), out_q=q)
    return tw.build_model((1,) + tuple(shape), q, [L], elem)


# (H, W), filter, strides, padding, the right output size, one with an empty last window
EMPTY = [((6, 6), (2, 2), (2, 2), "valid", (3, 3), (4, 3)),       # OH one too large under VALID: row 3 starts at input row 6
         ((6, 6), (2, 2), (2, 2), "valid", (3, 3), (3, 4)),
         ((7, 9), (3, 3), (2, 2), "same", (4, 5), (5, 5)),        # SAME: row 4 would start at 4 * 2 - 1 = 7
         ((7, 9), (3, 3), (2, 2), "same", (4, 5), (4, 6)),
         ((6, 7), (2, 3), (1, 2), "same", (6, 4), (7, 4))]


@pytest.mark.parametrize("case", range(len(EMPTY)))
def test_a_window_with_no_in_bounds_tap_is_refused(case):
    import microflow_rs_amd as mf
    import tflite_writer as tw
    from microflow_rs_amd import _lib
    (H, W), filt, strides, padding, good, bad = EMPTY[case]
    L = _lib.lib()
    for elem in (9, U8):
        assert mf.Model(_pool_model(tw, (H, W, 4), filt, strides, padding, good, elem)).op(0)["kind"] == 17
        with pytest.raises(mf.MicroflowError) as ei:
            mf.Model(_pool_model(tw, (H, W, 4), filt, strides, padding, bad, elem))
        assert ei.value.status == _lib.MF_ERR_INVALID_MODEL and "MaxPool2D" in str(ei.value)
        # the operator: a bad argument whether or not there is a device to create it on
        h = C.c_void_p()
        fn = L.mf_max_pool_2d_create_u8 if elem == U8 else L.mf_max_pool_2d_create
        st = fn(0, H, W, 4, filt[0], filt[1], 0.05, 100, 0, 0 if padding == "same" else 1, strides[0], strides[1], bad[0], bad[1], 1.0, 0.0, C.byref(h))
        assert st == _lib.MF_ERR_INVALID_ARG and not h.value and b"no in-bounds tap" in L.mf_last_error()
        st = fn(0, H, W, 4, filt[0], filt[1], 0.05, 100, 0, 0 if padding == "same" else 1, strides[0], strides[1], good[0], good[1], 1.0, 0.0, C.byref(h))
        if L.mf_device_count() > 0:
            assert st == _lib.MF_OK and h.value
            L.mf_op_destroy(h)
        else:
            assert st == _lib.MF_ERR_NO_DEVICE
    # the average pool of the same geometry is what it was: the reference's view fills such a window, the parser lets it through
    assert mf.Model(_pool_model(tw, (H, W, 4), filt, strides, padding, bad, 9, op="average_pool_2d")).op(0)["kind"] == 1


# ---- the restatement against a known answer worked out by hand ------------------------------------------------------------
KAT_X = np.array([[[1, -1], [-3, -5], [50, 30], [60, 30]],
                  [[7, -7], [2, -1], [61, 30], [-9, 30]],
                  [[-100, -1], [-90, -2], [83, 20], [84, 25]],
                  [[-95, -3], [-128, -4], [90, 33], [12, 5]]], np.int8)[None]          # [1][4][4][2]


def test_the_restatement_gives_the_hand_computed_answer():
    # 2x2 stride 2 VALID, (0.5, 10) -> (0.25, -20): c0 = 2, c1 = -20 - (0.5 * 10) / 0.25 = -40.  Window maxima: channel 0
    # [7 61; -90 90], channel 1 [-1 30; -1 33]; y = 2 m - 40 = [-26 82; -220 140] and [-42 20; -42 26]; -220 and 140 saturate
    c0, c1 = R.pool_constants(0.5, 10, 0.25, -20)
    assert (c0, c1) == (np.float32(2.0), np.float32(-40.0))
    want = {"none": [[[-26, -42], [82, 20]], [[-128, -42], [127, 26]]],
            "relu": [[[-20, -20], [82, 20]], [[-20, -20], [127, 26]]],                  # max(y, -20)
            "relu6": [[[-20, -20], [4, 4]], [[-20, -20], [4, 4]]]}                      # quantize(6.0) = roundf(6 / 0.25 - 20) = 4
    for act, w in want.items():
        got = R.max_pool_2d(KAT_X, (2, 2), (2, 2), "valid", (2, 2), c0, c1, act, 0.25, -20)
        assert got.dtype == np.int8 and np.array_equal(got[0], np.array(w, np.int8)), (act, got[0].tolist())
    # 3x3 stride 2 SAME (shift 1: the rows and columns -1 and 4 are outside), (0.5, 10) -> (1.0, 3): c0 = 0.5, c1 = 3 - 5 = -2.
    # Maxima over the in-bounds taps: channel 0 [7 61; 7 90] -> 1.5, 28.5, 1.5, 43 -> 2, 29, 2, 43 (ties away from zero);
    # channel 1 [-1 30; -1 33] -> -2.5, 13, -2.5, 14.5 -> -3, 13, -3, 15.  A zero-filled halo would turn both -1 into 0 (-> -2)
    c0, c1 = R.pool_constants(0.5, 10, 1.0, 3)
    assert (c0, c1) == (np.float32(0.5), np.float32(-2.0))
    got = R.max_pool_2d(KAT_X, (3, 3), (2, 2), "same", (2, 2), c0, c1, "none", 1.0, 3)
    assert np.array_equal(got[0], np.array([[[2, -3], [29, 13]], [[2, -3], [43, 15]]], np.int8)), got[0].tolist()
    # u8: the same values + 128 with zero points + 128: c1 = 131 - 69 = 62, y = 0.5 (m + 128) + 62 = the i8 y + 128, so the negative
    # ties now round upwards: 129.5, 156.5, 129.5, 171 -> 130, 157, 130, 171 and 125.5, 141, 125.5, 142.5 -> 126, 141, 126, 143
    c0u, c1u = R.pool_constants(0.5, 138, 1.0, 131)
    assert (c0u, c1u) == (np.float32(0.5), np.float32(62.0))
    gotu = R.max_pool_2d((KAT_X.astype(np.int16) + 128).astype(np.uint8), (3, 3), (2, 2), "same", (2, 2), c0u, c1u, "none", 1.0, 131)
    assert gotu.dtype == np.uint8 and np.array_equal(gotu[0], np.array([[[130, 126], [157, 141]], [[130, 126], [171, 143]]], np.uint8)), gotu[0].tolist()
    with pytest.raises(ValueError):
        R.max_pool_2d(KAT_X, (2, 2), (2, 2), "valid", (3, 2), c0, c1, "none", 1.0, 3)


def test_roundf_and_saturation_of_the_restatement():
    y = np.array([0.5, -0.5, 1.5, -1.5, 2.5, 0.49999997, -0.49999997, 126.5, -128.5, 300.0, -300.0, np.nan], np.float32)
    assert R.roundf(y)[:11].tolist() == [1, -1, 2, -2, 3, 0, -0.0, 127, -129, 300, -300]
    assert R.saturate(R.roundf(y), np.int8).tolist() == [1, -1, 2, -2, 3, 0, 0, 127, -128, 127, -128, 0]
    assert R.saturate(R.roundf(y), np.uint8).tolist() == [1, 0, 2, 0, 3, 0, 0, 127, 0, 255, 0, 0]


@pytest.mark.parametrize("dt", [np.int8, np.uint8])
def test_equal_quantisation_is_the_plain_window_max_for_every_byte(dt):
    """what converters emit: the pool's output has its input's scale and zero point, and the f32 step returns the byte it was given"""
    lo = 0 if dt == np.uint8 else -128
    vals = np.arange(lo, lo + 256)
    rng = np.random.default_rng(3)
    # 256 images, 4x4x3, 2x2 stride 2: image v holds values <= v, and v itself in every window
    x = np.minimum(rng.integers(lo, lo + 256, (256, 4, 4, 3)), vals[:, None, None, None])
    x[:, ::2, 1::2, :] = vals[:, None, None, None]
    x = x.astype(dt)
    for scale in (0.05, 0.0235294122, 0.37, 1.0 / 3.0):
        for zp in (lo, lo + 100, lo + 128, lo + 255):
            c0, c1 = R.pool_constants(scale, zp, scale, zp)
            got = R.max_pool_2d(x, (2, 2), (2, 2), "valid", (2, 2), c0, c1, "none", scale, zp)
            assert np.array_equal(got, np.broadcast_to(vals[:, None, None, None], got.shape).astype(dt)), (scale, zp)


# ---- the listing of the two layer-wise kernels --------------------------------------------------------------------------------
def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return hipcc


@pytest.fixture(scope="module")
def listing():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k_generic.s")
        subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mllvm",
                               "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "k_generic.hip")],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read().split("\n")


def test_the_kernels_listing(listing):
    spec = importlib.util.spec_from_file_location("asm_barrier_waits", os.path.join(ROOT, "scripts", "asm_barrier_waits.py"))
    abw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(abw)
    bodies = {n.replace("mf::k::", ""): b for n, b in abw.kernels(listing) if "maxpool" in n}
    assert sorted(bodies) == ["maxpool_c4", "maxpool_generic"], sorted(bodies)
    ins = lambda name: [l.split()[0] for l in bodies[name] if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    c4 = ins("maxpool_c4")
    # a tap of maxpool_c4 is one dword load, one shift and two packed 16-bit maxima; no f32 fma anywhere in either kernel (the
    # contract's c0 * x + c1 is two roundings)
    assert "v_pk_max_i16" in c4 and "global_load_dword" in c4 and "global_store_dword" in c4, sorted(set(c4))
    # (the only fused multiply-adds are the 2^32 steps of the 64-bit index divisions)
    fused = [l.strip() for n in bodies for l in bodies[n] if l.strip().startswith(("v_fma_f32", "v_fmac_f32", "v_mad_f32", "v_pk_fma_f32"))]
    assert all("0x4f800000" in l or "0xcf800000" in l for l in fused), fused
    assert any(i.startswith(("v_pk_mul_f32", "v_mul_f32")) for i in c4) and any(i.startswith(("v_pk_add_f32", "v_add_f32")) for i in c4)
    assert "global_load_sbyte" in ins("maxpool_generic") or "global_load_ubyte" in ins("maxpool_generic")
    text = "\n".join(listing)
    meta = text[text.index("amdhsa.kernels:"):]
    meta = meta[:meta.index("\namdhsa.target:")]
    seen = 0
    for e in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s*(\S+)", e).group(1)
        if "maxpool" not in name:
            continue
        seen += 1
        assert re.search(r"\.private_segment_fixed_size:\s*0\b", e), name
        assert re.search(r"\.vgpr_spill_count:\s*0\b", e) and re.search(r"\.sgpr_spill_count:\s*0\b", e), name
    assert seen == 2


# ---- conv_maxpool_rt (k_conv_maxpool.hip) and what it must leave alone ---------------------------------------------------------------
INSTANCES = 36                         # AL {16, 4, 1} x filter zero points {no, yes} x modes {0, 1, 2} x {i8, u8}, as conv_pool_rt


def _listing_of(src):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, src + ".s")
        subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mllvm",
                               "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, src)],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read().split("\n")


def _abw():
    spec = importlib.util.spec_from_file_location("asm_barrier_waits", os.path.join(ROOT, "scripts", "asm_barrier_waits.py"))
    abw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(abw)
    return abw


def _instances(kernel):
    return {"%s<%d, %s, %d, %du>" % (kernel, al, wz, mg, xr) for al in (16, 4, 1) for wz in ("false", "true") for mg in (0, 1, 2) for xr in (0, 0x80808080)}


def test_k_conv_pool_keeps_exactly_its_36_kernels():
    kernels = list(_abw().kernels(_listing_of("k_conv_pool.hip")))
    assert len(kernels) == INSTANCES and {n for n, _ in kernels} == _instances("conv_pool_rt"), sorted(n for n, _ in kernels)


def test_k_conv_maxpool_listing():
    """every instance exists under the kernel's name; four barriers each (weights staged | top of step | tile staged | Y complete), none
    reached with LDS operations pending; the matrix instruction, the LDS-DMA and the packed max are there; no scratch, no spills,
    registers inside the launch bounds (256 threads, two workgroups per CU)"""
    abw = _abw()
    listing = _listing_of("k_conv_maxpool.hip")
    kernels = list(abw.kernels(listing))
    assert len(kernels) == INSTANCES and {n for n, _ in kernels} == _instances("conv_maxpool_rt"), sorted(n for n, _ in kernels)
    for name, body in kernels:
        assert sum(1 for l in body if l.strip().startswith("s_barrier")) == 4, name
        assert not abw.scan(body), (name, abw.scan(body))
        ins = [l.split()[0] for l in body if l.startswith("\t") and not l.strip().startswith((".", ";"))]
        assert ins.count("v_pk_max_i16") == 2 and not any(i.startswith("v_dot4") for i in ins), name     # phase B takes maxima, sums nothing
        assert not any(i.startswith(("v_fma_f32", "v_fmac_f32", "v_mad_f32", "v_pk_fma_f32")) for i in ins), name
    text = "\n".join(listing)
    assert "v_mfma_i32_16x16x64_i8" in text and "global_load_lds_dwordx4" in text
    meta = text[text.index("amdhsa.kernels:"):]
    meta = meta[:meta.index("\namdhsa.target:")]
    seen = 0
    for e in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s*(\S+)", e).group(1)
        seen += 1
        vgpr = int(re.search(r"\.vgpr_count:\s*(\d+)", e).group(1))
        agpr = re.search(r"\.agpr_count:\s*(\d+)", e)
        assert 0 < vgpr and vgpr + (int(agpr.group(1)) if agpr else 0) <= 128, name
        assert re.search(r"\.private_segment_fixed_size:\s*0\b", e), name
        assert re.search(r"\.vgpr_spill_count:\s*0\b", e), name
    assert seen == INSTANCES
