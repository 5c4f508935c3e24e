"""k_pair_wz.hip without a GPU: the generated code keeps the house rules (every kernel a pair_wz_rt instance, no barrier reached
with LDS operations pending, M0 written only inside the LDS-DMA helper's asm, the int8 matrix instruction and the LDS-DMA present, no
scratch in any instance), the two ones images (tests/cpp/pair_wz_ones_dump.cpp, built with the host sanitizers) are what the
kernel's sums need, and the two-term formula the kernel computes -- acc = dot(v', w) - wzp * sum(v') + Kc over a tile whose halo
holds the input zero point -- is the reference's arithmetic (a numpy restatement against the CPU oracle; it does not load the
library)."""
import importlib.util
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "microflow_rs_amd", "csrc")
INSTANCES = 32                         # (one k step: modes 1, 2; two and four k steps: modes 0, 1, 2) x {resident, reloaded} x {i8, u8}
f32 = np.float32


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return hipcc


@pytest.fixture(scope="module")
def listing():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k_pair_wz.s")
        # (microflow_rs_amd/build.py's code-generation flags)
        subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mllvm",
                               "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "k_pair_wz.hip")],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read().split("\n")


@pytest.fixture(scope="module")
def abw():
    spec = importlib.util.spec_from_file_location("asm_barrier_waits", os.path.join(ROOT, "scripts", "asm_barrier_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the listing ----------------------------------------------------------------------------------------------------------
def test_design_states_the_instance_count():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.15"):]
    assert re.search(r"\b%d instances\b" % INSTANCES, sec[:sec.index("\n## ") if "\n## " in sec else len(sec)])


def test_pair_wz_barriers_wait_for_lds(listing, abw):
    kernels = list(abw.kernels(listing))
    assert len(kernels) == INSTANCES, [n for n, _ in kernels]
    for name, body in kernels:
        assert name.startswith("pair_wz_rt<"), name
        assert sum(1 for l in body if l.strip().startswith("s_barrier")) >= 3, name    # after the halo fill | top of step | depthwise -> pointwise
        assert not abw.scan(body), (name, abw.scan(body))


def test_pair_wz_m0_only_inside_asm(listing):
    in_asm, seen = False, 0
    for n, l in enumerate(listing):
        s = l.strip()
        if s.startswith(";;#ASMSTART"):
            in_asm = True
        elif s.startswith(";;#ASMEND"):
            in_asm = False
        elif l.startswith("\t") and re.search(r"\bm0\b", s.split(";")[0]):
            assert in_asm, (n, s)
            seen += 1
    assert seen >= INSTANCES, seen


def test_pair_wz_runs_on_the_matrix_pipe_with_lds_dma_and_no_scratch(listing):
    text = "\n".join(listing)
    assert "v_mfma_i32_16x16x64_i8" in text
    assert "global_load_lds_dwordx4" in text
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == INSTANCES and set(sizes) == {"0"}, sizes


def test_pair_wz_registers_leave_room_for_one_workgroup_per_cu(listing):
    """eight waves per workgroup = two per SIMD: at most 256 registers each (DESIGN 4.15 states the counts)"""
    counts = [int(v) for v in re.findall(r"\.vgpr_count:\s*(\d+)", "\n".join(listing))]
    assert len(counts) == INSTANCES and max(counts) <= 256, counts


# ---- the ones images --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def images(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("pair_wz") / "pair_wz_ones_dump")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(CSRC, "wimage.cpp"),
                           os.path.join(ROOT, "tests", "cpp", "pair_wz_ones_dump.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    by = {}
    for l in out.stdout.splitlines():
        name, shape, hx = l.split()
        by[(name, int(shape))] = np.frombuffer(bytes.fromhex(hx), np.int8)
    return by


def test_depthwise_ones_image_is_the_tap_image_of_an_all_ones_filter(images):
    img = images[("dw_ones", 16)]
    assert np.array_equal(img, images[("dw_mm_of_ones", 16)])
    img = img.reshape(3, 64, 16)                          # [filter row][lane][k byte]
    want = np.zeros((64, 16), np.int8)
    for lane in range(64):
        if lane >> 4 < 3:                                 # lane group = tap column; group 3 is padding: zeros
            want[lane, lane & 15] = 1                     # row r = channel r meets byte r of the tap's pixel
    for ty in range(3):
        assert np.array_equal(img[ty], want), ty          # (three equal rows: the kernel keeps one)


@pytest.mark.parametrize("C", [16, 48, 80, 128, 192, 256])
def test_pointwise_ones_tile_ends_at_the_channel_count(images, C):
    KS = (C + 63) // 64
    img = images[("pw_ones", C)]
    assert img.size == KS * 1024
    img = img.reshape(KS, 4, 16, 16)                      # [k step][lane group][row][byte]: k = 64 ks + 16 g + i
    k = np.transpose(img, (2, 0, 1, 3)).reshape(16, KS * 64)  # [row][k]
    for r in range(16):
        assert (k[r, :C] == 1).all() and (k[r, C:] == 0).all(), r     # exactly C ones per row, none in the padded k positions


# ---- the formula --------------------------------------------------------------------------------------------------------------
def _roundf(x):                                           # half away from zero (tests/test_u8.py)
    x = np.asarray(x, f32)
    return np.where(np.abs(x) < 8388608.0, np.trunc(x + np.copysign(f32(0.49999997), x)), x).astype(f32)


def _epilogue(acc, c0, c1, oscale, ozp, act, dt):
    lo, hi = (0, 255) if dt == np.uint8 else (-128, 127)
    a = (f32(ozp) + np.asarray(c0, f32)).astype(f32)
    b = (np.asarray(c1, f32) * acc.astype(f32)).astype(f32)
    y = np.clip(np.trunc(_roundf((a + b).astype(f32))), lo, hi).astype(np.int64)
    if act in (1, 3):
        y = np.maximum(y, ozp)
    if act == 3:
        six = int(np.clip(np.trunc(_roundf(f32(f32(6.0) / f32(oscale)) + f32(ozp))), lo, hi))
        y = np.minimum(y, six)
    return y.astype(dt)


def _two_term_pair(x, wd, zd, izp, cd, wp, zp_, izp2, cp, S, dt):
    """the kernel's arithmetic in the i8 domain it works in (u8: every byte and zero point minus 128): a halo'd tile filled with the
    input zero point, acc = dot(v', w) - wzp sum(v') + Kc with Kc = -izp sum(w) + T izp wzp, the reference's epilogue"""
    sh = 128 if dt == np.uint8 else 0
    H, W, C = x.shape
    OH, OW = -(-H // S), -(-W // S)
    v = x.astype(np.int64) - sh
    w = wd.astype(np.int64) - sh                          # [3][3][C]
    z = zd.astype(np.int64) - sh
    iz = izp - sh
    # SAME in the reference: (K - 1) / 2 = one pixel before, at either stride -- the halo pixel the kernel's tile has on every side
    tile = np.full((H + 2, W + 2, C), iz, np.int64)
    tile[1:H + 1, 1:W + 1] = v
    Kc = -iz * w.sum(axis=(0, 1)) + 9 * iz * z
    mid = np.zeros((OH, OW, C), np.int64)
    for oy in range(OH):
        for ox in range(OW):
            y0, x0 = oy * S, ox * S                       # (tile coordinates: input pixel -1 is tile pixel 0)
            win = tile[y0:y0 + 3, x0:x0 + 3]
            mid[oy, ox] = (win * w).sum(axis=(0, 1)) - z * win.sum(axis=(0, 1)) + Kc
    oscale, ozp, act, c0, c1 = cd
    m = _epilogue(mid, c0, c1, oscale, ozp, act, dt)
    u = m.astype(np.int64) - sh                           # MID, [OH][OW][C]
    wq = wp.astype(np.int64) - sh                         # [N][C]
    zq = zp_.astype(np.int64) - sh
    iz2 = izp2 - sh
    Kc2 = -iz2 * wq.sum(axis=1) + C * iz2 * zq
    acc = u @ wq.T - zq[None, None, :] * u.sum(axis=2, keepdims=True) + Kc2
    oscale, ozp, act, c0, c1 = cp
    return m, _epilogue(acc, c0, c1, oscale, ozp, act, dt)


@pytest.mark.parametrize("dt", [np.int8, np.uint8], ids=["i8", "u8"])
@pytest.mark.parametrize("S", [1, 2])
def test_two_term_formula_over_a_halo_tile_is_the_reference(O, dt, S):
    """4x5x16 -> 16 (every pixel of it is a border pixel or next to one); input and filter zero points at the ends of the type's range"""
    lo, hi = (0, 255) if dt == np.uint8 else (-128, 127)
    H, W, C, N = 4, 5, 16, 16
    OH, OW = -(-H // S), -(-W // S)
    rng = np.random.default_rng(415 + S)
    for izp, zend in ((lo, hi), (hi, lo), (lo, lo), (hi, hi)):
        x = rng.integers(lo, hi + 1, (H, W, C)).astype(dt)
        wd = rng.integers(lo, hi + 1, (3, 3, C)).astype(dt)
        zd = np.where(np.arange(C) % 2 == 0, zend, lo + hi - zend).astype(dt)     # per channel: both ends
        wp = rng.integers(lo, hi + 1, (N, C)).astype(dt)
        zp_ = np.where(np.arange(N) % 3 == 0, lo + hi - zend, zend).astype(dt)
        mid_zp = hi if izp == lo else lo                                            # the intermediate tensor's zero point at an end too
        cd = (0.05, mid_zp, 0, rng.uniform(-30, 30, C).astype(f32), (rng.uniform(0.5, 1.5, C) * 40.0 / (5476.0 * 3.0)).astype(f32))
        cp = (0.05, int(rng.integers(lo, lo + 100)), 3, rng.uniform(-30, 30, N).astype(f32), (rng.uniform(0.5, 1.5, N) * 40.0 / (5476.0 * 4.0)).astype(f32))
        want_mid = O.depthwise_conv_2d(x, wd, zd, izp, cd[0], cd[1], cd[2], 0, (S, S), (OH, OW), cd[3], cd[4])
        want = O.conv_2d(want_mid, wp.reshape(N, 1, 1, C), zp_, mid_zp, cp[0], cp[1], cp[2], 0, (1, 1), (OH, OW), cp[3], cp[4])
        got_mid, got = _two_term_pair(x, wd, zd, izp, cd, wp, zp_, mid_zp, cp, S, dt)
        assert np.array_equal(got_mid, want_mid), (izp, zend)
        assert np.array_equal(got, want), (izp, zend)
