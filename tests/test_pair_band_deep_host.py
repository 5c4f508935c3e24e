"""k_pair_band_deep.hip without a GPU: the generated code keeps the house rules (every kernel a pair_band_deep_rt instance, no barrier
reached with LDS operations pending, the int8 matrix instruction and the LDS-DMA present, no scratch, at most 256 registers per lane),
and the band plan for 256 < C <= 512 (k::pair_band_deep_plan, through tests/cpp/pair_band_deep_plan.cpp linked against the built
library) for the shapes tests/test_gpu_pair_band_deep.py runs and scripts/time_pair_band.py --deep times."""
import importlib.util
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "microflow_rs_amd", "csrc")
LDS_MAX = 159 * 1024                   # kernels.hpp PAIR_BAND_LDS_MAX
INSTANCES = 6                          # epilogue modes 0, 1, 2 x {i8, u8}
REGS_MAX = 256                         # __launch_bounds__(512, 2): two waves per SIMD share its 512 registers per lane


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return hipcc


@pytest.fixture(scope="module")
def listing():
    src = "k_pair_band_deep.hip"
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, src + ".s")
        # (the flags of tests/test_pair_band_host.py)
        subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mllvm",
                               "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, src)],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read().split("\n")


@pytest.fixture(scope="module")
def abw():
    spec = importlib.util.spec_from_file_location("asm_barrier_waits", os.path.join(ROOT, "scripts", "asm_barrier_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_design_states_the_instance_count():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.14"):]
    assert re.search(r"\b%d instances\b" % INSTANCES, sec[:sec.index("\n## ") if "\n## " in sec else len(sec)])


def test_pair_band_deep_barriers_wait_for_lds(listing, abw):
    kernels = list(abw.kernels(listing))
    assert len(kernels) == INSTANCES, [n for n, _ in kernels]
    for name, body in kernels:
        assert name.startswith("pair_band_deep_rt<"), name
        assert sum(1 for l in body if l.strip().startswith("s_barrier")) >= 2, name    # top of step | depthwise -> pointwise
        assert not abw.scan(body), (name, abw.scan(body))


def test_pair_band_deep_runs_on_the_matrix_pipe_with_lds_dma_and_no_scratch(listing):
    text = "\n".join(listing)
    assert "v_mfma_i32_16x16x64_i8" in text
    assert "global_load_lds_dwordx4" in text
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == INSTANCES and set(sizes) == {"0"}, sizes


def test_pair_band_deep_registers_fit_two_waves_per_simd(listing):
    """from the listing's metadata: one entry per kernel; vector + accumulation registers per lane (gfx950's file is unified)"""
    text = "\n".join(listing)
    meta = text[text.index("amdhsa.kernels:"):]
    meta = meta[:meta.index("\namdhsa.target:")]
    entries = re.split(r"\n  - ", meta)[1:]
    assert len(entries) == INSTANCES, len(entries)
    for e in entries:
        name = re.search(r"\.name:\s*(\S+)", e).group(1)
        vgpr = int(re.search(r"\.vgpr_count:\s*(\d+)", e).group(1))
        agpr = re.search(r"\.agpr_count:\s*(\d+)", e)
        agpr = int(agpr.group(1)) if agpr else 0
        assert "pair_band_deep_rt" in name, name
        assert 0 < vgpr and vgpr + agpr <= REGS_MAX, (name, vgpr, agpr)
        assert re.search(r"\.vgpr_spill_count:\s*0\b", e), name
    # the kernel descriptors say the same: the next free register of the unified file
    nf = [int(v) for v in re.findall(r"\.amdhsa_next_free_vgpr\s+(\d+)", text)]
    assert len(nf) == INSTANCES and max(nf) <= REGS_MAX, nf


# ---- the plan ------------------------------------------------------------------------------------------------------------
def _exe(tmp_path_factory, name):
    lib = os.path.join(ROOT, "microflow_rs_amd", "libmicroflow_amd.so")
    if not os.path.exists(lib):
        pytest.skip("libmicroflow_amd.so not built")
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(_hipcc()))), "include")
    out = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", rocm_inc, os.path.join(ROOT, "tests", "cpp", name + ".cpp"),
                           lib, "-Wl,-rpath," + os.path.dirname(lib), "-o", out])
    return out


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return _exe(tmp_path_factory, "pair_band_deep_plan")


@pytest.fixture(scope="module")
def shallow_plan_exe(tmp_path_factory):
    return _exe(tmp_path_factory, "pair_band_plan")


KEYS = ["RB", "NB", "TR", "ROW", "TILE", "dbuf", "tile_off", "mid_off", "mid_bytes", "q_off", "lds", "wgs", "CX", "CY", "UX", "UY", "NCH", "TB", "NBLK",
        "SLOTS", "NWB", "KSC"]


def plan(exe, H, W, C, S, N):
    r = subprocess.run([exe] + [str(v) for v in (H, W, C, S, N)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.split()
    if f[0] == "none":
        return None
    assert len(f) == 1 + len(KEYS), f
    return dict(zip(KEYS, [int(x) for x in f[1:]]))


# (H, W, C, S, N): tests/test_gpu_pair_band_deep.py's cases, then the shapes scripts/time_pair_band.py --deep times
GPU_CASES = [(14, 14, 512, 1, 512), (8, 8, 512, 1, 528), (16, 16, 512, 2, 1024), (10, 10, 320, 1, 320), (12, 12, 272, 1, 288), (13, 7, 384, 1, 384),
             (8, 8, 512, 1, 512)]
TIMED = [(12, 12, 512, 1, 512), (10, 10, 512, 1, 512), (6, 6, 512, 1, 512), (14, 14, 384, 1, 384), (14, 14, 320, 1, 320), (14, 14, 512, 1, 256),
         (7, 7, 512, 1, 512)]
# the band count each shape must get; 1 = the whole image fits the budget in one band
BANDS = {(14, 14, 512, 1, 512): 2, (16, 16, 512, 2, 1024): 2, (12, 12, 512, 1, 512): 2, (10, 10, 512, 1, 512): 2, (14, 14, 384, 1, 384): 2,
         (14, 14, 320, 1, 320): 2, (14, 14, 512, 1, 256): 2}


@pytest.mark.parametrize("H,W,C,S,N", GPU_CASES + TIMED, ids=lambda v: str(v))
def test_pair_band_deep_plan_layout(plan_exe, H, W, C, S, N):
    p = plan(plan_exe, H, W, C, S, N)
    assert p is not None
    OH, OW = -(-H // S), -(-W // S)
    RB, NB = p["RB"], p["NB"]
    assert NB * RB >= OH > (NB - 1) * RB
    assert NB == BANDS.get((H, W, C, S, N), 1)
    assert p["TR"] == (RB - 1) * S + 3
    # the tile: whole halo'd rows, chain_rt's pixel layout
    assert p["ROW"] >= (W + 2) * C and p["ROW"] % 16 == 0 and p["TILE"] >= p["TR"] * p["ROW"]
    # the regions in order, 16-byte aligned, none overlapping: tile(s), MID, the step queue's slot
    ntile = 2 if p["dbuf"] else 1
    assert p["tile_off"] == 0 and p["mid_off"] >= p["tile_off"] + ntile * p["TILE"]
    assert p["q_off"] >= p["mid_off"] + p["mid_bytes"] and p["lds"] >= p["q_off"] + 8
    assert all(p[k] % 16 == 0 for k in ("tile_off", "TILE", "mid_off", "q_off", "lds"))
    assert p["lds"] <= LDS_MAX
    assert p["wgs"] == 1                                               # (256 registers: one workgroup per CU whatever the LDS)
    # the whole budget: the next band size up (before the bands are evened out) would not have fitted with one tile, or is the image
    CY = p["CY"]
    if NB > 1:
        nxt = (-(-OH // (NB - 1)) + CY - 1) // CY * CY                  # the fewest rows per band that NB - 1 bands would need
        tile = (((nxt - 1) * S + 3) * p["ROW"] + 255) & ~255
        assert tile + C // 16 * (-(-nxt * OW // 16)) * 256 + 16 > LDS_MAX
    # the tile is doubled exactly when two fit
    assert bool(p["dbuf"]) == (2 * p["TILE"] + p["mid_bytes"] + 16 <= LDS_MAX)
    # MID: the band's pixels rounded up to 16, times C
    assert p["NCH"] == -(-RB * OW // 16) and p["mid_bytes"] == p["NCH"] * 16 * C
    # the depthwise units tile the band exactly; the pointwise blocks cover N and fit the eight waves
    assert p["CX"] * p["CY"] == 16 and p["UX"] * p["CX"] == OW and p["UY"] * p["CY"] == RB
    assert OW % (2 * p["CX"]) != 0 or p["CX"] == 16                    # the largest power of two <= 16 dividing OW
    assert p["TB"] * p["NBLK"] * 16 == N and p["TB"] in (1, 2) and p["SLOTS"] * p["NWB"] <= 8 and p["SLOTS"] >= 1 and p["NWB"] >= 1
    assert p["KSC"] == 8


def test_pair_band_deep_plan_refuses_what_is_outside_its_range(plan_exe):
    assert plan(plan_exe, 28, 28, 256, 1, 256) is None                 # C <= 256: pair_band_rt's or chain_rt's
    assert plan(plan_exe, 14, 14, 64, 1, 64) is None
    assert plan(plan_exe, 7, 7, 1024, 1, 1024) is None                 # C > 512
    assert plan(plan_exe, 14, 14, 528, 1, 64) is None
    assert plan(plan_exe, 14, 14, 328, 1, 64) is None                  # C % 16 != 0
    assert plan(plan_exe, 14, 14, 512, 1, 40) is None                  # N % 16 != 0
    assert plan(plan_exe, 15, 15, 512, 2, 64) is None                  # odd width at stride 2
    # OW = 7: one-column units, 16-row bands, a tile of 33 rows x 8 KiB: the smallest band does not fit
    assert plan(plan_exe, 14, 14, 512, 2, 1024) is None


def test_pair_band_plan_still_refuses_more_than_256_channels(shallow_plan_exe):
    assert plan(shallow_plan_exe, 40, 40, 320, 1, 64) is None
