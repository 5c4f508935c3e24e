"""k_pair_band.hip without a GPU: the generated code keeps the house rules (every kernel a pair_band_rt instance, no barrier reached
with LDS operations pending, M0 written only inside the LDS-DMA helper's asm, the int8 matrix instruction and the LDS-DMA present, no
scratch), and the band plan (k::pair_band_plan, through tests/cpp/pair_band_plan.cpp linked against the built library) for the
MobileNet-v1-224 pairs and the shapes tests/test_gpu_pair_band.py runs."""
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
HALF_LDS = 80 * 1024 - 512             # kernels.hpp PAIR_BAND_LDS_HALF: two workgroups per CU
INSTANCES = 14                         # (KS 1, 2: modes 1, 2; KS 4: modes 0, 1, 2) x {i8, u8}


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return hipcc


def _listing(src):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, src + ".s")
        subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mllvm",
                               "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, src)],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read().split("\n")


@pytest.fixture(scope="module")
def listing():
    return _listing("k_pair_band.hip")


@pytest.fixture(scope="module")
def abw():
    spec = importlib.util.spec_from_file_location("asm_barrier_waits", os.path.join(ROOT, "scripts", "asm_barrier_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_design_states_the_instance_count():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.13"):]
    assert re.search(r"\b%d instances\b" % INSTANCES, sec[:sec.index("\n## ") if "\n## " in sec else len(sec)])


def test_pair_band_barriers_wait_for_lds(listing, abw):
    kernels = list(abw.kernels(listing))
    assert len(kernels) == INSTANCES, [n for n, _ in kernels]
    for name, body in kernels:
        assert name.startswith("pair_band_rt<"), name
        assert sum(1 for l in body if l.strip().startswith("s_barrier")) >= 2, name    # top of step | depthwise -> pointwise
        assert not abw.scan(body), (name, abw.scan(body))


def test_pair_band_m0_only_inside_asm(listing):
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


def test_pair_band_runs_on_the_matrix_pipe_with_lds_dma_and_no_scratch(listing):
    text = "\n".join(listing)
    assert "v_mfma_i32_16x16x64_i8" in text
    assert "global_load_lds_dwordx4" in text
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == INSTANCES and set(sizes) == {"0"}, sizes


# ---- the plan ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    lib = os.path.join(ROOT, "microflow_rs_amd", "libmicroflow_amd.so")
    if not os.path.exists(lib):
        pytest.skip("libmicroflow_amd.so not built")
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(_hipcc()))), "include")
    out = str(tmp_path_factory.mktemp("pair_band_plan") / "pair_band_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", rocm_inc, os.path.join(ROOT, "tests", "cpp", "pair_band_plan.cpp"),
                           lib, "-Wl,-rpath," + os.path.dirname(lib), "-o", out])
    return out


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


# (H, W, C, S, N): the first six pairs of a MobileNet-v1 at 224 x 224, then tests/test_gpu_pair_band.py's cases
MOBILENET = [(112, 112, 32, 1, 64), (112, 112, 64, 2, 128), (56, 56, 128, 1, 128), (56, 56, 128, 2, 256), (28, 28, 256, 1, 256), (28, 28, 256, 2, 512)]
GPU_CASES = [(36, 36, 64, 1, 64), (38, 40, 64, 1, 48), (50, 32, 128, 2, 256), (20, 20, 256, 1, 32), (37, 41, 64, 1, 64), (40, 40, 64, 1, 64),
             (57, 21, 64, 1, 64), (44, 44, 96, 1, 64), (30, 30, 192, 1, 288), (20, 20, 256, 1, 272)]


@pytest.mark.parametrize("H,W,C,S,N", MOBILENET + GPU_CASES, ids=lambda v: str(v))
def test_pair_band_plan_layout(plan_exe, H, W, C, S, N):
    p = plan(plan_exe, H, W, C, S, N)
    assert p is not None
    OH, OW = -(-H // S), -(-W // S)
    RB, NB = p["RB"], p["NB"]
    assert NB * RB >= OH > (NB - 1) * RB
    assert p["TR"] == (RB - 1) * S + 3
    # the tile: whole halo'd rows, chain_rt's pixel layout
    assert p["ROW"] >= (W + 2) * C and p["ROW"] % 16 == 0 and p["TILE"] >= p["TR"] * p["ROW"]
    # the regions in order, 16-byte aligned, none overlapping: tile(s), MID, the step queue's slot
    ntile = 2 if p["dbuf"] else 1
    assert p["tile_off"] == 0 and p["mid_off"] >= p["tile_off"] + ntile * p["TILE"]
    assert p["q_off"] >= p["mid_off"] + p["mid_bytes"] and p["lds"] >= p["q_off"] + 8
    assert all(p[k] % 16 == 0 for k in ("tile_off", "TILE", "mid_off", "q_off", "lds"))
    assert p["lds"] <= LDS_MAX
    assert p["wgs"] in (1, 2) and (p["wgs"] == 1 or p["lds"] <= HALF_LDS)
    assert p["wgs"] == 1 or C <= 128                                   # (four k steps: 180 registers, one workgroup per CU whatever the LDS)
    # MID: the band's pixels rounded up to 16, times C
    assert p["NCH"] == -(-RB * OW // 16) and p["mid_bytes"] == p["NCH"] * 16 * C
    # the depthwise units tile the band exactly; the pointwise blocks cover N and fit the eight waves
    assert p["CX"] * p["CY"] == 16 and p["UX"] * p["CX"] == OW and p["UY"] * p["CY"] == RB
    assert p["TB"] * p["NBLK"] * 16 == N and p["TB"] in (1, 2) and p["SLOTS"] * p["NWB"] <= 8 and p["SLOTS"] >= 1 and p["NWB"] >= 1
    assert p["KSC"] == (1 if C <= 64 else 2 if C <= 128 else 4)


def test_pair_band_plan_refuses_what_is_not_a_band_pair(plan_exe):
    assert plan(plan_exe, 12, 12, 64, 1, 64) is None                   # below the size bound (a table pair; chain_rt could hold it)
    assert plan(plan_exe, 40, 40, 24, 1, 32) is None                   # C % 16 != 0
    assert plan(plan_exe, 40, 40, 320, 1, 64) is None                  # C > 256
    assert plan(plan_exe, 40, 40, 64, 1, 20) is None                   # N % 16 != 0
    assert plan(plan_exe, 41, 41, 64, 2, 64) is None                   # odd width at stride 2
