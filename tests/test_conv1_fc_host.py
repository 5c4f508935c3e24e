"""k_conv1_fc.hip without a GPU: the generated code keeps the house rules (every kernel an instance of conv1_fc_rt, no barrier reached
with LDS operations pending, M0 written only inside the LDS-DMA helper's asm, the int8 matrix instruction, no scratch), and the
plan (k::conv1_fc_plan, through tests/cpp/conv1_fc_plan.cpp linked against the built library) for the shapes
tests/test_gpu_conv1_fc.py runs and for everything it must refuse."""
import importlib.util
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from tests.conftest import ROOT
from tests.conv1_fc_cases import CASES, out_hw

CSRC = os.path.join(ROOT, "microflow_rs_amd", "csrc")
FC_RT_LDS_MAX = 160 * 1024 - 1024      # kernels.hpp: the per-workgroup budget
FRONT = 64                             # kernels.hpp: CONV1_FC_BAND_FRONT


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return hipcc


@pytest.fixture(scope="module")
def listing():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k_conv1_fc.s")
        subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mllvm",
                               "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "k_conv1_fc.hip")],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read().split("\n")


@pytest.fixture(scope="module")
def abw():
    spec = importlib.util.spec_from_file_location("asm_barrier_waits", os.path.join(ROOT, "scripts", "asm_barrier_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_kernel_is_conv1_fc_rt_and_its_barriers_wait_for_lds(listing, abw):
    kernels = list(abw.kernels(listing))
    assert len(kernels) == 6, [n for n, _ in kernels]                  # 3 epilogue modes x 2 element types
    for name, body in kernels:
        assert name.startswith("conv1_fc_rt<"), name
        assert sum(1 for l in body if l.strip().startswith("s_barrier")) >= 5, name   # halo, tiles, band, sums, tile (, softmax)
        assert not abw.scan(body), (name, abw.scan(body))


def test_m0_only_inside_asm(listing):
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
    assert seen >= 6, seen


def test_matrix_pipe_and_no_scratch(listing):
    text = "\n".join(listing)
    assert "v_mfma_i32_16x16x64_i8" in text
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == 6 and set(sizes) == {"0"}, sizes


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
    out = str(tmp_path_factory.mktemp("conv1_fc_plan") / "conv1_fc_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", rocm_inc, os.path.join(ROOT, "tests", "cpp", "conv1_fc_plan.cpp"),
                           lib, "-Wl,-rpath," + os.path.dirname(lib), "-o", out])
    return out


KEYS = ["BH", "NB", "KS", "NT", "lds", "wres", "PP", "NRT", "KSC", "XO", "PITCH", "TROWS", "TILE", "BP", "toff", "tbytes", "boff", "qoff", "aoff", "poff"]


def plan(exe, H, W, N, KH, KW, sh, sw, same, nfc, wz=0, finite=1):
    r = subprocess.run([exe] + [str(int(v)) for v in (H, W, N, KH, KW, sh, sw, same, nfc, wz, finite)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.split()
    if f[0] == "none":
        return None
    return dict(zip(KEYS, [int(x) for x in f[1:]]))


def plan_case(exe, name):
    (H, W), (_, N, KH, KW, (sh, sw), padding), classes = CASES[name][:3]
    return plan(exe, H, W, N, KH, KW, sh, sw, padding == "same", classes)


# bands (rows per band, bands), k steps and whether the FullyConnected image is resident, worked out by hand from the rule "the
# fewest output rows with at least 256 bytes of k"
WANT = {"a": (4, 3, 10, 1), "b": (5, 1, 2, 1), "c": (3, 3, 12, 1), "d": (6, 2, 8, 1), "e": (1, 25, 125, 0), "f": (2, 13, 63, 1), "g": (7, 2, 7, 1)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_of_the_gpu_cases(plan_exe, name):
    p = plan_case(plan_exe, name)
    assert p is not None, name
    shape, stem, classes = CASES[name][:3]
    (H, W), (_, N, KH, KW, (sh, sw), padding) = shape, stem
    OH, OW = out_hw(shape, stem)
    K = OH * OW * N
    assert (p["BH"], p["NB"], p["KS"], p["wres"]) == WANT[name], p
    assert p["NB"] == -(-OH // p["BH"]) and p["KS"] == -(-K // 64) and p["NT"] == -(-classes // 16)
    assert p["BH"] == OH or p["BH"] * OW * N >= 256 > (p["BH"] - 1) * OW * N
    assert p["lds"] <= FC_RT_LDS_MAX
    # the convolution's product: PP pixels x N channels in NRT tiles of 16 rows, their windows inside 16 bytes; four filter rows per k step
    assert p["PP"] * N <= 16 * p["NRT"] and KW + (p["PP"] - 1) * sw <= 16 and p["PP"] in (1, 2, 4) and p["NRT"] in (1, 2)
    assert p["KSC"] == -(-KH // 4)
    # a tile: every window row inside it, the halos as wide as SAME needs, image column 0 on a dword, the bank phases
    padt, padl = ((KH - 1) // 2, (KW - 1) // 2) if padding == "same" else (0, 0)
    padb, padr = max((OH - 1) * sh - padt + KH - H, 0), max((OW - 1) * sw - padl + KW - W, 0)
    assert p["TROWS"] == padt + H + padb and p["XO"] % 4 == 0 and p["XO"] >= max(padl, padr)
    assert p["PITCH"] >= W + p["XO"] and p["PITCH"] % 4 == 0 and (p["PITCH"] // 4) % 2 == 1
    assert p["TILE"] >= p["TROWS"] * p["PITCH"] and (p["TILE"] // 4) % 64 == 4
    assert p["tbytes"] >= 16 * p["TILE"] + 36 + padr                   # (the 20 bytes an operand read takes past a window's 16)
    # a band buffer row: the front a k step may start in, the band, the rest of its last k step
    assert p["BP"] >= FRONT + p["BH"] * OW * N + 64 and (p["BP"] // 4) % 64 == 4
    # the regions in order, none overlapping
    assert p["toff"] == (p["NT"] * p["KS"] * 1024 if p["wres"] else 0)
    assert p["boff"] == p["toff"] + p["tbytes"] and p["qoff"] == p["boff"] + 2 * 16 * p["BP"]
    assert p["aoff"] >= p["qoff"] + 4 * p["NT"] * 1024 + 4 * 16 * 4 and p["poff"] >= p["aoff"] + 16 * classes
    assert p["lds"] >= p["poff"] + 16 * classes + 15                   # (the patch sits at the output's 16-byte phase)
    assert all(p[k] % 16 == 0 for k in ("toff", "tbytes", "boff", "qoff", "aoff", "poff"))


def test_plan_refuses_what_the_kernel_does_not_take(plan_exe):
    ok = plan(plan_exe, 12, 8, 8, 3, 3, 1, 1, 1, 6)
    assert ok is not None
    assert plan(plan_exe, 12, 10, 8, 3, 3, 1, 1, 1, 6) is None         # W % 4 != 0
    assert plan(plan_exe, 12, 8, 6, 3, 3, 1, 1, 1, 6) is None          # N = 6
    assert plan(plan_exe, 12, 8, 36, 3, 3, 1, 1, 1, 6) is None         # N > 32
    assert plan(plan_exe, 6, 20, 4, 2, 17, 1, 1, 1, 6) is None         # KW = 17
    assert plan(plan_exe, 20, 8, 4, 17, 2, 1, 1, 1, 6) is None         # KH = 17
    assert plan(plan_exe, 12, 8, 8, 3, 3, 3, 1, 1, 6) is None          # stride 3
    assert plan(plan_exe, 8, 8, 8, 3, 3, 1, 1, 1, 65) is None          # N_fc = 65
    assert plan(plan_exe, 8, 8, 8, 3, 3, 1, 1, 1, 64) is not None
    assert plan(plan_exe, 200, 64, 4, 3, 3, 2, 2, 1, 6) is None        # sixteen 202 x 68 tiles: 220 KiB
    assert plan(plan_exe, 12, 8, 8, 3, 3, 1, 1, 1, 6, wz=1) is None    # filter zero points
    assert plan(plan_exe, 12, 8, 8, 3, 3, 1, 1, 1, 6, finite=0) is None
    assert plan(plan_exe, 49, 40, 8, 10, 8, 2, 2, 1, 4) is None        # speech.tflite's geometry: dwc1_fc_softmax's
    assert plan(plan_exe, 49, 40, 8, 10, 8, 2, 2, 1, 12) is not None   # ... with 12 keywords
    assert plan(plan_exe, 49, 40, 8, 10, 8, 2, 2, 0, 4) is not None    # ... VALID
