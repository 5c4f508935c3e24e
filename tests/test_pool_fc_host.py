"""k_pool_fc.hip without a GPU: the generated code keeps the house rules (no barrier reached with LDS operations pending, M0
written only inside the LDS-DMA helper's asm, the int8 matrix instruction, no scratch); k_fc_rt.hip still holds its 18 kernels
now that the layer step lives in k_fc_layer.hpp; and the LDS plan (k::pool_fc_plan, through tests/cpp/pool_fc_plan.cpp linked
against the built library) for the shapes tests/test_gpu_pool_fc.py runs."""
import importlib.util
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "microflow_rs_amd", "csrc")
FC_RT_LDS_MAX = 160 * 1024 - 1024      # kernels.hpp
HALF_LDS = 80 * 1024 - 512             # k_pool_fc.hip: two workgroups per CU


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
    return _listing("k_pool_fc.hip")


@pytest.fixture(scope="module")
def abw():
    spec = importlib.util.spec_from_file_location("asm_barrier_waits", os.path.join(ROOT, "scripts", "asm_barrier_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pool_fc_barriers_wait_for_lds(listing, abw):
    kernels = list(abw.kernels(listing))
    # 3 epilogue modes x 2 element types, as fc_chain
    assert len(kernels) == 6, [n for n, _ in kernels]
    for name, body in kernels:
        assert name.startswith("pool_fc_chain<"), name
        assert sum(1 for l in body if l.strip().startswith("s_barrier")) >= 3, name   # pool -> layer -> (softmax ->) patch
        assert not abw.scan(body), (name, abw.scan(body))


def test_pool_fc_m0_only_inside_asm(listing):
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


def test_pool_fc_runs_on_the_matrix_pipe_without_scratch(listing):
    text = "\n".join(listing)
    assert "v_mfma_i32_16x16x64_i8" in text
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == 6 and set(sizes) == {"0"}, sizes


def test_fc_rt_keeps_its_kernels_after_the_header_move(abw):
    kernels = list(abw.kernels(_listing("k_fc_rt.hip")))
    assert len(kernels) == 18, [n for n, _ in kernels]
    assert sum(1 for n, _ in kernels if n.startswith("fc_rt<")) == 12 and sum(1 for n, _ in kernels if n.startswith("fc_chain<")) == 6
    for name, body in kernels:
        assert not abw.scan(body), (name, abw.scan(body))


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
    out = str(tmp_path_factory.mktemp("pool_fc_plan") / "pool_fc_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", rocm_inc, os.path.join(ROOT, "tests", "cpp", "pool_fc_plan.cpp"),
                           lib, "-Wl,-rpath," + os.path.dirname(lib), "-o", out])
    return out


def plan(exe, H, W, C, sizes, softmax):
    r = subprocess.run([exe, str(H), str(W), str(C), str(int(softmax))] + [str(n) for n in sizes], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.split()
    if f[0] == "none":
        return None
    v = [int(x) for x in f[1:]]
    keys = ["R", "lds", "xoff", "xbytes", "aoff", "abytes", "poff", "CGW", "NS", "NPASS", "NIT"]
    d = dict(zip(keys, v))
    d["woff"] = v[len(keys):]
    return d


# (H, W, C, sizes, softmax): tests/test_gpu_pool_fc.py's cases
SHAPES = [(2, 2, 256, (10,), True), (3, 3, 256, (2,), True), (7, 7, 64, (10,), True), (4, 4, 96, (12,), False), (14, 14, 16, (20,), True),
          (1, 1, 32, (5,), False), (5, 5, 320, (17, 10), True), (8, 8, 128, (100, 10), False), (7, 7, 1024, (10,), True)]


@pytest.mark.parametrize("H,W,C,sizes,softmax", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_pool_fc_plan_lds_layout(plan_exe, H, W, C, sizes, softmax):
    p = plan(plan_exe, H, W, C, sizes, softmax)
    assert p is not None
    R = p["R"]
    assert R % 16 == 0 and 16 <= R <= 128
    # the regions in order, none overlapping: layer images, the pooled [R][C] tile, two activation tiles, the patch
    K, W_end = C, 0
    for l, N in enumerate(sizes):
        assert p["woff"][l] == W_end and W_end % 1024 == 0
        W_end += -(-N // 16) * -(-K // 64) * 1024
        K = N
    assert p["xoff"] == W_end and p["xbytes"] >= R * C + 20           # (+ the 20 bytes a 16-byte operand piece reads past a row)
    assert p["aoff"] == p["xoff"] + p["xbytes"]
    nmax = max([n for n in sizes[:-1]] + ([sizes[-1]] if softmax else []) + [0])
    assert p["abytes"] >= R * nmax + 20 and p["poff"] == p["aoff"] + 2 * p["abytes"]
    assert p["lds"] >= p["poff"] + R * sizes[-1] + 15                  # (the patch sits at the output's 16-byte phase)
    assert all(v % 16 == 0 for v in (p["xoff"], p["aoff"], p["poff"], p["lds"]))
    assert p["lds"] <= HALF_LDS                                        # these weights leave room for two workgroups per CU
    # the pool product: CGW channel groups x NS pixel subsets fill at most the 16 columns; NPASS x 16 groups cover C; NIT loads the pixels
    CG = C // 16
    assert p["CGW"] == min(CG, 16) and p["NS"] == 16 // p["CGW"] and p["CGW"] * p["NS"] <= 16
    assert p["NPASS"] * 16 >= CG > (p["NPASS"] - 1) * 16
    assert p["NIT"] * 4 * p["NS"] >= H * W > (p["NIT"] - 1) * 4 * p["NS"]


def test_pool_fc_plan_refuses_what_does_not_fit(plan_exe):
    assert plan(plan_exe, 2, 2, 256, (1000,), True) is None            # 63 tiles x 4 k steps = 252 KiB of weights
    assert plan(plan_exe, 4, 4, 24, (10,), True) is None               # C % 16 != 0
    big = plan(plan_exe, 2, 2, 1024, (100,), False)                    # 112 KiB of weights: one workgroup per CU, inside the budget
    assert big is not None and HALF_LDS < big["lds"] <= FC_RT_LDS_MAX and big["R"] % 16 == 0
