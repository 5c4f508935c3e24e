"""conv_pool_rt (k_conv_pool.hip) without a GPU: the listing of the kernel file keeps the house rules (every instance exists and
carries the kernel's name, no scratch, registers inside the launch bounds, no barrier reached with LDS operations pending, m0 written
inside asm blocks only, the matrix instruction is there), and the plan (k::conv_pool_plan, through tests/cpp/conv_pool_plan.cpp
linked against the built library) lays its regions out in order inside the budget, takes G and PB as DESIGN 4.17 rules them for the
shapes tests/test_gpu_conv_pool.py runs, and refuses what it must."""
import importlib.util
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "microflow_rs_amd", "csrc")
LDS_MAX = 159 * 1024                   # kernels.hpp CONV_GEMM_LDS_MAX
HALF_LDS = 80 * 1024                   # two workgroups per CU
INSTANCES = 36                         # AL {16, 4, 1} x filter zero points {no, yes} x modes {0, 1, 2} x {i8, u8} (MF_DISPATCH4)


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return hipcc


@pytest.fixture(scope="module")
def listing():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k_conv_pool.s")
        subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mllvm",
                               "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "k_conv_pool.hip")],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read().split("\n")


@pytest.fixture(scope="module")
def abw():
    spec = importlib.util.spec_from_file_location("asm_barrier_waits", os.path.join(ROOT, "scripts", "asm_barrier_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_instance_exists_and_its_barriers_wait_for_lds(listing, abw):
    kernels = list(abw.kernels(listing))
    assert len(kernels) == INSTANCES, [n for n, _ in kernels]
    want = {"conv_pool_rt<%d, %s, %d, %du>" % (al, wz, mg, xr) for al in (16, 4, 1) for wz in ("false", "true") for mg in (0, 1, 2) for xr in (0, 0x80808080)}
    assert {n for n, _ in kernels} == want, sorted({n for n, _ in kernels} ^ want)
    for name, body in kernels:
        assert name.startswith("conv_pool_rt<"), name
        # weights staged | top of step | tile staged | Y complete
        assert sum(1 for l in body if l.strip().startswith("s_barrier")) == 4, name
        assert not abw.scan(body), (name, abw.scan(body))
    text = "\n".join(listing)
    assert "v_mfma_i32_16x16x64_i8" in text and "global_load_lds_dwordx4" in text


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
    assert seen >= 2 * INSTANCES, seen           # the weights' DMA and the rows' in every instance


def test_no_scratch_and_registers_inside_the_launch_bounds(listing):
    """256 threads = one wave per SIMD per workgroup, two workgroups per CU: far inside 256 registers per lane; no spills, no scratch"""
    text = "\n".join(listing)
    meta = text[text.index("amdhsa.kernels:"):]
    meta = meta[:meta.index("\namdhsa.target:")]
    seen = 0
    for e in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s*(\S+)", e).group(1)
        seen += 1
        vgpr = int(re.search(r"\.vgpr_count:\s*(\d+)", e).group(1))
        agpr = re.search(r"\.agpr_count:\s*(\d+)", e)
        agpr = int(agpr.group(1)) if agpr else 0
        assert 0 < vgpr and vgpr + agpr <= 128, (name, vgpr, agpr)
        assert re.search(r"\.private_segment_fixed_size:\s*0\b", e), name
        assert re.search(r"\.vgpr_spill_count:\s*0\b", e), name
    assert seen == INSTANCES


def test_design_states_the_instance_count():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.17"):]
    assert re.search(r"\b%d instances\b" % INSTANCES, sec[:sec.index("\n## ") if "\n## " in sec else len(sec)])


# ---- the plan --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    lib = os.path.join(ROOT, "microflow_rs_amd", "libmicroflow_amd.so")
    if not os.path.exists(lib):
        pytest.skip("libmicroflow_amd.so not built")
    cxx = shutil.which("g++") or shutil.which("c++")
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(_hipcc()))), "include")
    if not cxx or not os.path.isdir(rocm_inc):
        pytest.skip("no host compiler / ROCm headers")
    out = str(tmp_path_factory.mktemp("conv_pool_plan") / "conv_pool_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", rocm_inc, os.path.join(ROOT, "tests", "cpp", "conv_pool_plan.cpp"),
                           lib, "-Wl,-rpath," + os.path.dirname(lib), "-o", out])
    return out


def plan(exe, H, W, C, N, K, S=1, same=False, wz=False, P=2, PS=2, psame=False):
    r = subprocess.run([exe] + [str(int(v)) for v in (H, W, C, N, K, K, S, same, wz, P, P, PS, psame)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.split()
    if f[0] == "none":
        return None
    assert f[0] == "ok", r.stdout
    p = {k: int(v) for k, v in (t.split("=") for t in f[1:] if not t.startswith("band="))}
    p["bands"] = [tuple(int(v) for v in t[5:].split(":")) for t in f[1:] if t.startswith("band=")]
    return p


# the shapes of tests/test_gpu_conv_pool.py and scripts/time_conv_pool.py: (H, W, C, N, K, options)
SHAPES = {
    "a": (28, 28, 1, 6, 5, dict()),
    "b": (12, 12, 6, 16, 5, dict()),
    "c": (16, 16, 3, 32, 3, dict(same=True)),
    "d": (12, 12, 8, 24, 3, dict(same=True, wz=True, P=3, psame=True)),
    "e": (11, 11, 4, 8, 3, dict()),
    "f": (16, 16, 16, 32, 3, dict(S=2, same=True)),
    "g": (8, 8, 64, 16, 3, dict(same=True)),
    "j": (64, 64, 4, 64, 3, dict(same=True)),
    "k": (48, 48, 8, 96, 3, dict(same=True, P=3, psame=True)),
    "cifar": (32, 32, 3, 32, 3, dict(same=True)),
    "wide": (16, 16, 32, 64, 3, dict(same=True)),
    "mono96": (96, 96, 1, 8, 3, dict(same=True)),
    "deep": (16, 16, 64, 64, 3, dict(same=True)),
}
BANDS = {"j": 2, "k": 2}


@pytest.mark.parametrize("case", sorted(SHAPES))
def test_plan_regions_and_step(plan_exe, case):
    H, W, C, N, K, kw = SHAPES[case]
    p = plan(plan_exe, H, W, C, N, K, **kw)
    assert p is not None
    S, P, PS = kw.get("S", 1), kw.get("P", 2), kw.get("PS", 2)
    KWCP = -(-K * C // 16) * 16
    KS, NT = -(-K * KWCP // 64), -(-N // 16)
    assert (p["KS"], p["NT"], p["TB"]) == (KS, NT, min(4, NT))
    tabb = KS * 16 + (KS * 64 if kw.get("wz") else 0) + NT * 256               # tap table, masks, the constants [Kc | A | S | wzp][NT 16]
    # the regions in order, 16-byte aligned, disjoint, inside the budget: weights, G tiles (+ 256 bytes behind them), Y, tap table, masks,
    # constants
    G, TILE, YIMG = p["G"], p["TILE"], p["YIMG"]
    assert p["xoff"] == NT * KS * 1024
    assert p["yoff"] == p["xoff"] + G * TILE + 256 and p["toff"] == p["yoff"] + G * YIMG and p["moff"] == p["toff"] + KS * 16
    assert p["coff"] == p["moff"] + (KS * 64 if kw.get("wz") else 0) and p["lds"] == p["coff"] + NT * 256 == p["toff"] + tabb and p["lds"] <= LDS_MAX
    assert all(p[k] % 16 == 0 for k in ("xoff", "yoff", "toff", "moff", "coff", "TILE", "YIMG", "ROW"))
    assert p["ntap"] == KS * 4 and p["nmask"] == KS * 16
    # the tile holds the rows the step's convolution rows read, a row the image row inside its halo and the last window's padded filter row
    assert p["RB"] == (p["CB"] - 1) * S + K and TILE == p["RB"] * p["ROW"] and TILE <= 48 * 1024
    padl = (K - 1) // 2 if kw.get("same") else 0
    assert p["LP"] >= padl * C and p["ROW"] >= p["LP"] + max(W * C, ((p["OW"] - 1) * S - padl) * C + KWCP + 4)
    # Y: an odd number of dwords per pixel that holds N bytes; an image of Y holds CB rows
    assert p["NP"] % 4 == 0 and (p["NP"] // 4) % 2 == 1 and N <= p["NP"] <= N + 7
    assert YIMG >= p["CB"] * p["OW"] * p["NP"]
    # the bands cover the pooled rows once, in order, and hold the convolution rows their windows read
    NB, PB, POH, OH = p["NB"], p["PB"], p["POH"], p["OH"]
    assert len(p["bands"]) == NB and NB * PB >= POH > (NB - 1) * PB
    pshy = (P - 1) // 2 if kw.get("psame") else 0
    assert p["pshy"] == pshy
    for b, (py0, py1, c0, c1) in enumerate(p["bands"]):
        assert (py0, py1) == (b * PB, min(POH, (b + 1) * PB))
        assert (c0, c1) == (max(0, py0 * PS - pshy), min(OH, (py1 - 1) * PS - pshy + P))
        assert 0 < c1 - c0 <= p["CB"]
    assert max(c1 - c0 for _, _, c0, c1 in p["bands"]) == p["CB"]
    # the step: whole images where one fits -- inside 80 KiB if that holds one, as many as fit up to 16 images and 48 KiB of tiles --
    # else bands, as few as fit
    per_img = TILE + YIMG
    fixed = p["xoff"] + tabb + 256
    if case in BANDS:
        assert G == 1 and NB == BANDS[case] and fixed + per_img <= LDS_MAX
        whole = ((OH - 1) * S + K) * p["ROW"] + OH * p["OW"] * p["NP"]
        assert fixed + whole > LDS_MAX                                      # one whole image does not fit
    else:
        assert NB == 1 and PB == POH
        budget = HALF_LDS if fixed + per_img <= HALF_LDS else LDS_MAX
        assert G == min(16, 48 * 1024 // TILE, (budget - fixed) // per_img) and G >= 1
        assert (p["lds"] <= HALF_LDS) == (budget == HALF_LDS)


def test_plan_takes_the_expected_steps(plan_exe):
    """the numbers DESIGN 4.17 quotes"""
    got = {c: plan(plan_exe, *SHAPES[c][:5], **SHAPES[c][5]) for c in SHAPES}
    assert {c: got[c]["G"] for c in "abcdefg"} == {"a": 9, "b": 16, "c": 7, "d": 12, "e": 16, "f": 9, "g": 7}
    assert (got["j"]["PB"], got["j"]["NB"], got["k"]["PB"], got["k"]["NB"]) == (16, 2, 12, 2)
    assert got["k"]["bands"] == [(0, 12, 0, 24), (12, 24, 23, 48)]            # row 23 is computed by both bands
    assert got["e"]["CB"] == 8 and got["e"]["OH"] == 9                        # the last convolution row is never computed


def test_plan_refuses(plan_exe):
    assert plan(plan_exe, 9, 9, 3, 8, 3, same=True) is None                   # (W C) % 4 != 0
    assert plan(plan_exe, 8, 8, 4, 8, 3, same=True, P=8, PS=8) is None        # a global pool
    assert plan(plan_exe, 8, 8, 128, 256, 3, same=True) is None               # 16 tiles x 18 k steps = 288 KiB of resident weights
    assert plan(plan_exe, 16, 16, 192, 16, 7, same=True) is None              # K' = 7 x 1344 = 9408: 147 k steps > 128
    assert plan(plan_exe, 8, 8, 4, 8, 3, same=True, P=4, PS=4) is not None    # (2 x 2 pooled pixels are not a global pool)
