"""block_band_rt (k_block_band.hip) without a GPU.  tests/cpp/block_match.cpp -- a stand-alone program with its own main, built with the
address and undefined-behaviour sanitizers on the host side and linked against the built library for the plan -- fills three
operators by hand and prints the verdicts of fused_impl.hpp's match_expand_block, the plans of k::block_band_plan and, per band, the
ranges k::block_band_rows gives the kernel.  The listing of the kernel file keeps the house rules: every instance exists, no scratch,
registers inside the launch bounds, three barriers per step and none reached with LDS operations pending."""
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
INSTANCES = 28                         # (k steps of E 1, 2: modes 1, 2; 4: modes 0, 1, 2) x k steps of C {1, 2} x {i8, u8}

# the six blocks of tests/test_gpu_expand_block.py: (H, W, C, E, S, N)
ACCEPTED = {"6x6x8-32-8": (6, 6, 8, 32, 1, 8), "9x7x16-64-24": (9, 7, 16, 64, 1, 24), "13x11x12-48-20": (13, 11, 12, 48, 1, 20),
            "10x10x24-144s2-32": (10, 10, 24, 144, 2, 32), "40x40x16-96-16": (40, 40, 16, 96, 1, 16), "34x30x32-256s2-64": (34, 30, 32, 256, 2, 64),
            "base": (12, 12, 16, 64, 1, 16)}
REFUSED = ["E_le_N", "E_le_C", "E_mod16", "E_272", "expand3x3", "expand_stride2", "expand_other_HW", "wzp_expand", "wzp_depthwise", "wzp_project",
           "element_type", "element_type_pair", "expand_not_finite", "depthwise_not_finite", "project_not_finite", "odd_width_stride2",
           "generic_expand", "generic_depthwise", "generic_project", "device", "dw5x5"]


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return hipcc


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    lib = os.path.join(ROOT, "microflow_rs_amd", "libmicroflow_amd.so")
    if not os.path.exists(lib):
        pytest.skip("libmicroflow_amd.so not built")
    exe = str(tmp_path_factory.mktemp("block_match") / "block_match")
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-x", "hip", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "block_match.cpp"), "-x", "none", lib,
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    by = {}
    for l in out.stdout.splitlines():
        name, rest = l.split(" ", 1)
        by[name] = rest
    return by


def _plan(line):
    f = line.split()
    assert f[0] == "ok", line
    p = {k: int(v) for k, v in (t.split("=") for t in f[1:] if not t.startswith("band="))}
    p["bands"] = [tuple(int(v) for v in t[5:].split(":")) for t in f[1:] if t.startswith("band=")]
    return p


def test_every_case_ran(verdicts):
    assert sorted(verdicts) == sorted(list(ACCEPTED) + REFUSED)


@pytest.mark.parametrize("case", REFUSED)
def test_refuses_what_is_not_a_block(verdicts, case):
    assert verdicts[case] == "no"


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_accepts_the_block_and_its_plan_holds(verdicts, case):
    H, W, C, E, S, N = ACCEPTED[case]
    p = _plan(verdicts[case])
    assert (p["H"], p["W"], p["CI"], p["E"], p["S"], p["N"], p["izp"]) == (H, W, C, E, S, N, 4)
    OH, OW = -(-H // S), -(-W // S)
    RB, NB, TR = p["RB"], p["NB"], p["TR"]
    assert RB % p["CY"] == 0 and p["CX"] * p["CY"] == 16 and p["UX"] == -(-OW // p["CX"]) and p["UY"] * p["CY"] == RB
    # (the column grid hangs over the row only where that computes fewer pixels per image than the grid that divides OW, or that one has no plan)
    padded = lambda cx: -(-OW // cx) * cx * (-(-OH // (16 // cx)) * (16 // cx))
    divides = max(c for c in (1, 2, 4, 8, 16) if OW % c == 0)
    no_plan = ((16 // divides - 1) * S + 3) * (W + 2) * E > LDS_MAX            # the dividing grid's smallest band: its tile alone is beyond the LDS
    assert p["CX"] == divides or padded(p["CX"]) < padded(divides) or no_plan
    assert no_plan == (case == "34x30x32-256s2-64")                             # (the one case that exists for it)
    assert NB * RB >= OH > (NB - 1) * RB
    assert TR == (RB - 1) * S + 3
    # the regions in order, 16-byte aligned, disjoint, inside the budget: input band, tile, MID, the step queue's slot
    assert p["in_off"] == 0 and p["in_bytes"] >= 15 + TR * W * C + 64 * p["KSI"] + 16       # the last pixel's whole k steps stay inside the region
    assert p["tile_off"] >= p["in_off"] + p["in_bytes"]
    assert p["ROW"] >= (W + 2) * E and p["ROW"] % 16 == 0 and p["TILE"] >= TR * p["ROW"]
    assert p["mid_off"] >= p["tile_off"] + p["TILE"]
    assert p["NCH"] == -(-RB * OW // 16) and p["mid_bytes"] == p["NCH"] * 16 * E
    assert p["q_off"] >= p["mid_off"] + p["mid_bytes"] and p["lds"] >= p["q_off"] + 8
    assert all(p[k] % 16 == 0 for k in ("in_off", "in_bytes", "tile_off", "TILE", "mid_off", "q_off", "lds"))
    assert p["lds"] <= LDS_MAX and p["wgs"] in (1, 2) and (p["wgs"] == 1 or p["lds"] <= HALF_LDS)
    # the instance and the project's blocks: whole (padded) tiles of N on at most eight waves
    assert p["KSC"] == (1 if E <= 64 else 2 if E <= 128 else 4) and p["KSI"] == (1 if C <= 64 else 2)
    assert p["TB"] * p["NBLK"] * 16 == -(-N // 16) * 16 and p["TB"] in ((1,) if p["KSC"] == 4 else (1, 2)) and 1 <= p["SLOTS"] and 1 <= p["NWB"] and p["SLOTS"] * p["NWB"] <= 8
    assert p["nfull"] == (1 if N % 16 == 0 else 0)
    # every band's staged range: the tile rows inside the image, one contiguous range of it that ends inside it
    assert len(p["bands"]) == NB
    for band, (lo_r, hi_r, start, length) in enumerate(p["bands"]):
        iy0 = S * band * RB - 1
        inside = [r for r in range(TR) if 0 <= iy0 + r < H]
        assert (lo_r, hi_r) == (inside[0], inside[-1] + 1), band
        assert start == (iy0 + lo_r) * W * C and length == (hi_r - lo_r) * W * C
        assert 0 <= start and start + length <= H * W * C
        assert (start % 16) + length + 15 <= p["in_bytes"]                  # with the bytes in front of an unaligned start and the round-up behind


def test_small_images_are_one_band(verdicts):
    for case in ("6x6x8-32-8", "9x7x16-64-24", "13x11x12-48-20", "10x10x24-144s2-32", "base"):
        assert _plan(verdicts[case])["NB"] == 1, case
    assert _plan(verdicts["40x40x16-96-16"])["NB"] >= 2 and _plan(verdicts["34x30x32-256s2-64"])["NB"] >= 2


# ---- the listing -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def listing():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k_block_band.s")
        # (the flags of tests/test_pair_band_host.py)
        subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mllvm",
                               "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "k_block_band.hip")],
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
    sec = text[text.index("### 4.16"):]
    assert re.search(r"\b%d instances\b" % INSTANCES, sec[:sec.index("\n## ") if "\n## " in sec else len(sec)])


def test_every_instance_exists_and_its_barriers_wait_for_lds(listing, abw):
    kernels = list(abw.kernels(listing))
    assert len(kernels) == INSTANCES, [n for n, _ in kernels]
    want = {"block_band_rt<%d, %d, %d, %du>" % (ke, kc, mg, xr) for ke in (1, 2, 4) for kc in (1, 2) for mg in ((0, 1, 2) if ke == 4 else (1, 2)) for xr in (0, 0x80808080)}
    assert {n for n, _ in kernels} == want, sorted({n for n, _ in kernels} ^ want)
    for name, body in kernels:
        assert sum(1 for l in body if l.strip().startswith("s_barrier")) == 3, name     # top of step | expand -> depthwise | depthwise -> project
        assert not abw.scan(body), (name, abw.scan(body))
    text = "\n".join(listing)
    assert "v_mfma_i32_16x16x64_i8" in text and "global_load_lds_dwordx4" in text


def test_no_scratch_and_registers_inside_the_launch_bounds(listing):
    """from the listing's metadata: 512 threads = 2 waves per SIMD per workgroup, two workgroups per CU: 128 registers per lane, every instance"""
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
