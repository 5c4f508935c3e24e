"""block_slice_rt (k_block_slice.hip) without a GPU.  tests/cpp/block_slice_match.cpp -- a stand-alone program with its own main, built
with the address and undefined-behaviour sanitizers on the host side and linked against the built library for the plan -- fills three
operators by hand and prints the verdicts of fused_impl.hpp's match_expand_block_deep and the plans of k::block_slice_plan."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "microflow_rs_amd", "csrc")
LDS_MAX = 159 * 1024                   # kernels.hpp PAIR_BAND_LDS_MAX
# the blocks of tests/test_gpu_block_slice.py: (H, W, C, E, S, N, units per wave of the instance)
ACCEPTED = {"10x10x8-320s2-8": (10, 10, 8, 320, 2, 8, 1), "9x7x96-384-24": (9, 7, 96, 384, 1, 24, 2), "9x7x96-384-40": (9, 7, 96, 384, 1, 40, 4),
            "6x6x8-320-8": (6, 6, 8, 320, 1, 8, 1), "9x7x16-384-24": (9, 7, 16, 384, 1, 24, 2), "10x10x24-320s2-32": (10, 10, 24, 320, 2, 32, 1),
            "14x14x96-576-96": (14, 14, 96, 576, 1, 96, 16), "7x7x160-960-320": (7, 7, 160, 960, 1, 320, 16), "40x40x16-320-16": (40, 40, 16, 320, 1, 16, 8)}
REFUSED = ["E_272", "E_256", "E_le_N", "C_196", "N_324", "wzp_project", "odd_width_stride2"]


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    lib = os.path.join(ROOT, "microflow_rs_amd", "libmicroflow_amd.so")
    if not os.path.exists(hipcc) or not os.path.exists(lib):
        pytest.skip("hipcc or libmicroflow_amd.so not available")
    exe = str(tmp_path_factory.mktemp("block_slice_match") / "block_slice_match")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-x", "hip", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "block_slice_match.cpp"), "-x", "none", lib,
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return dict(l.split(" ", 1) for l in out.stdout.splitlines())


@pytest.mark.parametrize("case", REFUSED)
def test_refuses_what_is_outside_the_range(verdicts, case):
    assert sorted(verdicts) == sorted(list(ACCEPTED) + REFUSED) and verdicts[case] == "no"


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_accepts_the_block_and_its_plan_holds(verdicts, case):
    H, W, C, E, S, N, UPW = ACCEPTED[case]
    f = verdicts[case].split()
    assert f[0] == "ok", verdicts[case]
    p = {k: int(v) for k, v in (t.split("=") for t in f[1:])}
    assert (p["H"], p["W"], p["CI"], p["E"], p["S"], p["N"], p["izp"]) == (H, W, C, E, S, N, 4)
    OH, OW = -(-H // S), -(-W // S)
    assert p["NS"] * 64 == E and p["NT"] == -(-N // 16) and p["KSI"] == -(-C // 64)
    # the units fit eight waves of the instance's rectangle
    assert p["UPW"] == UPW and p["PC"] * p["PT"] == p["UPW"] and p["WC"] * p["WT"] == 8
    assert p["NCH"] == -(-p["RB"] * OW // 16) and p["NCH"] * p["NT"] <= 8 * p["UPW"]
    assert p["WC"] * p["PC"] >= p["NCH"] and p["WT"] * p["PT"] >= p["NT"]
    # the bands cover OH exactly: whole depthwise units per band, no band beyond the image
    assert p["RB"] % p["CY"] == 0 and p["NB"] * p["RB"] >= OH > (p["NB"] - 1) * p["RB"] and p["TR"] == (p["RB"] - 1) * S + 3
    assert (p["NB"] == 1) == (case != "40x40x16-320-16")
    # the regions in order, 16-byte aligned, disjoint, inside the budget: input band, slice tile, slice MID, the step queue's slot
    assert p["in_off"] == 0 and p["in_bytes"] >= 15 + p["TR"] * W * C + 64 * p["KSI"] + 16
    assert p["tile_off"] >= p["in_off"] + p["in_bytes"]
    assert p["ROW"] >= (W + 2) * 64 and p["ROW"] % 16 == 0 and p["TILE"] >= p["TR"] * p["ROW"]
    assert p["mid_off"] >= p["tile_off"] + p["TILE"] and p["mid_bytes"] == p["NCH"] * 16 * 64
    assert p["q_off"] >= p["mid_off"] + p["mid_bytes"] and p["lds"] >= p["q_off"] + 8
    assert all(p[k] % 16 == 0 for k in ("in_off", "in_bytes", "tile_off", "TILE", "mid_off", "q_off", "lds"))
    assert p["lds"] <= LDS_MAX and p["wgs"] in (1, 2)
