"""The explicit-pad entries of the run-time-geometry planners (k::conv_rows_plan_pads, conv_mm_plan_pads, conv_gemm_plan_pads,
dw_gemm_plan_pads) without a GPU, through tests/cpp/pad_conv_plan.cpp: with SAME's placement they fill the argument
block byte for byte as the pad_same entries do, and with a PAD's top / left rows and columns and the VALID-on-padded output size
the tile covers the furthest row and column any window reads."""
import os
import shutil
import subprocess

import pytest

from tests import pad_cases as P
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "microflow_rs_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from microflow_rs_amd import _lib
    _lib.lib()  # (builds the library where it is missing)
    lib = _lib.lib_path()
    cxx = shutil.which("g++") or shutil.which("c++")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    assert cxx and os.path.isdir(rocm_inc), "a host compiler and the ROCm headers are needed"
    out = str(tmp_path_factory.mktemp("pad_conv_plan") / "pad_conv_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", rocm_inc, os.path.join(ROOT, "tests", "cpp", "pad_conv_plan.cpp"),
                           lib, "-Wl,-rpath," + os.path.dirname(lib), "-o", out])
    return out


def run(exe, *args):
    r = subprocess.run([exe] + [str(int(a)) if not isinstance(a, str) else a for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (args, r.stdout + r.stderr)
    return r.stdout


ALL = dict(P.EVERY, **P.REFUSED)   # (the banded, small and many-step geometries of tests/test_gpu_pad_conv_steps.py included)


@pytest.mark.parametrize("name", list(ALL))
def test_same_placement_fills_the_block_as_the_pad_same_entry(exe, name):
    """(t, l) = ((K - 1) / 2, (K - 1) / 2) with SAME's OH / OW: byte-identical argument blocks and tables, for every planner that
    takes the geometry -- and the same refusal where one does not"""
    dw, H, W, C, K, S, pads, N, wz = ALL[name]
    seen = 0
    for as_dw in (False, True):  # (every planner is asked about the geometry, not only the one the operator routes to)
        got = dict(t.split("=") for t in run(exe, "same", as_dw, H, W, C, C if as_dw else N, K, K, S, wz and not as_dw).split())
        assert set(got) == {"conv_rows", "conv_mm", "conv_gemm", "dw_gemm"}, got
        assert "differ" not in got.values(), (name, as_dw, got)
        seen += sum(v == "same" for v in got.values())
    if (W * C) % 4 == 0:  # (whole-dword image rows: what every planner but conv_rows' one-channel byte form asks)
        assert seen, "no planner takes %s at all" % name


def _fields(line):
    f = line.split()
    return f[0], (None if f[1] == "none" else {k: int(v) for k, v in (t.split("=") for t in f[1:])})


@pytest.mark.parametrize("name", list(ALL))
def test_the_tile_covers_every_window_of_the_padded_geometry(exe, name):
    """the PAD's (top, left) and the VALID-on-padded OH / OW: every row and column a window reads lies inside the tile the plan sizes
    -- also below and right of the image, where the reach may be further than SAME's ever was"""
    dw, H, W, C, K, S, (t, b, l, r), N, wz = ALL[name]
    OH, OW = P.out_hw(ALL[name])
    plans = dict(_fields(line) for line in run(exe, "pads", dw, H, W, C, N, K, K, S, wz, t, l, OH, OW).splitlines())
    assert set(plans) == {"conv_rows", "conv_mm", "conv_gemm", "dw_gemm"}
    if name in P.REFUSED:
        assert all(p is None for p in plans.values()), plans
        return
    last_row, last_col = (OH - 1) * S + K, (OW - 1) * S + K  # one past the furthest padded row / column a window reads
    assert last_row <= t + H + b and last_col <= l + W + r
    for planner, p in plans.items():
        if p is None:
            continue
        if planner == "conv_rows":
            assert p["shy"] == t and p["X0"] == p["XO"] - l * C and p["X0"] >= 0 and p["XO"] % 4 == 0
            assert max(last_row, t + H) * p["TWP"] <= p["TILE"]                 # rows: the windows' and the image's
            assert p["X0"] + last_col * C <= p["TWP"] and p["XO"] + W * C <= p["TWP"]
            # (a window row is read as KG + 1 aligned dwords from its first byte's dword)
            assert ((p["X0"] + (OW - 1) * S * C) & ~3) + 4 * (p["KG"] + 1) <= p["TWP"]
        else:
            assert p["padt"] == t and p["padl"] == l and p["LP"] % 16 == 0 and p["LP"] >= l * C
            assert p["LP"] + max((last_col - l) * C, W * C) <= p["ROW"]       # columns: the last window's last tap, the image row
            assert p["TILE"] == p["RB"] * p["ROW"]
            if p["NBANDS"] == 1:
                assert p["BH"] == OH and p["RB"] >= last_row
            else:
                assert p["BH"] * p["NBANDS"] >= OH and p["RB"] >= (p["BH"] - 1) * S + K and p["G"] == 1


def _plans(exe, case):
    dw, H, W, C, K, S, (t, b, l, r), N, wz = case
    OH, OW = P.out_hw(case)
    return dict(_fields(line) for line in run(exe, "pads", dw, H, W, C, N, K, K, S, wz, t, l, OH, OW).splitlines())


def _routed(plans, dw):
    """the planner op_create_padded_conv's route order ends at: conv_rows, dw_mm (conv_mm_plan_pads in its depthwise mode: the conv_mm
    line of a depthwise), dw_gemm, conv_mm, conv_gemm"""
    for planner in ("conv_rows", "conv_mm", "dw_gemm", "conv_gemm"):
        if plans[planner] is not None:
            return ("dw_mm" if dw and planner == "conv_mm" else planner), plans[planner]
    return None, None


def test_every_pinned_case_is_a_case():
    assert set(P.PINNED) == set(P.BANDED) | set(P.SMALL) | set(P.MANY_STEPS)
    assert set(P.MANY_STEPS) <= set(P.EVERY) and set(P.SMALL_BATCH) <= set(P.SMALL) and set(P.BYTE_FORM) <= set(P.SMALL)


@pytest.mark.parametrize("name", list(P.PINNED))
def test_the_plans_the_gpu_tests_rest_on(exe, name):
    """what tests/test_gpu_pad_conv_steps.py takes for granted about the planner the group routes to: the bands and their height, a
    ragged last band, the images per step, conv_mm_rt's 1024-thread form, image and step bases off the dword boundary"""
    case = P.EVERY[name]
    dw, H, W, C, K, S, pads, N, wz = case
    OH, OW = P.out_hw(case)
    planner, want, ragged = P.PINNED[name]
    got_planner, p = _routed(_plans(exe, case), dw)
    assert got_planner == planner, (name, got_planner)
    assert {k: p[k] for k in want} == want, (name, p)
    if name in P.BANDED:
        assert p["NBANDS"] >= 2 and p["G"] == 1, p
        assert (OH % p["BH"] != 0) == ragged and (p["NBANDS"] - 1) * p["BH"] < OH <= p["NBANDS"] * p["BH"], (OH, p)
    else:
        assert planner == "conv_rows" or p["NBANDS"] == 1, p
    G = p["G"]
    batch = P.SMALL_BATCH.get(name, 4 if name in P.BANDED else 5)
    if name in P.SMALL_BATCH:
        assert batch // G >= 3 and 0 < batch % G < G, (batch, G)              # several steps and a ragged last one
    if name in P.BYTE_FORM:
        assert planner == "conv_rows" and C == 3 and (W * C) % 4 != 0 and (H * W * C) % 4 != 0
    if name.startswith("conv3s2_45x31x3"):
        assert (G * H * W * C) % 2 == 1 and G * H * W * C < 32768           # consecutive steps start at byte shifts 0, 3, 2, 1
    if name in P.MANY_STEPS:
        g, nthr, batch = P.MANY_STEPS[name]
        assert g == G and nthr == p.get("NTHR", 512 if planner == "conv_rows" else 256), (name, p)
        steps, r = divmod(batch, G)
        assert 0 < r < G and steps >= 2 * 256 * (2048 // nthr) + 1
        assert batch * (H * W * C + OH * OW * (C if dw else N)) < 256 << 20


def test_pads_beyond_the_filter_put_whole_windows_in_fill():
    for name in ("conv3s1_10x8x16_p3", "dw3s1_10x8x16_p3", "conv3s1_9x9x3_p4"):
        dw, H, W, C, K, S, (t, b, l, r), N, wz = P.SMALL[name]
        assert min(t, b, l, r) >= K
    for name in ("conv3s1_71x48x16_tl", "dw3s1_71x48x16_tl"):
        dw, H, W, C, K, S, (t, b, l, r), N, wz = P.BANDED[name]
        assert b == 0 and r == 0 and t > (K - 1) // 2 and l > (K - 1) // 2
