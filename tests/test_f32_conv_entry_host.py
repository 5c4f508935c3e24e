"""The f32-entry instances of conv_rows_lds (k_rt.hip) without a GPU: the generated code has them (conv_rows_lds_f32: one per int8
instance), with no scratch, registers inside their launch bounds and no barrier reached with LDS operations pending; and the plans
(k::conv_rows_plan, k::conv_gemm_plan through tests/cpp/conv_entry_plan.cpp linked against the built library) give the images per
step, bands and slices that tests/test_gpu_f32_conv_entry.py's batches and cases rest on.  (conv_gemm_rt has no f32 instance: DESIGN 6.)"""
import importlib.util
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "microflow_rs_amd", "csrc")
# file -> (int8 kernel, f32 kernel, instances of each, registers per lane that the launch bound leaves: 512 per SIMD lane, shared by
# the waves of a workgroup on that SIMD -- 512 threads = 2 waves per SIMD at __launch_bounds__(512), one at (256))
FILES = {"k_rt.hip": ("conv_rows_lds", "conv_rows_lds_f32", 12, 128)}       # {wzp, none} x modes 0, 1, 2 x {i8, u8}


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return hipcc


@pytest.fixture(scope="module", params=sorted(FILES))
def listing(request):
    src = request.param
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, src + ".s")
        # (the flags of tests/test_pair_band_host.py)
        subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mllvm",
                               "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, src)],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return src, open(out).read().split("\n")


@pytest.fixture(scope="module")
def abw():
    spec = importlib.util.spec_from_file_location("asm_barrier_waits", os.path.join(ROOT, "scripts", "asm_barrier_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_f32_instances_exist_and_their_barriers_wait_for_lds(listing, abw):
    src, lines = listing
    i8, f32, count, _ = FILES[src]
    kernels = list(abw.kernels(lines))
    mine = [(n, b) for n, b in kernels if n.startswith(f32 + "<")]
    assert len(mine) == count, (src, [n for n, _ in mine])
    assert len([n for n, _ in kernels if n.startswith(i8 + "<")]) == count       # the int8 instances keep their names
    for name, body in mine:
        assert sum(1 for l in body if l.strip().startswith("s_barrier")) >= 2, name    # top of step | tiles staged
        assert not abw.scan(body), (name, abw.scan(body))


def test_f32_instances_use_no_scratch_and_fit_their_launch_bounds(listing):
    """from the listing's metadata: one entry per kernel; vector + accumulation registers per lane (gfx950's file is unified)"""
    src, lines = listing
    _, f32, count, regs_max = FILES[src]
    text = "\n".join(lines)
    meta = text[text.index("amdhsa.kernels:"):]
    meta = meta[:meta.index("\namdhsa.target:")]
    seen = 0
    for e in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s*(\S+)", e).group(1)
        if f32 not in name:
            continue
        seen += 1
        vgpr = int(re.search(r"\.vgpr_count:\s*(\d+)", e).group(1))
        agpr = re.search(r"\.agpr_count:\s*(\d+)", e)
        agpr = int(agpr.group(1)) if agpr else 0
        assert 0 < vgpr and vgpr + agpr <= regs_max, (name, vgpr, agpr)
        assert re.search(r"\.private_segment_fixed_size:\s*0\b", e), name
        assert re.search(r"\.vgpr_spill_count:\s*0\b", e), name
    assert seen == count, (src, seen)


# ---- the plans -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    lib = os.path.join(ROOT, "microflow_rs_amd", "libmicroflow_amd.so")
    if not os.path.exists(lib):
        pytest.skip("libmicroflow_amd.so not built")
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(_hipcc()))), "include")
    out = str(tmp_path_factory.mktemp("conv_entry_plan") / "conv_entry_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", rocm_inc, os.path.join(ROOT, "tests", "cpp", "conv_entry_plan.cpp"),
                           lib, "-Wl,-rpath," + os.path.dirname(lib), "-o", out])
    return out


def plan(exe, H, W, C, N, KH, KW, S, same):
    r = subprocess.run([exe] + [str(int(v)) for v in (H, W, C, N, KH, KW, S, same)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.split()
    return f[0], [int(v) for v in f[1:]]


# the stems of tests/test_gpu_f32_conv_entry.py that conv_rows_lds takes: (H, W, C, N, KH, KW, stride, SAME) -> images per step
ROWS = {(12, 12, 3, 16, 3, 3, 2, True): 8, (40, 40, 3, 8, 3, 3, 1, True): 6, (80, 80, 3, 16, 3, 3, 2, True): 1, (28, 28, 1, 6, 5, 5, 1, False): 8,
        (10, 10, 2, 12, 3, 3, 1, True): 8, (20, 12, 1, 12, 4, 3, 1, True): 8,
        (76, 76, 3, 12, 3, 3, 1, True): 1, (136, 128, 1, 12, 4, 3, 1, True): 1, (144, 128, 1, 6, 5, 5, 1, False): 1}
G1 = [s for s, g in ROWS.items() if g == 1]                                    # the ones whose first launch takes the floats


@pytest.mark.parametrize("shape", sorted(ROWS), ids=lambda v: "x".join(str(int(x)) for x in v))
def test_conv_rows_plan_gives_the_images_per_step_the_gpu_batches_are_ragged_against(plan_exe, shape):
    kind, f = plan(plan_exe, *shape)
    assert kind == "rows", (shape, kind)
    G, tile, lds = f
    assert G == ROWS[shape]
    H, W, C = shape[:3]
    assert G * H * (W * C // 4) <= 512 * 16 and lds <= 96 * 1024 and G * tile < lds      # 16 staged dwords per thread; the tiles fit
    assert (G == 1) == (4096 < H * (W * C // 4) <= 8192) and len(G1) == 4     # one image per step: more than half the staging slots
    # the batches are ragged against G: 77 for G > 1 (1 divides everything: there the step count matters)
    assert G == 1 or 77 % G != 0
    assert 2053 > 2 * 1024                                 # (the 80 x 80 x 3 model) more steps than twice the largest grid (4 x 256 workgroups)


# ... and those conv_gemm_rt takes -> (slices, banded?)
GEMM = {(16, 16, 3, 80, 3, 3, 1, True): (1, False), (10, 10, 2, 72, 3, 3, 1, True): (1, False), (16, 16, 4, 96, 3, 3, 1, True): (1, False),
        (128, 128, 3, 16, 3, 3, 2, True): (1, True), (128, 128, 3, 16, 3, 3, 1, True): (1, True), (8, 8, 4, 640, 7, 7, 1, True): (3, False)}


@pytest.mark.parametrize("shape", sorted(GEMM), ids=lambda v: "x".join(str(int(x)) for x in v))
def test_conv_gemm_plan_gives_the_slices_bands_and_row_bytes_of_the_gpu_cases(plan_exe, shape):
    kind, f = plan(plan_exe, *shape)
    assert kind == "gemm", (shape, kind)
    NSL, NBANDS, G, ROWB, lds = f
    assert (NSL, NBANDS > 1) == GEMM[shape]
    assert NBANDS == 1 or G == 1
    assert G == 1 or 77 % G != 0 or NSL > 1
    # both row paths of the staging are among the cases: LDS-DMA (whole 16-byte groups) and dword loads
    assert (ROWB % 16 == 0) == (shape[:3] in ((16, 16, 3), (16, 16, 4), (128, 128, 3), (8, 8, 4)))
