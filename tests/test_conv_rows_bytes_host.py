"""conv_rows_bytes (k_rt.hip) without a GPU: conv_rows_lds for one-channel images whose rows are not whole dwords.  The plan
(k::conv_rows_plan) takes those shapes with the BYTES flag and keeps the whole-dword ones as they were; the staging map
(conv_rows_bytes_map.hpp, the text the kernel runs) stages whole batches into a host copy of the tiles, byte for byte, with aligned
loads only and none wholly outside the batch -- once more under AddressSanitizer and UBSan; and the listing has the twelve instances
inside their launch bound, without scratch, with no barrier reached while LDS operations are pending.
(tests/cpp/conv_rows_bytes_plan.cpp linked against the built library.)"""
import importlib.util
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "microflow_rs_amd", "csrc")


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return hipcc


def _build(tmp, name, extra=()):
    lib = os.path.join(ROOT, "microflow_rs_amd", "libmicroflow_amd.so")
    if not os.path.exists(lib):
        pytest.skip("libmicroflow_amd.so not built")
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(_hipcc()))), "include")
    out = str(tmp / name)
    subprocess.check_call([cxx, "-std=c++17", "-O1", *extra, "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", rocm_inc,
                           os.path.join(ROOT, "tests", "cpp", "conv_rows_bytes_plan.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib), "-o", out])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("conv_rows_bytes_plan"), "conv_rows_bytes_plan")


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    """the same stand-alone program (host code only) with AddressSanitizer and UBSan, every finding fatal"""
    return _build(tmp_path_factory.mktemp("conv_rows_bytes_san"), "conv_rows_bytes_san",
                  ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MF_")}
    env.update(kw)
    return env


def plan(exe, H, W, C, N, KH, KW, sh, sw, same, **env):
    r = subprocess.run([exe, "plan"] + [str(int(v)) for v in (H, W, C, N, KH, KW, sh, sw, same)], capture_output=True, text=True, timeout=60,
                       env=_env(**env))
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.split()
    if f[0] == "none":
        return None
    return dict(zip(("G", "TILE", "lds", "BYTES", "step_bytes"), [int(v) for v in f[1:]]))


# (H, W, N, KH, KW, sh, sw, SAME) of the one-channel shapes the GPU tests run, and the batch each is staged at here (a ragged last step)
SHAPES = {"ds_cnn-stem": ((49, 10, 64, 10, 4, 2, 2, True), 9), "5x5": ((5, 5, 4, 3, 3, 1, 1, True), 11), "7x3": ((7, 3, 8, 3, 3, 1, 1, True), 9),
          "9x13-valid": ((9, 13, 12, 4, 13, 2, 1, False), 6), "67x63": ((67, 63, 5, 3, 3, 1, 1, True), 31),
          "131x129": ((131, 129, 8, 3, 3, 2, 2, True), 5)}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_plan_takes_rows_that_are_not_whole_dwords(exe, name):
    (H, W, N, KH, KW, sh, sw, same), batch = SHAPES[name]
    p = plan(exe, H, W, 1, N, KH, KW, sh, sw, same)
    assert p is not None and p["BYTES"] == 1, (name, p)
    rowd = -(-W // 4)
    G = p["G"]
    # sixteen staged elements per thread, one per tile dword of a row; the tiles fit; the packed element fits its fields
    assert 1 <= G <= 8 and G * H * rowd <= 512 * 16 and (G == 8 or (G + 1) * H * rowd > 512 * 16 or (G + 1) * p["TILE"] > 65536)
    assert G * p["TILE"] <= 65536 and p["lds"] <= 96 * 1024 and G * p["TILE"] < p["lds"]
    assert p["step_bytes"] == G * H * W < 32768
    assert batch % G != 0 or G == 1                                            # the batches staged below and on the GPU are ragged
    if name == "67x63":
        assert G < 8 and p["step_bytes"] % 2 == 1                              # step bases take all four byte shifts
    if name == "131x129":
        assert G == 1


def test_plan_refuses_what_the_route_does_not_take(exe):
    assert plan(exe, 6, 7, 3, 5, 3, 3, 1, 1, True) is None                     # rows that are not whole dwords with C >= 2
    assert plan(exe, 49, 10, 1, 80, 10, 4, 2, 2, True) is None                 # N > 64
    assert plan(exe, 49, 10, 1, 64, 3, 65, 1, 1, True) is None                 # a window row of more than 64 bytes
    assert plan(exe, 49, 10, 1, 64, 17, 4, 1, 1, True) is None                 # KH > 16
    assert plan(exe, 250, 133, 1, 8, 3, 3, 1, 1, True) is None                 # 250 x 34 tile dwords: more than the 8192 a step stages
    # MF_NO_CONV_ROWS_BYTES (with MF_DEV=1 only) gives the generic kernels back
    assert plan(exe, 49, 10, 1, 64, 10, 4, 2, 2, True, MF_DEV="1", MF_NO_CONV_ROWS_BYTES="1") is None
    assert plan(exe, 49, 10, 1, 64, 10, 4, 2, 2, True, MF_NO_CONV_ROWS_BYTES="1")["BYTES"] == 1
    assert plan(exe, 49, 12, 1, 64, 10, 4, 2, 2, True, MF_DEV="1", MF_NO_CONV_ROWS_BYTES="1")["BYTES"] == 0


@pytest.mark.parametrize("shape,G", [((12, 12, 3, 16, 3, 3, 2, 2, True), 8), ((40, 40, 3, 8, 3, 3, 1, 1, True), 6), ((136, 128, 1, 12, 4, 3, 1, 1, True), 1)])
def test_whole_dword_shapes_keep_their_plan(exe, shape, G):
    """(tests/test_f32_conv_entry_host.py ROWS pins their images per step)"""
    p = plan(exe, *shape)
    assert p is not None and p["BYTES"] == 0 and p["G"] == G, p


def _stage(exe, name):
    (H, W, N, KH, KW, sh, sw, same), batch = SHAPES[name]
    r = subprocess.run([exe, "stage"] + [str(int(v)) for v in (H, W, N, KH, KW, sh, sw, same, batch)], capture_output=True, text=True, timeout=120,
                       env=_env())
    assert r.returncode == 0, (name, r.stdout[-500:], r.stderr[-3000:])
    f = r.stdout.split()
    assert f[0] == "ok", r.stdout
    G, steps, shifts = int(f[1]), int(f[2]), int(f[3])
    assert steps == -(-batch // G)
    if name in ("5x5", "67x63", "131x129"):
        assert shifts == 15, (name, shifts)                                    # all four byte shifts occurred
    return shifts


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_staging_map_fills_the_tiles_byte_for_byte(exe, name):
    """extreme image bytes, a non-zero input zero point, sentinels in front of and behind the batch: every image byte in its place,
    the zero point everywhere else (the row tails included), no sentinel, no load wholly outside the batch -- the program checks"""
    _stage(exe, name)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_staging_map_under_address_and_ub_sanitizers(exe_sanitized, name):
    _stage(exe_sanitized, name)


# ---- three channels behind a PAD: conv_rows_plan_pads(..., bytes_any_c = true), what the PAD + convolution group routes here ----------
# (tests/pad_cases.py; the batch staged: whole steps and a ragged last one).  RGB rows that are not whole dwords put image bases -- 75
# and 243 bytes -- and with G = 7 images of 4185 bytes step bases too at every byte shift: the map's low2, its two-dword fetch and the
# alignbyte at shifts 1, 2, 3, which one-channel images of the same sizes reach only through W.
PADDED_C3 = {"conv3s2_5x5x3": 21, "conv3s2_45x31x3": 23, "conv3s1_9x9x3_p4": 13}


def _stage_pads(exe, name):
    from tests import pad_cases as P
    dw, H, W, C, K, S, (t, b, l, r), N, wz = P.SMALL[name]
    OH, OW = P.out_hw(P.SMALL[name])
    batch = PADDED_C3[name]
    assert not dw and C == 3 and (W * C) % 4 != 0 and (H * W * C) % 4 != 0
    res = subprocess.run([exe, "stage_pads"] + [str(int(v)) for v in (H, W, C, N, K, K, S, S, t, l, OH, OW, batch)], capture_output=True, text=True,
                         timeout=120, env=_env())
    assert res.returncode == 0, (name, res.stdout[-500:], res.stderr[-3000:])
    f = res.stdout.split()
    assert f[0] == "ok", res.stdout
    G, steps, shifts, bases = (int(v) for v in f[1:5])
    assert G == P.PINNED[name][1]["G"] and steps == -(-batch // G) and steps >= 2 and batch % G != 0
    assert shifts == 15, (name, shifts)                                        # all four byte shifts occurred
    if name == "conv3s2_45x31x3":
        assert bases == 15, bases                                              # ... and a step started at each of them
    return G


@pytest.mark.parametrize("name", sorted(PADDED_C3))
def test_staging_map_with_three_channels_and_explicit_pads(exe, name):
    """the claim conv_rows_plan_pads makes for bytes_any_c -- the staging is written in row bytes and has no C = 1 assumption -- byte
    for byte, with the image at the tile row and column the PAD's top and left put it"""
    _stage_pads(exe, name)


@pytest.mark.parametrize("name", sorted(PADDED_C3))
def test_three_channel_staging_under_address_and_ub_sanitizers(exe_sanitized, name):
    _stage_pads(exe_sanitized, name)


# ---- the listing ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def listing():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k_rt.s")
        # (the flags of tests/test_f32_conv_entry_host.py)
        subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mllvm",
                               "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "k_rt.hip")],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read().split("\n")


def test_twelve_instances_whose_barriers_wait_for_lds(listing):
    spec = importlib.util.spec_from_file_location("asm_barrier_waits", os.path.join(ROOT, "scripts", "asm_barrier_waits.py"))
    abw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(abw)
    mine = [(n, b) for n, b in abw.kernels(listing) if n.startswith("conv_rows_bytes<")]
    assert len(mine) == 12, [n for n, _ in mine]                               # {wzp, none} x modes 0, 1, 2 x {i8, u8}
    for name, body in mine:
        assert sum(1 for l in body if l.strip().startswith("s_barrier")) >= 2, name      # top of step | tiles staged
        assert not abw.scan(body), (name, abw.scan(body))
        assert any("v_alignbyte_b32" in l for l in body), name


def test_instances_use_no_scratch_and_fit_their_launch_bound(listing):
    """512 threads = two waves per SIMD; 128 registers each leave room for a second workgroup on the CU"""
    text = "\n".join(listing)
    meta = text[text.index("amdhsa.kernels:"):]
    meta = meta[:meta.index("\namdhsa.target:")]
    seen = 0
    for e in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s*(\S+)", e).group(1)
        if "conv_rows_bytes" not in name:
            continue
        seen += 1
        vgpr = int(re.search(r"\.vgpr_count:\s*(\d+)", e).group(1))
        agpr = re.search(r"\.agpr_count:\s*(\d+)", e)
        agpr = int(agpr.group(1)) if agpr else 0
        assert 0 < vgpr and vgpr + agpr <= 128, (name, vgpr, agpr)
        assert re.search(r"\.private_segment_fixed_size:\s*0\b", e), name
        assert re.search(r"\.vgpr_spill_count:\s*0\b", e), name
    assert seen == 12, seen
