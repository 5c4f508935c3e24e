"""conv_stream_rt (k_conv_stream.hip) without a GPU: k::conv_stream_plan's classes (tests/cpp/conv_stream_plan.cpp against the built library),
the listing scans of tests/test_host_logic.py on the new file, and mf_op_kernel_name_at in the header, the binding table and the library."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT
from tests.test_pair_band_deep_host import CSRC, _exe, _hipcc, abw  # noqa: F401  (abw: the barrier-scan fixture)

INSTANCES = 12   # two tile sizes x epilogue modes 0, 1, 2 x {i8, u8}


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return _exe(tmp_path_factory, "conv_stream_plan")


def plan(exe, H, W, C, N, KH, KW, s=1, same=True, pads=None, dil=(1, 1), groups=1, dw=False, wz=False, finite=True):
    OH, OW = (-(-H // s), -(-W // s)) if same else ((H - KH) // s + 1, (W - KW) // s + 1)
    padt, padl = pads if pads else (((KH - 1) // 2, (KW - 1) // 2) if same else (0, 0))
    args = (H, W, C, N, KH, KW, s, s, OH, OW, padt, padl, dil[0], dil[1], groups, int(dw), int(wz), int(finite))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MF_")}
    r = subprocess.run([exe] + [str(v) for v in args], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.split()
    return None if f[0] == "none" else tuple(int(x) for x in f[1:])


# (H, W, C, N, K, stride, SAME): timed and tested shapes, K' > 8192, 7x7 and 5x5 filters
ACCEPTED = [(8, 8, 256, 512, 3, 2, True), (4, 4, 512, 512, 3, 1, True), (8, 8, 128, 128, 3, 1, True), (7, 7, 512, 1024, 1, 1, True),
            (8, 8, 256, 512, 1, 2, True), (2, 2, 1024, 1024, 3, 1, True), (4, 4, 128, 256, 3, 1, False), (9, 9, 256, 128, 7, 1, True),
            (6, 6, 512, 128, 5, 1, False)]


@pytest.mark.parametrize("H,W,C,N,K,s,same", ACCEPTED, ids=lambda v: str(v))
def test_conv_stream_plan_accepts_deep_convolutions(plan_exe, H, W, C, N, K, s, same):
    p = plan(plan_exe, H, W, C, N, K, K, s, same)
    assert p is not None
    assert p[0] == K * K * C                                           # no upper bound on K'
    assert 64 <= p[1] <= 65536                                         # a launch-time threshold the GPU test can reach
    assert p[2] == (256 if N % 256 == 0 and 256 * (N // 256) >= 192 else 128)


def test_conv_stream_plan_refuses_what_is_outside_its_class(plan_exe):
    ok = (4, 4, 128, 128, 3, 3)
    assert plan(plan_exe, *ok) is not None
    assert plan(plan_exe, *ok, pads=(2, 0), same=False) is not None    # explicit top / left pads
    assert plan(plan_exe, 4, 4, 64, 128, 3, 3) is None and plan(plan_exe, 4, 4, 192, 128, 3, 3) is None   # C % 128
    assert plan(plan_exe, 4, 4, 128, 130, 3, 3) is None and plan(plan_exe, 4, 4, 128, 64, 3, 3) is None   # N % 128
    assert plan(plan_exe, *ok, wz=True) is None                        # filter zero points: conv_gemm_rt<wzp>
    assert plan(plan_exe, *ok, finite=False) is None                   # NaN constants: conv2d_generic
    assert plan(plan_exe, *ok, dw=True) is None and plan(plan_exe, *ok, groups=2) is None
    assert plan(plan_exe, *ok, dil=(2, 2)) is None and plan(plan_exe, *ok, dil=(1, 2)) is None and plan(plan_exe, *ok, pads=(-1, 0)) is None


def test_conv_stream_listing_keeps_the_house_rules(abw):
    from microflow_rs_amd import build as B                             # the shipped object's flags (NO_PACKED_FP32 included)
    assert "k_conv_stream.hip" in B.SOURCES and "k_conv_stream.hip" in B.NO_PACKED_FP32
    with __import__("tempfile").TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k_conv_stream.s")
        subprocess.check_call([_hipcc(), "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"] + [f for f in B.FLAGS if f not in ("-fPIC", "-Wall")] +
                              ["--cuda-device-only", "-S", "-x", "hip", "-o", out, os.path.join(CSRC, "k_conv_stream.hip")],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        lines = open(out).read().split("\n")
    kernels = list(abw.kernels(lines))
    assert len(kernels) == INSTANCES and all(n.startswith("conv_stream_rt<") for n, _ in kernels), [n for n, _ in kernels]
    for name, body in kernels:
        assert any(l.strip().startswith("s_barrier") for l in body) and not abw.scan(body), (name, abw.scan(body))
        assert any("v_mfma_i32_32x32x32_i8" in l for l in body) and any("global_load_lds_dwordx4" in l for l in body), name
    in_asm = False
    for l in lines:                                                    # M0: inside the DMA helper's asm statement only
        s = l.strip()
        in_asm = s.startswith(";;#ASMSTART") or (in_asm and not s.startswith(";;#ASMEND"))
        assert in_asm or not (l.startswith("\t") and re.search(r"\bm0\b", s.split(";")[0])), s
    text = "\n".join(lines)
    assert set(re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)) == {"0"}
    nf = [int(v) for v in re.findall(r"\.amdhsa_next_free_vgpr\s+(\d+)", text)]
    assert len(nf) == INSTANCES and max(nf) <= 256, nf                  # two waves per SIMD


def test_kernel_name_at_is_declared_bound_and_exported():
    from microflow_rs_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "microflow_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mf_op_kernel_name_at\s*\(\s*const mf_op \*op,\s*size_t batch,\s*char \*buf,\s*size_t len\s*\)", header)
    res, args = _lib.SIGNATURES["mf_op_kernel_name_at"]
    assert res is ctypes.c_int and [a for a in args[1:]] == [ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "mf_op_kernel_name_at")
    assert _lib.lib().mf_op_kernel_name_at(None, 1, ctypes.create_string_buffer(8), 8) == _lib.MF_ERR_INVALID_ARG
