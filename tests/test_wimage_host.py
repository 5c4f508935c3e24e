"""The host-built weight layouts (microflow_rs_amd/csrc/wimage.cpp) without a GPU: tests/cpp/wimage_dump.cpp, compiled with the
host compiler under the address and undefined-behaviour sanitizers, prints `name shape bytes fnv1a64` for every layout at the
smallest shapes that reach each branch of its index arithmetic; the lines must equal tests/golden/wimage_layouts.txt, which was
recorded right after the builders moved out of ops.hip unchanged (so the bytes are those of the layouts the kernels were tested
with).  `pw_rr K8,N8` was recorded later: before, that shape read past the weights."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "microflow_rs_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "wimage_layouts.txt")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("wimage") / "wimage_dump")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(CSRC, "wimage.cpp"),
                           os.path.join(ROOT, "tests", "cpp", "wimage_dump.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def test_layouts_match_the_recorded_bytes(lines):
    golden = open(GOLDEN).read().splitlines()
    assert len(golden) == 57
    assert lines == golden


def test_ones_tile_is_the_tail_of_pw_rt_with_ones(lines):
    """both users of the shared ones tile (pw_rt's and conv_mm_rt's <wzp> images) get what build_pw_rt_weights(ones) appended"""
    by = {}
    for l in lines:
        name, shape, size, h = l.split()
        by[(name, shape)] = (size, h)
    shapes = [s for (n, s) in by if n == "ones_tile"]
    assert sorted(shapes) == ["K144,KS3", "K80,KS2"]
    for s in shapes:
        assert by[("ones_tile", s)] == by[("pw_rt_tail", s)]
