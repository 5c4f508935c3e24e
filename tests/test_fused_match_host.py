"""The fused units' one pair test (fused_impl.hpp: match_dw3x3_pw1x1) without a GPU, through tests/cpp/pair_match.cpp: a stand-alone
program with its own main, built with the address and undefined-behaviour sanitizers on the host side, that fills two operators by
hand and prints the verdicts.  Expected verdicts: a condition that chain_pair_ok, pair_band_create, pair_wz_create,
fused_pair_tail_create and fused_front_pair_tail_create ALL applied before they shared the matcher must refuse; a condition only
some of them apply (the members' own kernels, force_generic, the width rules) must not -- it stays with its callers."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "microflow_rs_amd", "csrc")

ACCEPTED = {"stride1": "{6, 6, 16, 1, 6, 6, 16, izp4}", "stride2": "{6, 6, 16, 2, 3, 3, 32, izp4}"}
REFUSED = ["filter5x5", "valid", "sh_ne_sw", "stride3", "multiplier2", "second3x3", "second_stride2", "second_H", "second_C", "element_type",
           "device", "dw_not_finite", "pw_not_finite"]
LEFT_TO_THE_CALLERS = {"other_kernels": 0, "force_generic": 1, "odd_width_stride2": 1}  # accepted; f = the depthwise is on dw3x3_rt / a table kernel


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("pair_match") / "pair_match")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-x", "hip", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "pair_match.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    by = {}
    for l in out.stdout.splitlines():
        name, rest = l.split(" ", 1)
        by[name] = rest
    return by


def test_every_case_ran(verdicts):
    assert sorted(verdicts) == sorted(list(ACCEPTED) + REFUSED + list(LEFT_TO_THE_CALLERS))


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_accepts_the_pair_with_its_geometry(verdicts, case):
    assert verdicts[case] == "ok " + ACCEPTED[case] + " f=1"


@pytest.mark.parametrize("case", REFUSED)
def test_refuses_what_every_caller_refused(verdicts, case):
    assert verdicts[case] == "no"


@pytest.mark.parametrize("case", sorted(LEFT_TO_THE_CALLERS))
def test_leaves_the_callers_their_own_conditions(verdicts, case):
    assert verdicts[case].startswith("ok ") and verdicts[case].endswith(" f=%d" % LEFT_TO_THE_CALLERS[case])
