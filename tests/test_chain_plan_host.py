"""The forced chain plan's text form (MF_CHAIN_PLAN, microflow_rs_amd/csrc/switches.cpp: chain_plan_parse) without a GPU:
tests/cpp/chain_plan_parse.cpp, compiled with the host compiler under the address and undefined-behaviour sanitizers.  A malformed
string must be refused (mf_model_prepare then answers MF_ERR_INVALID_ARG) and never be read as some other plan: the plan sweep
(tests/test_gpu_chain_plans.py) relies on "what I wrote is what ran"."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "microflow_rs_amd", "csrc")

GOOD = ["1:0:-1", "4:0:-1", "1:3:1,3:12:-1", "1:8:0,2:0:-1,1:128:1", "2:6:-1,0:0:-1,1:0:-1", "16:128:-1",
        "1:1:0,1:1:1,1:2:0,1:2:1", "0:0:-1"]
BAD = ["", ",", "1", "1:2", "1:2:", "1:2:0,", ",1:2:0", "1:2:0,,1:2:0", "1:2:0:1", "1:2:0;1:2:0", " 1:2:0", "1:2:0 ", "1: 2:0", "1:+2:0",
       "1:0x10:0", "1:2.0:0", "a:2:0", "1:2:x", "-1:2:0", "17:0:-1", "1:129:0", "1:-2:0", "1:2:2", "1:2:-2", "1:2:--1", "1:99999999999999999999:0",
       "0:4:-1", "0:0:0", "2:8:1", "3:0:0", "1:2:0\n", "len:G:dbuf"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("chain_plan") / "chain_plan_parse")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(CSRC, "switches.cpp"), os.path.join(ROOT, "tests", "cpp", "chain_plan_parse.cpp"), "-o", out])
    return out


def run(exe, args, **env_extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MF_")}
    env.update(env_extra)
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split("\n")[:-1]


def test_well_formed_plans_parse_to_themselves(exe):
    lines = run(exe, GOOD)
    assert lines[:-1] == ["ok " + g for g in GOOD]
    assert lines[-1] == "env unset"


def test_malformed_plans_are_refused_with_a_reason(exe):
    lines = run(exe, BAD)
    assert len(lines) == len(BAD) + 1
    for text, line in zip(BAD, lines):
        assert line.startswith("bad ") and len(line) > 8, (text, line)


def test_the_environment_counts_only_with_the_master_switch(exe):
    assert run(exe, [], MF_CHAIN_PLAN="1:3:1,3:12:-1") == ["env unset"]                      # (no MF_DEV=1: ignored like every routing switch)
    assert run(exe, [], MF_DEV="1") == ["env unset"]
    assert run(exe, [], MF_DEV="1", MF_CHAIN_PLAN="1:3:1,3:12:-1") == ["env ok 1:3:1,3:12:-1"]
    assert run(exe, [], MF_DEV="1", MF_CHAIN_PLAN="1:3")[0].startswith("env bad ")
    assert run(exe, [], MF_DEV="1", MF_CHAIN_PLAN="")[0].startswith("env bad ")              # (set but empty is not "unset")
