"""k_fc_rt.hip without a GPU: the generated code keeps the house rules (no barrier reached with LDS operations pending, M0
written only inside the LDS-DMA helper's asm, the int8 matrix instruction, no scratch).  The host-side plan and weight image are
exercised through the library on the GPU (tests/test_gpu_fc_rt.py: parity over the shape grid, the K limit, guard bytes)."""
import importlib.util
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "microflow_rs_amd", "csrc")


@pytest.fixture(scope="module")
def listing():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k_fc_rt.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mllvm",
                               "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "k_fc_rt.hip")],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        yield open(out).read().split("\n")


def test_fc_rt_barriers_wait_for_lds(listing):
    spec = importlib.util.spec_from_file_location("asm_barrier_waits", os.path.join(ROOT, "scripts", "asm_barrier_waits.py"))
    abw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(abw)
    kernels = list(abw.kernels(listing))
    # fc_rt: 2 operand-read forms x 3 epilogue modes x 2 element types; fc_chain: 3 epilogue modes x 2 element types
    assert len(kernels) == 18, [n for n, _ in kernels]
    for name, body in kernels:
        assert name.startswith("fc_rt<") or name.startswith("fc_chain<"), name
        assert sum(1 for l in body if l.strip().startswith("s_barrier")) >= 2, name
        assert not abw.scan(body), (name, abw.scan(body))


def test_fc_rt_m0_only_inside_asm(listing):
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
    assert seen >= 18, seen


def test_fc_rt_runs_on_the_matrix_pipe_without_scratch(listing):
    text = "\n".join(listing)
    assert "v_mfma_i32_16x16x64_i8" in text
    assert "global_load_lds_dwordx4" in text
    assert not re.search(r"^\s*scratch_", text, re.M)
    for m in re.finditer(r"\.private_segment_fixed_size:\s*(\d+)", text):
        assert m.group(1) == "0"
    assert not re.search(r"^\s*s_(buffer_|scratch_)?(store|atomic)", text, re.M)
