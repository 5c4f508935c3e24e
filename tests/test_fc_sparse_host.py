"""k_fc_sparse.hip without a GPU: the generated code keeps the house rules (no barrier reached with LDS operations pending, M0
written only inside the LDS-DMA helper's asm, the sparse int8 matrix instruction, no scratch, no scalar stores or atomics).  The
weight image and the routing are exercised through the library on the GPU (tests/test_gpu_fc_sparse.py)."""
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
        out = os.path.join(tmp, "k_fc_sparse.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mllvm",
                               "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "k_fc_sparse.hip")],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        yield open(out).read().split("\n")


def _abw():
    spec = importlib.util.spec_from_file_location("asm_barrier_waits", os.path.join(ROOT, "scripts", "asm_barrier_waits.py"))
    abw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(abw)
    return abw


def test_fc_sparse_barriers_wait_for_lds(listing):
    abw = _abw()
    kernels = list(abw.kernels(listing))
    # 256 x 256 tiles with 8 waves, 128 x 128 with 4
    assert sorted(n for n, _ in kernels) == ["fc_sparse24<128, 128, 2, 2>", "fc_sparse24<256, 256, 2, 4>"], [n for n, _ in kernels]
    for name, body in kernels:
        assert sum(1 for l in body if l.strip().startswith("s_barrier")) >= 1, name
        assert not abw.scan(body), (name, abw.scan(body))


def test_fc_sparse_m0_only_inside_asm(listing):
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
    assert seen >= 2, seen


def test_fc_sparse_runs_on_the_sparse_matrix_pipe_without_scratch(listing):
    text = "\n".join(listing)
    assert re.search(r"^\s*v_smfmac_i32_16x16x128_i8\b", text, re.M)
    assert not re.search(r"^\s*v_mfma_", text, re.M)     # sparse instructions only: no dense / sparse pair on one accumulator
    assert "global_load_lds_dwordx4" in text
    assert not re.search(r"^\s*scratch_", text, re.M)
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == 2 and set(sizes) == {"0"}, sizes
    assert not re.search(r"^\s*s_(buffer_|scratch_)?(store|atomic)", text, re.M)
