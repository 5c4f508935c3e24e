"""k_dw_gemm.hip without a GPU: the generated code keeps the house rules (no barrier reached with LDS operations pending, M0
written only inside the LDS-DMA helper's asm, the int8 matrix instruction, no scratch, no scalar stores or atomics).  The host-side
plan and the routing are exercised through the library on the GPU (tests/test_gpu_dw_gemm.py), its operand A layout in
tests/test_wimage_host.py."""
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
        out = os.path.join(tmp, "k_dw_gemm.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mllvm",
                               "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "k_dw_gemm.hip")],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        yield open(out).read().split("\n")


def _abw():
    spec = importlib.util.spec_from_file_location("asm_barrier_waits", os.path.join(ROOT, "scripts", "asm_barrier_waits.py"))
    abw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(abw)
    return abw


def test_dw_gemm_barriers_wait_for_lds(listing):
    abw = _abw()
    kernels = list(abw.kernels(listing))
    # 4 operand-read forms (C % 16 == 0, C % 8 == 0, C % 4 == 0, other C) x filter zero points or not x 3 register-held k-step
    # counts (4, 7, 13) x 3 epilogue modes x 2 element types
    assert len(kernels) == 144, [n for n, _ in kernels]
    for name, body in kernels:
        assert name.startswith("dw_gemm_rt<"), name
        assert sum(1 for l in body if l.strip().startswith("s_barrier")) >= 2, name
        assert not abw.scan(body), (name, abw.scan(body))


def test_dw_gemm_reads_operand_b_at_its_natural_alignment(listing):
    """a _b64 / _b128 LDS read off its natural alignment is replayed (SQ_LDS_UNALIGNED_STALL): the C % 8 forms read two ds_read_b64
    (hipcc fuses them into a misaligned ds_read_b128 unless kept apart), the C % 4 and other forms dwords only"""
    kernels = list(_abw().kernels(listing))
    for name, body in kernels:
        al = int(name.split("<")[1].split(",")[0])
        reads = {l.split()[0] for l in body if l.strip().startswith("ds_read")}
        if al == 8:
            assert "ds_read_b128" not in reads and "ds_read_b64" in reads, (name, reads)
        elif al in (4, 1):
            assert not reads & {"ds_read_b128", "ds_read_b64", "ds_read2_b64", "ds_read_b96"}, (name, reads)


def test_dw_gemm_m0_only_inside_asm(listing):
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
    assert seen >= 144, seen


def test_dw_gemm_runs_on_the_matrix_pipe_without_scratch(listing):
    text = "\n".join(listing)
    assert "v_mfma_i32_16x16x64_i8" in text
    assert "global_load_lds_dwordx4" in text
    assert "v_alignbyte_b32" in text
    assert not re.search(r"^\s*scratch_", text, re.M)
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == 144 and set(sizes) == {"0"}, sizes
    assert not re.search(r"^\s*s_(buffer_|scratch_)?(store|atomic)", text, re.M)
