"""mf_model_device_ops, the diagnostic behind the launch counts of tests/test_gpu_f32_boundary.py: present in the library, the
header and the binding table, and 0 for a model that has enqueued nothing.  No GPU needed."""
import ctypes as C
import os
import re

from tests.conftest import ROOT, model_path


def test_device_ops_is_exported_declared_and_bound():
    from microflow_rs_amd import _lib
    fn = getattr(_lib.lib(), "mf_model_device_ops")            # (AttributeError: the library does not export it)
    assert fn.restype is C.c_ulonglong
    assert _lib.SIGNATURES["mf_model_device_ops"][0] is C.c_ulonglong and len(_lib.SIGNATURES["mf_model_device_ops"][1]) == 1
    header = open(os.path.join(ROOT, "include", "microflow_amd.h")).read()
    assert re.search(r"unsigned long long\s+mf_model_device_ops\(const mf_model \*model\);", header)
    assert "#define MF_ABI_VERSION 3" in header or re.search(r"MF_ABI_VERSION\s*=?\s*3\b", header)
    rust = open(os.path.join(ROOT, "rust", "microflow-amd", "src", "lib.rs")).read()
    assert "fn mf_model_device_ops(model: *const mf_model)" in rust


def test_unprepared_model_has_enqueued_nothing():
    import microflow_rs_amd as mf
    m = mf.Model(model_path("sine"))
    assert m.device_ops() == 0
    from microflow_rs_amd import _lib
    assert _lib.lib().mf_model_device_ops(None) == 0           # (a null handle is answered, not dereferenced)


def test_the_dev_switch_is_parsed_documented_and_in_the_matrix():
    csrc = os.path.join(ROOT, "microflow_rs_amd", "csrc")
    assert '"MF_NO_F32_BOUNDARY"' in open(os.path.join(csrc, "switches.cpp")).read()
    assert re.search(r"//\s+MF_NO_F32_BOUNDARY\b", open(os.path.join(csrc, "mf_switches.hpp")).read())
    assert "MF_NO_F32_BOUNDARY=1" in open(os.path.join(ROOT, "scripts", "switch_matrix.sh")).read()


def test_first_and_last_launch_kernels_have_f32_instances_without_scratch():
    """k_dwfc.hip (dwc1_fc_softmax_f32: 3 epilogue modes x 2 element types x with / without weight zero point x 3 boundaries), k_tail3.hip
    (pair3_tail_f32: one per pair3_tail / pair_front_tail instance) and k_rt.hip (dw3x3_stem_rt_f32: 2 widths x 3 modes x 2 element types):
    the instances exist beside the int8 ones, whose count did not change, and none uses scratch"""
    import shutil
    import subprocess
    import tempfile
    import pytest
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "microflow_rs_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        procs = [subprocess.Popen([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mllvm", "-amdgpu-mfma-vgpr-form=1",
                                   "--cuda-device-only", "-S", "-o", os.path.join(tmp, f + ".s"), os.path.join(csrc, f + ".hip")],
                                  stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) for f in ("k_dwfc", "k_tail3", "k_rt")]
        assert all(p.wait() == 0 for p in procs)
        text = {f: open(os.path.join(tmp, f + ".s")).read() for f in ("k_dwfc", "k_tail3", "k_rt")}
    def kernels(t, prefix):
        return [m for m in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", t, re.M) if re.match(r"_ZN2mf1k\d+" + prefix + "I", m)]
    for f, name, n_int8, n_f32 in (("k_dwfc", "dwc1_fc_softmax", 12, 36), ("k_tail3", "pair3_tail", 28, 28), ("k_rt", "dw3x3_stem_rt", 12, 12)):
        assert len(kernels(text[f], name)) == n_int8, (name, len(kernels(text[f], name)))
        assert len(kernels(text[f], name + "_f32")) == n_f32, (name, len(kernels(text[f], name + "_f32")))
        sizes = set(re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text[f]))
        assert sizes == {"0"}, (f, sizes)


def test_f32_instances_keep_the_house_rules():
    """k_fc_f32.hip's generated code: 36 fc_rt_f32 (2 operand-read forms x 3 epilogue modes x 2 element types x 3 boundaries), 18
    fc_chain_f32 and 6 pool_fc_chain_f32 kernels, no barrier reached with LDS operations pending (every barrier is wg_sync's), M0
    only inside the LDS-DMA helper's asm, no scratch, and 16-byte loads of the floats"""
    import importlib.util
    import shutil
    import subprocess
    import tempfile
    import pytest
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k_fc_f32.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mllvm",
                               "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-S", "-o", out,
                               os.path.join(ROOT, "microflow_rs_amd", "csrc", "k_fc_f32.hip")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        listing = open(out).read().split("\n")
    spec = importlib.util.spec_from_file_location("asm_barrier_waits", os.path.join(ROOT, "scripts", "asm_barrier_waits.py"))
    abw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(abw)
    kernels = list(abw.kernels(listing))
    count = {p: sum(1 for n, _ in kernels if n.startswith(p + "<")) for p in ("fc_rt_f32", "fc_chain_f32", "pool_fc_chain_f32")}
    assert count == {"fc_rt_f32": 36, "fc_chain_f32": 18, "pool_fc_chain_f32": 6} and len(kernels) == 60, (count, len(kernels))
    for name, body in kernels:
        assert sum(1 for l in body if l.strip().startswith("s_barrier")) >= 2, name
        assert not abw.scan(body), (name, abw.scan(body))
    text = "\n".join(listing)
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == 60 and set(sizes) == {"0"}, sizes
    assert not re.search(r"^\s*scratch_", text, re.M)
    assert "global_load_dwordx4" in text and "v_mfma_i32_16x16x64_i8" in text
    in_asm = False
    for n, l in enumerate(listing):
        s = l.strip()
        if s.startswith(";;#ASMSTART"):
            in_asm = True
        elif s.startswith(";;#ASMEND"):
            in_asm = False
        elif l.startswith("\t") and re.search(r"\bm0\b", s.split(";")[0]):
            assert in_asm, (n, s)
