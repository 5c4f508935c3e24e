"""Grouped Conv2D without a GPU: the loader reads G from the shapes, reports it and refuses what divides nothing; the planner's facts."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import tflite_writer as tw  # noqa: E402

Q = (0.05, -3)


def _load(layers, shape=(1, 6, 6, 16)):
    return __import__("microflow_rs_amd").model(tw.build_model(shape, Q, layers))


def test_resnext_parses_and_reports_its_groups():
    import microflow_rs_amd as mf
    in_shape, in_q, layers = tw.resnext_layers(np.random.default_rng(25))
    m = mf.model(tw.build_model(in_shape, in_q, layers))
    assert m.num_ops == len(layers)
    for i, L in enumerate(layers):
        if L["op"] == "conv_2d":
            C = m.op(i)["in_shape"][3]
            assert m.op(i)["groups"] == m.op_groups(i) == C // np.asarray(L["filters"]).shape[3], i
        else:
            assert m.op(i)["groups"] == 1
            with pytest.raises(mf._lib.MicroflowError):
                m.op_groups(i)
    assert sorted(m.op(i)["groups"] for i in range(m.num_ops))[-2:] == [4, 4] and m.op(0)["groups"] == 1


@pytest.mark.parametrize("filt_c,n,words", [(5, 16, ("channel mismatch",)), (4, 18, ("4 groups", "18 output"))], ids=["C-not-divided", "N-not-divided"])
def test_refusals(filt_c, n, words):
    from microflow_rs_amd import _lib
    L = tw._conv_layer(np.random.default_rng(1), (6, 6, 16), Q, False, n, 3, 1)
    L["filters"] = np.asarray(L["filters"])[:, :, :, :filt_c]
    with pytest.raises(_lib.MicroflowError) as e:
        _load([L])
    assert e.value.status == _lib.MF_ERR_INVALID_MODEL, e.value
    for w in words:
        assert w in e.value.message, e.value.message


#                                   H  W  C    N    G  K  S same wz    GPT TPG SPAN KS PW NT NSL
@pytest.mark.parametrize("case", [(7, 7, 16,  16,  4, 3, 1, 1, 0,   4, 0, 16,  3,  3,  1,  1),     # g1: four groups in one tile, 9 taps x 16 B = 144 -> 3 k steps
                                  (7, 7, 16,  16,  4, 3, 1, 1, 1,   4, 0, 16,  3,  6,  1,  1),     # ... with filter zero points: the pieces of ones behind the weights
                                  (6, 6, 8,   40,  2, 3, 1, 1, 0,   0, 2, 4,   1,  1,  4,  1),     # g5: Ng = 20, two tiles per group, K = 36
                                  (4, 4, 256, 256, 2, 3, 1, 1, 0,   0, 8, 128, 18, 18, 16, 6),     # g9: 288 KiB of weights: 6 slices of 3 tiles (54 KiB) leave room for a 4-row tile under 80 KiB
                                  (7, 7, 18,  12,  3, 3, 1, 1, 0)], ids=lambda c: "x".join(map(str, c[:9])))   # g10: Cg = 6 is outside the class
def test_planner_facts(case, tmp_path):
    """conv_grp_plan's tile layout, K steps, image pieces and N slices as worked out by hand (tests/cpp/conv_grp_plan.cpp)"""
    from tests.test_f32_conv_entry_host import CSRC, _hipcc
    lib, exe = os.path.join(ROOT, "microflow_rs_amd", "libmicroflow_amd.so"), str(tmp_path / "plan")
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(_hipcc()))), "include")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", inc, os.path.join(ROOT, "tests", "cpp", "conv_grp_plan.cpp"), lib,
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    out = subprocess.run([exe] + [str(v) for v in case[:9]], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.split() == ([str(v) for v in case[9:]] or ["none"]), out.stdout + out.stderr
