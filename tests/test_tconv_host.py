"""TRANSPOSE_CONV without a GPU.  The loader: the writer's models parse and report kind 67 with shapes, strides and padding, operand 2
is the running value, a file without a bias has c0 == +0, and every refusal answers with its status and reason.  (Before the operator
existed, loading these models failed with `unsupported operator: 67`.)  The phase weight images, Kc and tap tables of tconv_phase_rt
(wimage.cpp) multiplied on the CPU against the table's gather of a staged tile (tests/cpp/tconv_phase_dump.cpp, built under the address and undefined-behaviour sanitizers) give
the accumulators of the contract's numpy statement (tests/tconv_ref.py), which knows no phases."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import tconv_ref as T
from tests.conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import tflite_writer as tw  # noqa: E402

CSRC = os.path.join(ROOT, "microflow_rs_amd", "csrc")
Q = (0.05, -3)


def _tconv(rng=None, **kw):
    d = tw._tconv_layer(rng or np.random.default_rng(1), (4, 6, 8), Q, 12, 3, 2, **{k: kw.pop(k) for k in ("padding", "bias", "act") if k in kw})
    d.update(kw)
    return d


def _load(layers, elem=tw.INT8):
    import microflow_rs_amd as mf
    return mf.model(tw.build_model((1, 4, 6, 8), Q, layers, elem))


@pytest.mark.parametrize("padding,bias", [("same", True), ("valid", False)])
def test_a_transpose_conv_model_loads_and_reports_its_geometry(padding, bias):
    from microflow_rs_amd import _lib
    m = _load([_tconv(padding=padding, bias=bias, act="relu6"), tw._conv_layer(np.random.default_rng(2), (8, 12, 12) if padding == "same" else (9, 13, 12), (0.1, -128), False, 4, 3, 1)])
    a, b = m.ops
    oh, ow = (8, 12) if padding == "same" else (9, 13)
    assert _lib.MF_OP_TRANSPOSE_CONV == 67 and (a["kind"], a["name"], b["kind"]) == (67, "transpose_conv", 3)
    assert a["in_shape"] == (1, 4, 6, 8) and a["out_shape"] == (1, oh, ow, 12) and a["out_elems"] == oh * ow * 12   # operand 2 is the running value
    assert (a["KH"], a["KW"], a["sh"], a["sw"], a["pad"], a["act"]) == (3, 3, 2, 2, 0 if padding == "same" else 1, 3)
    assert (a["in_scale"], a["in_zp"]) == (np.float32(Q[0]), Q[1]) and b["in_shape"] == a["out_shape"]
    c0 = np.asarray(m.op_constants(0)[0])
    assert len(c0) == 12 and (bias or (np.all(c0 == 0) and not np.any(np.signbit(c0))))


def test_transpose_conv_refusals():
    from microflow_rs_amd import _lib
    U, I = _lib.MF_ERR_UNSUPPORTED, _lib.MF_ERR_INVALID_MODEL

    def refused(layer, status, *words):
        with pytest.raises(_lib.MicroflowError) as e:
            _load([layer])
        assert e.value.status == status, e.value
        for w in words:
            assert w in e.value.message, e.value.message
    refused(_tconv(shape_const=False), U, "unsupported operator: 67", "TRANSPOSE_CONV", "non-constant output_shape")
    refused(_tconv(shape=(1, 8, 11, 12)), I, "output_shape disagrees")
    refused(_tconv(out_shape=(1, 9, 12, 12)), I, "not what SAME gives")                      # ceil(9 / 2) != 4
    refused(_tconv(padding="valid", out_shape=(1, 8, 13, 12)), I, "not what VALID gives")    # (4 - 1) 2 + 3 == 9


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("tconv")
    exe = str(d / "tconv_phase_dump")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(CSRC, "wimage.cpp"),
                           os.path.join(ROOT, "tests", "cpp", "tconv_phase_dump.cpp"), "-o", exe])
    return exe, d


#                                   H  W  C   N   KH KW sh sw same NTS
@pytest.mark.parametrize("case", [(4, 4, 16, 16, 3, 3, 2, 2, True, 1),     # phases of 4 / 2 / 2 / 1 taps
                                  (5, 3, 16, 8, 4, 4, 2, 2, True, 1),      # padt = 1, bases beyond H - 1 and W - 1
                                  (3, 3, 16, 16, 2, 2, 3, 3, False, 1),    # phases with no tap
                                  (3, 4, 20, 40, 3, 3, 2, 2, False, 2)],   # C % 16 != 0, odd output, three tiles in slices of two
                         ids=lambda c: "x".join(map(str, c[:8])))
def test_phase_images_times_the_gathered_tile_are_the_accumulators(dump, case):
    exe, d = dump
    H, W, C, N, KH, KW, sh, sw, same, NTS = case
    OH, OW = T.out_hw(H, W, KH, KW, sh, sw, same)
    rng = np.random.default_rng(sum(case))
    x = rng.integers(-128, 128, (1, H, W, C)).astype(np.int8)
    w = rng.integers(-127, 128, (N, KH, KW, C)).astype(np.int8)
    izp = int(rng.integers(-128, 128))
    fin, fout = str(d / "in.bin"), str(d / "out.bin")
    with open(fin, "wb") as f:
        f.write(x.tobytes() + w.tobytes())
    args = [H, W, C, N, KH, KW, sh, sw, OH, OW, izp, NTS]
    out = subprocess.run([exe] + [str(a) for a in args] + [fin, fout], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stderr)
    got = np.fromfile(fout, np.int32).reshape(OH, OW, N)
    want = T.accumulators(x, w, izp, [0], (sh, sw), (OH, OW))[0]
    assert np.array_equal(got, want), int((got != want).sum())
