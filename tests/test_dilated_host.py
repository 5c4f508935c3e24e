"""Dilation factors without a GPU.  The loader reads Conv2DOptions fields 4 / 5 and DepthwiseConv2DOptions fields 5 / 6 (before, they
were never read and such a layer ran as a dilation-1 convolution), defaults them to 1, refuses factors <= 0 and a declared output
shape the contract does not give."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import tflite_writer as tw  # noqa: E402

Q = (0.05, -3)


def _layer(dw=False, **kw):
    d = tw._conv_layer(np.random.default_rng(1), (6, 20, 8), Q, dw, 12, 3, 1, kw.pop("padding", "valid"), dilation=kw.pop("dilation", (1, 4)))
    d.update(kw)
    return d


def _load(layers):
    return __import__("microflow_rs_amd").model(tw.build_model((1, 6, 20, 8), Q, layers))


@pytest.mark.parametrize("dw", [False, True], ids=["conv", "depthwise"])
def test_the_factors_are_read_and_default_to_one(dw):
    m = _load([_layer(dw), tw._conv_layer(np.random.default_rng(2), (4, 12, 8 if dw else 12), (0.1, -128), dw, 4, 3, 1)])
    assert m.op(0)["out_shape"] == (1, 4, 12, 8 if dw else 12)          # VALID: 6 - 2, 20 - 2 * 4
    assert m.op_dilation(0) == (1, 4) and m.op_dilation(1) == (1, 1)
    same = _load([_layer(dw, padding="same", dilation=(2, 3))])
    assert same.op(0)["out_shape"][1:3] == (6, 20) and same.op_dilation(0) == (2, 3)


def test_refusals():
    from microflow_rs_amd import _lib

    def refused(layer, *words):
        with pytest.raises(_lib.MicroflowError) as e:
            _load([layer])
        assert e.value.status == _lib.MF_ERR_INVALID_MODEL, e.value
        for w in words:
            assert w in e.value.message, e.value.message
    refused(_layer(dilation=(0, 4)), "Conv2D", "0x4", "not positive")
    refused(_layer(True, dilation=(1, -1)), "DepthwiseConv2D", "1x-1")
    refused(_layer(out_shape=(1, 4, 18, 12)), "Conv2D with dilation 1x4", "VALID gives (4 x 12)")     # the dilation-1 size
    refused(_layer(True, padding="same", out_shape=(1, 6, 19, 8)), "DepthwiseConv2D with dilation 1x4", "SAME")
    with pytest.raises(_lib.MicroflowError):
        _load([tw._fc_layer(np.random.default_rng(1), 960, 4, Q)]).op_dilation(0)                   # neither convolution


#                                   W   C   KW sw dw OW padl   PL PP
@pytest.mark.parametrize("case", [(7,  16, 3, 1, 2, 7,  2,    6, 96),     # SAME 3x3 at 2: two planes, halo both sides
                                  (11, 4,  3, 1, 3, 5,  0,    4, 16),     # VALID, W no multiple of dw: planes of 4, 4 and 3 columns
                                  (5,  16, 3, 1, 1, 5,  1,    7, 112),    # one plane: the image's first byte on a 16-byte boundary
                                  (20, 8,  3, 1, 4, 12, 0,    5, 48),     # the TCN layer
                                  (24, 8,  3, 1, 4, 24, 8,    8, 64),     # ... behind its causal pad
                                  (8,  16, 3, 2, 3, 4,  3,    5, 80)],    # stride 2: windows start in every phase
                         ids=lambda c: "x".join(map(str, c[:7])))
def test_plane_tile_facts(case, tmp_path):
    """wimage.cpp's plane geometry staged and gathered on the CPU (tests/cpp/conv_dil_tile_dump.cpp, under the sanitizers): every tap is
    its input column or the halo, every read aligned and inside the row; plane length and pitch as worked out by hand.  (Bands, slices
    and the LDS budget are conv_dil_plan's: tests/test_gpu_dilated.py.)"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    exe = str(tmp_path / "dump")
    csrc = os.path.join(ROOT, "microflow_rs_amd", "csrc", "wimage.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", csrc,
                           os.path.join(ROOT, "tests", "cpp", "conv_dil_tile_dump.cpp"), "-o", exe])
    out = subprocess.run([exe] + [str(a) for a in case[:7]], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stderr)
    PL, PP, LP, ROW = map(int, out.stdout.split())
    dw, C, padl = case[4], case[1], case[6]
    assert (PL, PP) == case[7:], (PL, PP)
    assert ROW % 16 == 0 and LP + dw * PP + 16 <= ROW <= LP + dw * PP + 48, (LP, ROW)   # (the planes, the over-read room, the bank offset; no more)
    assert (LP + padl * C) % 16 == 0 and LP < 16 if dw == 1 else LP == 0, LP
