"""tflite_writer.tcn end to end against its TWIN: every dilated layer rewritten as the undilated VALID convolution with the zero-stuffed
filter, the stuffed taps holding the filter zero point ((w - wzp) is 0 there: the contract's accumulator), run through the CPU oracle
and the numpy PAD / ADD (tests/pad_ref.segments).  Dilated layers are pad+conv_dil_rt launches; MF_NO_CONV_DIL gives the same bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dilated_ref as D
from tests import pad_ref as P
from tests.conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import tflite_writer as tw  # noqa: E402

pytestmark = pytest.mark.gpu
T_, C_, F_ = 40, 8, 16


@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
def test_tcn_runs_as_the_composed_operators(u8, tmp_path):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import microflow_rs_amd as mf
    from oracle import oracle as O
    elem, dt = (tw.UINT8, np.uint8) if u8 else (tw.INT8, np.int8)
    in_shape, in_q, layers = tw.tcn_layers(np.random.default_rng(24), T_, C_, F_, elem=elem)
    blob = tw.build_model(in_shape, in_q, layers, elem)
    m = mf.model(blob)
    xq = (np.random.default_rng(5).integers(-128, 128, (7, 1, T_, C_)) + (128 if u8 else 0)).astype(dt)
    want = P.segments(tw, O, in_shape, in_q, D.twin(layers), elem)(xq)[-1]
    got = m.run_quantized(xq).reshape(7, -1)
    assert np.array_equal(got, want), int((got != want).sum())
    names = [m.op(i)["kernel"] for i in (4, 7, 10)]   # d = 2: the stuffed filter (under 3x the taps); then the generic kernel, in a process of its own
    assert names[0].startswith("pad+") and names[0].endswith("[d1x2]") and names[1:] == ["pad+conv_dil_rt<d1x4>", "pad+conv_dil_rt<d1x8>"], names
    path, xpath, ypath = (str(tmp_path / n) for n in ("tcn.tflite", "x.npy", "y.npy"))
    open(path, "wb").write(blob)
    np.save(xpath, xq)
    code = ("import sys, numpy as np, microflow_rs_amd as mf\n"
            "m = mf.model(open(sys.argv[1], 'rb').read()); y = m.run_quantized(np.load(sys.argv[2]))\n"
            "assert not any('conv_dil' in m.op(i)['kernel'] or '[d' in m.op(i)['kernel'] for i in range(m.num_ops)); np.save(sys.argv[3], y)\n")
    subprocess.run([sys.executable, "-c", code, path, xpath, ypath], check=True, timeout=300, cwd=ROOT, env=dict(os.environ, MF_DEV="1", MF_NO_CONV_DIL="1"))
    assert np.array_equal(np.load(ypath).reshape(7, -1), want)


@pytest.mark.parametrize("kind", ["pair", "conv1_fc", "conv_pool", "stuffed_pair"])
def test_the_fused_matchers_pass_a_dilated_operator_by(kind):
    """A depthwise 3x3 + 1x1 pair, a one-channel convolution + FullyConnected and a convolution + pool, each a fused group when
    undilated, with factors 3 x 3 (no stuffed filter): the dilated operator launches alone and the model gives its twin's bytes.
    stuffed_pair: a 2x2 depthwise at 2 x 2 IS the undilated 3x3 SAME depthwise and may pair: whatever launches, the twin's bytes."""
    import microflow_rs_amd as mf
    from oracle import oracle as O
    rng, q = np.random.default_rng(9), (0.05, -3)
    if kind in ("pair", "stuffed_pair"):
        shape, first = (12, 12, 16), tw._conv_layer(rng, (12, 12, 16), q, True, 16, 3 if kind == "pair" else 2, 1, dilation=(3, 3) if kind == "pair" else (2, 2))
        rest = [tw._conv_layer(rng, (12, 12, 16), first["out_q"], False, 32, 1, 1)]
    elif kind == "conv1_fc":
        shape, first = (12, 12, 1), tw._conv_layer(rng, (12, 12, 1), q, False, 8, 3, 1, dilation=(3, 3))
        rest = [dict(op="reshape", out_shape=(1, 1152), out_q=first["out_q"]), tw._fc_layer(rng, 1152, 4, first["out_q"])]
    else:
        shape, first = (12, 12, 16), tw._conv_layer(rng, (12, 12, 16), q, False, 16, 3, 1, dilation=(3, 3))
        rest = [dict(op="average_pool_2d", filter=(2, 2), padding="valid", strides=(2, 2), act="none", out_shape=(1, 6, 6, 16), out_q=first["out_q"])]
    layers, in_shape = [first] + rest, (1,) + shape
    m = mf.model(tw.build_model(in_shape, q, layers))
    xq = rng.integers(-128, 128, (3,) + shape).astype(np.int8)
    want = P.segments(tw, O, in_shape, q, D.twin(layers), tw.INT8)(xq)[-1]
    assert np.array_equal(m.run_quantized(xq).reshape(3, -1), want)
    if kind == "stuffed_pair":
        return
    assert "d3x3" in m.op(0)["kernel"] or m.op(0)["kernel"] == "conv2d_generic", m.op(0)["kernel"]
    assert m.op(m.num_ops - 1)["kernel"] not in ("", "(fused into the previous operator)"), m.op(m.num_ops - 1)["kernel"]
