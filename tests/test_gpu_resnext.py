"""tflite_writer.resnext end to end against its TWIN: every grouped Conv2D rewritten as the dense one with the block-diagonal filter
(tests/grouped_ref.twin), the MEAN as the whole-image pool, through the CPU oracle (tests/shortcut_ref.segments: tests/pad_ref.segments
knows no side operator).  The grouped layers are conv_grp_rt launches; MF_NO_CONV_GRP gives the same bytes from the twin."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import grouped_ref as G
from tests import pad_ref as P
from tests import shortcut_ref as S
from tests.conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import tflite_writer as tw  # noqa: E402

pytestmark = pytest.mark.gpu


def expected(in_shape, in_q, layers, elem, xq):
    return S.segments(tw, __import__("oracle.oracle", fromlist=["oracle"]), in_shape, in_q, P.twin_layers(G.twin(layers, in_shape[3]), in_shape), elem)(xq)[-1]


@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
def test_resnext_runs_as_the_composed_operators(u8, tmp_path):
    import microflow_rs_amd as mf
    elem, dt = (tw.UINT8, np.uint8) if u8 else (tw.INT8, np.int8)
    in_shape, in_q, layers = tw.resnext_layers(np.random.default_rng(25), elem=elem)   # 16x16x8, two blocks, G = 4
    blob = tw.build_model(in_shape, in_q, layers, elem)
    m = mf.model(blob)
    xq = (np.random.default_rng(5).integers(-128, 128, (5,) + in_shape[1:]) + (128 if u8 else 0)).astype(dt)
    want = expected(in_shape, in_q, layers, elem, xq)
    got = m.run_quantized(xq).reshape(5, -1)
    assert np.array_equal(got, want), int((got != want).sum())
    grouped = [i for i in range(m.num_ops) if m.op(i)["groups"] != 1]
    assert len(grouped) == 2 and all(m.op(i)["kernel"].startswith("conv_grp_rt<g4") for i in grouped), [m.op(i)["kernel"] for i in grouped]
    path, xpath, ypath = (str(tmp_path / n) for n in ("resnext.tflite", "x.npy", "y.npy"))
    open(path, "wb").write(blob)
    np.save(xpath, xq)
    code = ("import sys, numpy as np, microflow_rs_amd as mf\n"
            "m = mf.model(open(sys.argv[1], 'rb').read()); y = m.run_quantized(np.load(sys.argv[2]))\n"
            "assert not any('conv_grp' in m.op(i)['kernel'] for i in range(m.num_ops)); np.save(sys.argv[3], y)\n")
    subprocess.run([sys.executable, "-c", code, path, xpath, ypath], check=True, timeout=300, cwd=ROOT, env=dict(os.environ, MF_DEV="1", MF_NO_CONV_GRP="1"))
    assert np.array_equal(np.load(ypath).reshape(5, -1), want)


@pytest.mark.parametrize("kind", ["pair", "conv_pool", "side_add"])
def test_the_fused_matchers_pass_a_grouped_operator_by(kind):
    """Each a fused group when the Conv2D is dense; grouped, it launches alone on its own kernel and the model gives its twin's bytes."""
    import microflow_rs_amd as mf
    rng, q, shape = np.random.default_rng(9), (0.05, -3), (12, 12, 16)
    if kind == "pair":
        first = tw._conv_layer(rng, shape, q, True, 16, 3, 1)
        layers, at = [first, tw._conv_layer(rng, shape, first["out_q"], False, 32, 1, 1, groups=4)], 1
    elif kind == "conv_pool":
        first = tw._conv_layer(rng, shape, q, False, 16, 3, 1, groups=4)
        layers, at = [first, dict(op="average_pool_2d", filter=(2, 2), padding="valid", strides=(2, 2), act="none", out_shape=(1, 6, 6, 16), out_q=first["out_q"])], 0
    else:
        side = dict(tw._conv_layer(rng, shape, q, False, 16, 1, 1, "same", "none", groups=4), side_of=-1)
        main = tw._conv_layer(rng, shape, q, False, 16, 3, 1, "same", "none")
        layers, at = [side, main, tw._add_layer(rng, 0, (1, 12, 12, 16), main["out_q"], side["out_q"], "relu")], 0
    in_shape = (1,) + shape
    m = mf.model(tw.build_model(in_shape, q, layers))
    xq = rng.integers(-128, 128, (3,) + shape).astype(np.int8)
    assert np.array_equal(m.run_quantized(xq).reshape(3, -1), expected(in_shape, q, layers, tw.INT8, xq))
    assert m.op(at)["kernel"].startswith("conv_grp_rt<g4"), m.op(at)["kernel"]
    assert m.op(m.num_ops - 1)["kernel"] not in ("", "(fused into the previous operator)"), m.op(m.num_ops - 1)["kernel"]
