"""The block form of pair A in the five-operator launch (k_quad.hip BlkPhase: person_detect ops 1..2 inside `penta_rr`, the depthwise
taps as one matrix instruction per 2 x 2 pixel block and channel quad, the pointwise through four isolating operands).  Its results
must be the bytes of the oracle and of the row form, which the quad without the stem (MF_NO_PENTA) and the single pairs (MF_NO_QUAD)
still run.  The geometry of these launches is fixed at 96 x 96; the small axis is the batch: 1, 2, 5 and 13 images (fewer steps
than workgroups, a batch that divides nothing), uniform noise and the structured images.  Every child process is a fresh
interpreter (the switches are read once per process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT, ROUTING_SWITCHED, model_path
from tests.synth import structured_images, synth_i8

pytestmark = pytest.mark.gpu

BATCHES = (1, 2, 5, 13)
STRUCT_FIRST = {13: 0, 5: 13, 2: 18, 1: 20}  # the structured images of a batch; 21..27 go to the f32 and u8 tests
ELEMS = 96 * 96


def _inputs():
    st = structured_images(96)
    cases = {}
    for n in BATCHES:
        cases["noise%d" % n] = synth_i8(3, 0, n, ELEMS)
        cases["struct%d" % n] = st[STRUCT_FIRST[n]:STRUCT_FIRST[n] + n]
    return cases


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, {root!r})
import microflow_rs_amd as mf
from tests.test_gpu_block_dw import _inputs, _run
m = mf.model({root!r} + "/models/person_detect.tflite")
out = _run(m, _inputs())
m.prepare(13)
out["names"] = np.array([m.op(i)["kernel"] for i in range(m.num_ops)])
np.savez({out!r}, **out)
print("child ok")
"""


def _run(m, cases):
    out = {}
    for name, x in cases.items():
        n = x.shape[0]
        xs = x.reshape((n,) + tuple(m.input_shape))
        out[name + ".4"] = np.asarray(m.run_until(xs, 4)).reshape(n, -1)
        out[name + ".8"] = np.asarray(m.run_until(xs, 8)).reshape(n, -1)
        out[name + ".out"] = np.asarray(m.run_quantized(xs)).reshape(n, -1)
    return out


def _child(tmp_path, tag, **switches):
    out = str(tmp_path / (tag + ".npz"))
    env = dict(os.environ, MF_DEV="1", **switches)
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, out=out)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr
    return dict(np.load(out))


@pytest.fixture(scope="module")
def mf():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import microflow_rs_amd as m
    return m


@pytest.fixture(scope="module")
def model(mf):
    return mf.model(model_path("person_detect"))


@pytest.fixture(scope="module")
def cases():
    return _inputs()


@pytest.fixture(scope="module")
def got(model, cases):
    return _run(model, cases)


@pytest.fixture(scope="module")
def names(model):
    model.prepare(13)
    return [model.op(i)["kernel"] for i in range(model.num_ops)]


def _needs_penta(names):
    if ROUTING_SWITCHED:
        pytest.skip("non-default routing")
    assert names[0].startswith("penta_rr"), names   # the parent really ran the five-operator launch ...
    assert names[5].startswith("quad_rr"), names    # ... and ops 5..8 as the quad behind it


@pytest.mark.parametrize("n", BATCHES)
def test_block_form_equals_the_oracle(O, got, cases, n):
    om = O.Model(model_path("person_detect"))
    for kind in ("noise", "struct"):
        x = cases["%s%d" % (kind, n)]
        for b in range(n):
            final, layers = om.run_quantized(x[b], layers=True)
            for last in (4, 8):
                assert np.array_equal(got["%s%d.%d" % (kind, n, last)][b], layers[last].reshape(-1)), (kind, n, b, last)
            assert np.array_equal(got["%s%d.out" % (kind, n)][b], np.asarray(final).reshape(-1)), (kind, n, b)


@pytest.mark.parametrize("switch", ["MF_NO_PENTA", "MF_NO_QUAD"])
def test_block_form_equals_the_row_form(got, names, tmp_path, switch):
    """the row form of the same pair: in the quad without the stem (MF_NO_PENTA), in the single pair launches (MF_NO_QUAD)"""
    _needs_penta(names)
    old = _child(tmp_path, switch.lower(), **{switch: "1"})
    cn = [str(k) for k in old.pop("names")]
    assert not any(k.startswith("penta_rr") for k in cn), cn
    if switch == "MF_NO_PENTA":
        assert cn[1].startswith("quad_rr"), cn
    else:
        assert not any(k.startswith("quad_rr") for k in cn) and cn[1].startswith("dwpw_rr"), cn
    assert sorted(old) == sorted(got)
    for k in got:
        assert np.array_equal(got[k], old[k]), k


def test_block_form_with_the_two_rounding_epilogues(got, names, tmp_path):
    """MF_NO_FMA_EPI: the five-operator launch's instances of the two-rounding epilogue forms, against the default process"""
    _needs_penta(names)
    two = _child(tmp_path, "no_fma_epi", MF_NO_FMA_EPI="1")
    cn = [str(k) for k in two.pop("names")]
    assert cn[0].startswith("penta_rr"), cn
    for k in got:
        assert np.array_equal(got[k], two[k]), k


def test_block_form_behind_the_f32_entry(O, model):
    """predict: the boundary quantisation inside the five-operator launch (its F32IN instance)"""
    om = O.Model(model_path("person_detect"))
    rng = np.random.default_rng(5)
    xq = structured_images(96)[21:26].astype(np.float32)
    xf = ((xq - np.float32(om.in_zp)) * np.float32(om.in_scale) + rng.normal(0, om.in_scale / 3, xq.shape)).astype(np.float32)
    pf = np.asarray(model.predict(xf.reshape((5,) + tuple(model.input_shape)))).reshape(5, -1)
    wf = np.stack([om.predict(x).reshape(-1) for x in xf])
    assert np.array_equal(pf.view(np.uint32), wf.view(np.uint32))


def test_block_form_u8(mf, O):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from make_u8_model import to_u8
    with open(model_path("person_detect"), "rb") as f:
        data = to_u8(f.read())
    m, om = mf.Model(data), O.Model(data)
    x = structured_images(96)[23:28].view(np.uint8) ^ np.uint8(0x80)
    m.prepare(5)
    if not ROUTING_SWITCHED:
        assert m.op(0)["kernel"].startswith("penta_rr"), m.op(0)["kernel"]
    res = _run(m, {"u8": x})
    for b in range(5):
        final, layers = om.run_quantized(x[b], layers=True)
        for last in (4, 8):
            assert np.array_equal(res["u8.%d" % last][b], layers[last].reshape(-1)), (b, last)
        assert np.array_equal(res["u8.out"][b], np.asarray(final).reshape(-1)), b
