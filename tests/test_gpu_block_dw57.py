"""The block form of pair A in the launch of ops 5..8 (k_quad.hip Blk32Phase inside `quad_rr<24,24,32,...>`: the depthwise taps as one
matrix instruction per 2 x 2 pixel block and channel quad, gathered from the DMA-staged NHWC tile; the 1 x 1 behind a barrier).  The
tensors behind op 6, op 8, op 10 and op 12 must be the bytes of the oracle and of the single pair launches (MF_NO_QUAD, a fresh
process: the switches are read once).  The launches' shapes are fixed; the small axis is the batch:
  1, 2, 3, 5    fewer steps than workgroups; the odd ones leave quad_mm (two images per step) a half-empty last step
  1029          above 2 x 256 x 2 images: every workgroup of both launches walks several steps through its step queue (and odd)
Models: the shipped person_detect (i8, the single-fma epilogue: mode 3), its u8 twin (mode 2), and the person_detect-shaped models of
tests/pd_quant.py -- input zero points other than the type's minimum (a wrong halo byte shows), relu6 / relu / no activation, full-range
weights, launches on mode 1; MF_NO_FMA_EPI puts the shipped models on the two-rounding forms.
A batch repeats six distinct images, so the oracle runs six times per model and the big batch is compared row by row with them."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import pd_quant as P
from tests.conftest import ROOT, ROUTING_SWITCHED, model_path
from tests.synth import structured_images, synth_i8

pytestmark = pytest.mark.gpu

PD_MODELS = ("shifted-i8", "shifted-u8", "varied-i8", "varied-u8")
MODELS = ("person_detect", "person_detect-u8") + PD_MODELS
BATCHES = (1, 2, 3, 5, 1029)
LASTS = (6, 8, 10, 12)
NDIST = 6


def blob(name):
    if name in PD_MODELS:
        return P.blob(name)
    with open(model_path("person_detect"), "rb") as f:
        data = f.read()
    if name.endswith("-u8"):
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from make_u8_model import to_u8
        data = to_u8(data)
    return data


def distinct(name):
    """[6, 96 * 96] in the model's element type"""
    if name in PD_MODELS:
        return P.inputs(name)
    x = np.concatenate([synth_i8(57, 0, 3, 96 * 96), structured_images(96)[[3, 22, 25]]])
    return x.view(np.uint8) ^ np.uint8(0x80) if name.endswith("-u8") else x


def rows(n):
    """the distinct image behind every row of a batch of n (a small batch does not always start at image 0)"""
    return [(n + i) % NDIST for i in range(n)]


def _run(m, name):
    """per batch and tensor: the first NDIST rows, and whether every further row equals the row of the same image among them"""
    d = distinct(name)
    out = {}
    for n in BATCHES:
        idx = rows(n)
        xs = d[idx].reshape((n,) + tuple(m.input_shape))
        for last in LASTS:
            got = np.asarray(m.run_until(xs, last)).reshape(n, -1)
            key = "%s.%d.%d" % (name, n, last)
            out[key] = got[:NDIST].copy()
            first = {idx[i]: i for i in reversed(range(min(n, NDIST)))}
            out[key + ".repeats"] = np.array(all(np.array_equal(got[i], got[first[idx[i]]]) for i in range(NDIST, n)))
    m.prepare(5)
    out[name + ".names"] = np.array([m.op(i)["kernel"] for i in range(m.num_ops)])
    out[name + ".modes"] = np.array([m.op_epilogue_mode(i) for i in range(m.num_ops)])
    return out


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, {root!r})
import microflow_rs_amd as mf
from tests.test_gpu_block_dw57 import _run, blob
out = {{}}
for name in {names!r}:
    out.update(_run(mf.Model(blob(name)), name))
np.savez({out!r}, **out)
print("child ok")
"""


def _child(tmp_path, tag, names, **switches):
    out = str(tmp_path / (tag + ".npz"))
    env = dict(os.environ, MF_DEV="1", **switches)
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, out=out, names=tuple(names))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr
    return dict(np.load(out))


@pytest.fixture(scope="module")
def mf():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import microflow_rs_amd as m
    return m


@pytest.fixture(scope="module")
def got(mf):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run(mf.Model(blob(name)), name)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def want(O):
    cache = {}

    def get(name):
        if name not in cache:
            om = O.Model(blob(name))
            runs = [om.run_quantized(x, layers=True)[1] for x in distinct(name)]
            cache[name] = {last: np.stack([r[last].reshape(-1) for r in runs]) for last in LASTS}
        return cache[name]
    return get


def _on_the_quads(res, name):
    names = [str(k) for k in res[name + ".names"]]
    if not ROUTING_SWITCHED:
        assert names[5].startswith("quad_rr<24,24,32") and names[9].startswith("quad_mm<12,12,64"), names
    return names


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("name", MODELS)
def test_block_form_equals_the_oracle(got, want, name, n):
    res, w = got(name), want(name)
    _on_the_quads(res, name)
    idx = rows(n)[:NDIST]
    for last in LASTS:
        key = "%s.%d.%d" % (name, n, last)
        assert np.array_equal(res[key], w[last][idx].view(res[key].dtype)), key
        assert bool(res[key + ".repeats"]), key


def test_block_form_equals_the_pair_launches(got, tmp_path):
    """the row form of the same pairs, one launch per pair (MF_NO_QUAD)"""
    if ROUTING_SWITCHED:
        pytest.skip("non-default routing")
    old = _child(tmp_path, "no_quad", MODELS, MF_NO_QUAD="1")
    for name in MODELS:
        cn = [str(k) for k in old[name + ".names"]]
        assert not any(k.startswith(("quad_", "penta_")) for k in cn), cn
        res = got(name)
        for key in res:
            if not key.endswith((".names", ".modes")):
                assert np.array_equal(res[key], old[key]), key


def test_block_form_with_the_two_rounding_epilogues(got, want, tmp_path):
    """MF_NO_FMA_EPI: the shipped models on the two-rounding forms; with the default runs of all models every mode has run"""
    if ROUTING_SWITCHED:
        pytest.skip("non-default routing")
    shipped = MODELS[:2]
    two = _child(tmp_path, "no_fma_epi", shipped, MF_NO_FMA_EPI="1")
    seen = {int(got(name)[name + ".modes"][5]) for name in MODELS}
    assert int(got("person_detect")["person_detect.modes"][5]) == 3, seen
    for name in shipped:
        _on_the_quads(two, name)
        assert int(two[name + ".modes"][5]) in (1, 2) and int(two[name + ".modes"][9]) in (1, 2), two[name + ".modes"]
        seen.add(int(two[name + ".modes"][5]))
        for n in BATCHES:
            idx = rows(n)[:NDIST]
            for last in LASTS:
                key = "%s.%d.%d" % (name, n, last)
                assert np.array_equal(two[key], want(name)[last][idx].view(two[key].dtype)), key
                assert bool(two[key + ".repeats"]), key
    assert seen == {1, 2, 3}, seen
