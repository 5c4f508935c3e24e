"""The fused table launches of person_detect (penta_rr, quad_rr, quad_mm, stage_6x6x128, pair_front_tail, and the dwpw_rr / dwpw_mm
pairs behind them) under activation quantisations the shipped model does not have.  The launches exist for the 96 x 96, width-1.0
shapes only, and every model of those shapes elsewhere in the suite has scale 6/255, zero point = the type's minimum and relu6 on
every tensor: clamps that are the whole range, padding fills of one byte value, and launches whose members all agree about the
epilogue form.  tests/pd_quant.py builds the same shapes under the plans of tools/tflite_writer.pd_quant_plan -- clamps inside the
range, zero points that differ between the operators of one launch, launches in which one member has no single-fma form -- and
tests/test_pd_quant_host.py shows on the oracle's tensors that every such bound is really held.  Here every launch's output is
compared with the CPU oracle, bit for bit: six images per model (constant lo, constant hi - 1, two of noise, two structured)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import pd_quant as P
from tests.conftest import ROOT, ROUTING_SWITCHED
from tests.synth import structured_images

pytestmark = pytest.mark.gpu

SWITCH_MODELS = ("varied-i8", "stage-i8")
CHILD_LASTS = (4, 8, 12, 22)   # the ends of the four launches in front (n_stage = 5)


class _Case:
    def __init__(self, mf, O, name):
        self.name, self.elem, self.nst = name, P.MODELS[name][1], P.MODELS[name][2]
        blob = P.blob(name)
        self.m, self.om = mf.Model(blob), O.Model(blob)
        self.x = P.inputs(name)
        runs = [self.om.run_quantized(x, layers=True) for x in self.x]
        self.want = np.stack([np.asarray(r[0]).reshape(-1) for r in runs])
        self.layers = [np.stack([r[1][i].reshape(-1) for r in runs]) for i in range(self.om.num_ops)]
        self.m.prepare(len(self.x))
        self.kernels = [self.m.op(i)["kernel"] for i in range(self.m.num_ops)]
        self.modes = [self.m.op_epilogue_mode(i) for i in range(self.m.num_ops)]

    def xs(self):
        return self.x.reshape((len(self.x),) + tuple(self.m.input_shape))

    def starts(self):
        """first operator of every launch of the fused step"""
        return [i for i, k in enumerate(self.kernels) if k and not k.startswith("(fused")]


@pytest.fixture(scope="module")
def mf():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import microflow_rs_amd as m
    return m


@pytest.fixture(scope="module")
def case(mf, O):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Case(mf, O, name)
        return cache[name]
    return get


def _until(c, last, rows=slice(None)):
    return np.asarray(c.m.run_until(c.xs()[rows], last)).reshape(c.layers[last][rows].shape)


@pytest.mark.parametrize("name", P.NAMES)
def test_fused_launches_equal_the_oracle(case, name):
    """the fused step's output, the tensor at the end of every one of its launches, and the dequantised output"""
    c = case(name)
    print("LAUNCHES", name, [(i, c.kernels[i], c.modes[i]) for i in c.starts()])
    starts = c.starts()
    ends = [i - 1 for i in starts[1:]] + [c.m.num_ops - 1]
    for last in ends:
        got = _until(c, last)
        bad = [b for b in range(len(c.x)) if not np.array_equal(got[b], c.layers[last][b])]
        assert not bad, (last, c.kernels[starts[ends.index(last)]], bad, int((got != c.layers[last]).sum()))
    got = np.asarray(c.m.run_quantized(c.xs())).reshape(c.want.shape)
    assert np.array_equal(got, c.want)
    pf = np.asarray(c.m.predict_quantized(c.xs()), np.float32).reshape(len(c.x), -1)
    wf = np.stack([c.om.predict_quantized(x).reshape(-1) for x in c.x]).astype(np.float32)
    assert np.array_equal(pf.view(np.uint32), wf.view(np.uint32))


@pytest.mark.parametrize("name", P.NAMES)
def test_layer_wise_and_generic_equal_the_oracle(case, name):
    """the same models without fusion (every conv-like layer) and on the shape-generic kernels"""
    c = case(name)
    try:
        c.m.set_fusion(False)
        assert np.array_equal(np.asarray(c.m.run_quantized(c.xs())).reshape(c.want.shape), c.want)
        for last in P.conv_like(c.om.ops):
            assert np.array_equal(_until(c, last), c.layers[last]), (last, c.m.op(last)["kernel"])
    finally:
        c.m.set_fusion(True)
    try:
        c.m.set_generic(True)
        assert np.array_equal(np.asarray(c.m.run_quantized(c.xs())).reshape(c.want.shape), c.want)
    finally:
        c.m.set_generic(False)


@pytest.mark.parametrize("name", P.NAMES)
def test_routing_and_epilogue_modes(case, O, name):
    """Any activation quantisation lands in the table launches (the routes look at shapes only); a stage run whose pairs read
    different zero points does not become a stage launch; and a launch with one member whose clamp is not the whole range leaves
    the single-fma form (mode 3) as a whole, whatever its other members could do."""
    if ROUTING_SWITCHED:
        pytest.skip("non-default routing")
    c = case(name)
    k, L = c.kernels, P.launches(c.nst)
    assert k[0].startswith("penta_rr") and k[5].startswith("quad_rr") and k[9].startswith("quad_mm"), k
    assert k[L["pair_front_tail"][0]].startswith("pair_front_tail"), k
    if P.MODELS[name][0] == "varied":
        assert not [n for n in k if n.startswith("stage")], k   # fused_stages.hip fused_stage_create: the izp4 refusal
    else:
        assert k[13] == "stage_6x6x128<4,512,%d>" % c.nst, k
    lo, hi = P.limits(c.elem)
    starts = c.starts()
    seen = 0
    for first, nxt in zip(starts, starts[1:] + [c.m.num_ops]):
        members = [i for i in P.conv_like(c.om.ops) if first <= i < nxt]
        if any(P.clamp(O, c.om.ops[i], c.elem) != (lo, hi - 1) for i in members):
            seen += 1
            assert c.modes[first] <= 2, (first, k[first], c.modes[first])
    assert seen >= 5, (seen, starts)
    if name == "one_odd-i8":   # the launches leave mode 3 although other members of theirs have a single-fma form of their own
        assert c.modes[0] <= 2 and c.modes[5] <= 2, c.modes
        try:
            c.m.set_fusion(False)   # (layer-wise, an operator's launch is its own: its own mode)
            own = [c.m.op_epilogue_mode(i) for i in range(c.m.num_ops)]
        finally:
            c.m.set_fusion(True)
        for launch in ("penta_rr", "quad_rr", "quad_mm", "stage"):
            first, last = L[launch]
            with_form = [i for i in range(first, last + 1) if own[i] == 3]
            print("ONE_ODD", launch, "members with a single-fma form:", with_form, "launch mode", c.modes[first])
            assert with_form and c.modes[first] <= 2, (launch, own[first:last + 1])


def test_f32_entry_with_another_input_quantisation(case):
    """predict on shifted-i8 (input scale 0.0125, zero point mid + 20): the five-operator launch's F32IN instance with a stem fill
    and an input quantiser that are not person_detect's"""
    c = case("shifted-i8")
    om = c.om
    assert (float(om.in_scale), om.in_zp) == (float(np.float32(P.F32_IN_Q[0])), P.F32_IN_Q[1])
    rng = np.random.default_rng(5)
    xq = structured_images(96)[21:26].astype(np.float32)
    xf = ((xq - np.float32(om.in_zp)) * np.float32(om.in_scale) + rng.normal(0, om.in_scale / 3, xq.shape)).astype(np.float32)
    pf = np.asarray(c.m.predict(xf.reshape((5,) + tuple(c.m.input_shape)))).reshape(5, -1)
    wf = np.stack([om.predict(x).reshape(-1) for x in xf])
    assert np.array_equal(pf.view(np.uint32), wf.view(np.uint32))
    if not ROUTING_SWITCHED:
        assert c.kernels[0].startswith("penta_rr"), c.kernels


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, {root!r})
import microflow_rs_amd as mf
from tests import pd_quant as P
from tests.test_gpu_pd_quant import SWITCH_MODELS, _run
out = {{}}
for name in SWITCH_MODELS:
    m = mf.Model(P.blob(name))
    out.update(_run(m, name))
    out[name + ".names"] = np.array([m.op(i)["kernel"] for i in range(m.num_ops)])
np.savez({out!r}, **out)
print("child ok")
"""


def _run(m, name):
    x = P.inputs(name)
    xs = x.reshape((len(x),) + tuple(m.input_shape))
    m.prepare(len(x))
    out = {"%s.%d" % (name, last): np.asarray(m.run_until(xs, last)).reshape(len(x), -1) for last in CHILD_LASTS}
    out[name + ".out"] = np.asarray(m.run_quantized(xs)).reshape(len(x), -1)
    return out


@pytest.mark.parametrize("switch", ["MF_NO_PENTA", "MF_NO_QUAD"])
def test_switch_comparators_give_the_same_bytes(case, tmp_path, switch):
    """varied-i8 and stage-i8 in a fresh process without the five-operator launch (MF_NO_PENTA: ops 1..4 as the quad's row form)
    and without any quad (MF_NO_QUAD: single pair launches): other kernels, other tables, the same bytes"""
    path = str(tmp_path / (switch.lower() + ".npz"))
    env = dict(os.environ, MF_DEV="1", **{switch: "1"})
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, out=path)], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr
    child = dict(np.load(path))
    for name in SWITCH_MODELS:
        c = case(name)
        cn = [str(k) for k in child.pop(name + ".names")]
        assert not any(k.startswith("penta_rr") for k in cn), cn
        if switch == "MF_NO_QUAD":
            assert not any(k.startswith("quad_") for k in cn), cn
        for last in CHILD_LASTS:
            assert np.array_equal(child["%s.%d" % (name, last)], c.layers[last]), (name, last)
        here = _run(c.m, name)
        for key, v in here.items():
            assert np.array_equal(child[key], v), key
