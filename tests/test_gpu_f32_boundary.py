"""M::predict (f32 in, f32 out) with the boundary quantisation inside the model's first launch and the dequantisation inside its
last one (fc_rt, fc_chain, pool_fc_chain): the floats of the CPU oracle's predict bit for bit -- at half-way points,
zeros, denormals, saturation, infinities and NaN --, the same floats with fusion off and on the shape-generic kernels, the number
of launches (mf_model_device_ops), the floats around the output, overlapping buffers, graph replay, the host-fed path and the dev
switch that brings the two separate passes back."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests.conftest import ROOT, ROUTING_SWITCHED, model_path

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))


def _blob(name):
    import tflite_writer as tw
    rng = np.random.default_rng(41)
    if name in ("sine", "speech", "person_detect"):
        return open(model_path(name), "rb").read()
    return {
        "pd64": lambda: tw.person_detect_like(rng, side=64),
        "pd64-half-u8": lambda: tw.person_detect_like(rng, side=64, width=0.5, elem=tw.UINT8),
        "mlp-20-33-7-sm": lambda: tw.mlp(rng, [20, 33, 7], softmax=True),
        "mlp-u8-wzp": lambda: tw.mlp(rng, [20, 33, 7], elem=tw.UINT8, wzp_nonzero=True, softmax=True),
        "mlp-1-16-1": lambda: tw.mlp(rng, [1, 16, 1]),
        "speech-u8-wzp": lambda: tw.speech_like(rng, elem=tw.UINT8, fc_wzp=9),
        "pool-head": lambda: tw.pool_head(rng, (4, 4, 32), (10,), softmax=True),
        # one FullyConnected layer alone is fc_rt, first and last launch at once; K % 4 != 0 on a u8 model with a weight zero point; 188
        # column tiles, which fc_rt cuts into two slices (each stages the rows again and stores its columns of every row); and fc_rt in
        # front of a Softmax launch (entry only)
        "fc-40-12": lambda: tw.mlp(rng, [40, 12]),
        "fc-37-50-u8": lambda: tw.mlp(rng, [37, 50], elem=tw.UINT8, wzp_nonzero=True),
        "fc-64-3000": lambda: tw.mlp(rng, [64, 3000]),
        "fc-40-12-sm": lambda: tw.mlp(rng, [40, 12], softmax=True),
    }[name]()


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# batches ragged against each kernel's step (16 rows / images); speech also one at which workgroups walk several steps
def _batches(name):
    if name == "sine":
        return (1, 1000)
    if name in ("speech", "speech-u8-wzp"):
        return (37, 3 * _cus() * 16 + 5)
    if name == "person_detect":
        return (19,)
    if name.startswith("pd64"):
        return (33,)
    return (77,)


MODELS = ["sine", "speech", "person_detect", "pd64", "pd64-half-u8", "mlp-20-33-7-sm", "mlp-u8-wzp", "mlp-1-16-1", "speech-u8-wzp", "pool-head",
          "fc-40-12", "fc-37-50-u8", "fc-64-3000", "fc-40-12-sm"]
# the models both of whose ends are inside a launch (first: fc_chain / fc_rt / dwc1_fc_softmax / the stems; last: fc_chain / fc_rt /
# dwc1_fc_softmax / pair3_tail / pair_front_tail): predict is run_quantized's launches
BOTH_ENDS_I8 = ["sine", "speech", "person_detect", "pd64", "mlp-20-33-7-sm", "mlp-1-16-1", "fc-40-12", "fc-64-3000"]
BOTH_ENDS_U8 = ["pd64-half-u8", "mlp-u8-wzp", "speech-u8-wzp", "fc-37-50-u8"]
ONE_END = ["pool-head", "fc-40-12-sm"]                         # (exit only; entry only)


def _inputs(om, n, seed):
    """n f32 images (q - zp) * scale over random q of the element type, with the hard values planted in every image that has room
    for them (an input of fewer elements gets them in turn, in every second image): half-way points (k + 0.5 - zp) * scale incl.
    the two that decide saturation, +-0, denormals, values far beyond both ends, +-inf, NaN"""
    rng = np.random.default_rng(seed)
    lo, hi = (0, 256) if om.dtype == np.uint8 else (-128, 128)
    sc, zp, E = np.float32(om.in_scale), om.in_zp, om.in_elems
    q = rng.integers(lo, hi, (n, E))
    x = ((q - zp).astype(np.float32) * sc).astype(np.float32)
    ks = np.array([lo - 1, lo, lo + 1, zp - 1, zp, hi - 2, hi - 1] + list(rng.integers(lo, hi, 9)), np.float64)
    half = ((ks + 0.5 - zp).astype(np.float32) * sc).astype(np.float32)
    big = np.float32(1e30)
    special = np.concatenate([half, -half, np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, big, -big, 3.4e38, -3.4e38, (hi + 1000 - zp) * sc,
                                                     (lo - 1000 - zp) * sc, np.inf, -np.inf, np.nan, -np.nan], np.float32)]).astype(np.float32)
    ns = special.size
    for b in range(n):
        if E >= 2 * ns:
            x[b, rng.choice(E, ns, replace=False)] = special
        elif b % 2:
            k = min(E, ns)
            x[b, :k] = special[(b // 2 * k + np.arange(k)) % ns]
    return x


class Case:
    """one model: the device model, the oracle, the f32 batch and the oracle's predict for the images checked, computed once"""

    def __init__(self, O, name):
        import microflow_rs_amd as mf
        import torch
        self.name = name
        self.blob = _blob(name)
        self.m = mf.Model(self.blob)
        self.m.prepare(1)
        self.om = O.Model(self.blob)
        self.batches = _batches(name)
        self.n = max(self.batches)
        self.x = _inputs(self.om, self.n, 900 + MODELS.index(name))
        self.N = self.om.out_elems
        # every image of the small batches; on a large one a spread of picked images (first and last step, random ones between)
        small = min(self.batches) if len(self.batches) > 1 and self.n > 2000 else self.n
        picks = set(range(small))
        if self.n > small:
            picks |= set(range(self.n - 21, self.n)) | set(np.random.default_rng(5).integers(0, self.n, 40).tolist())
        self.picks = np.array(sorted(picks))
        self.want = np.stack([self.om.predict(self.x[i]).reshape(-1) for i in self.picks]).astype(np.float32)
        self.xd = torch.as_tensor(self.x).cuda()
        lo, hi = (0, 256) if self.m.dtype == np.uint8 else (-128, 128)
        self.xq = torch.as_tensor(np.random.default_rng(6).integers(lo, hi, (self.n, self.om.in_elems)).astype(self.m.dtype)).cuda()

    def check(self, got, n, what):
        got = np.asarray(got, np.float32).reshape(n, -1)
        sel = self.picks[self.picks < n]
        a, b = got[sel].view(np.uint32), self.want[: sel.size].view(np.uint32)
        bad = np.flatnonzero((a != b).any(axis=1))
        assert not bad.size, (self.name, what, n, "images", sel[bad][:8].tolist(), got[sel[bad[0]]], self.want[bad[0]])


_cases = {}


def _case(O, name):
    if name not in _cases:
        _cases[name] = Case(O, name)
    return _cases[name]


@pytest.fixture(params=MODELS)
def case(request, O):
    return _case(O, request.param)


def _bits(t):
    return t.detach().cpu().numpy().reshape(-1).view(np.uint32)


def test_predict_is_the_oracles_floats_fused_layerwise_and_generic(case):
    m = case.m
    for n in case.batches:
        x = case.xd[:n]
        got = m.predict(x).cpu().numpy()
        case.check(got, n, "default")
        m.set_fusion(False)
        try:
            off = m.predict(x).cpu().numpy()
        finally:
            m.set_fusion(True)
        m.set_generic(True)
        try:
            gen = m.predict(x).cpu().numpy()
        finally:
            m.set_generic(False)
        assert np.array_equal(off.view(np.uint32), got.view(np.uint32)), (case.name, n, "fusion off")
        assert np.array_equal(gen.view(np.uint32), got.view(np.uint32)), (case.name, n, "generic")


def _deltas(m, x, xq, of, oq):
    """device_ops() added by one predict and by one run_quantized (after one of each: scratch buffers are sized by then)"""
    m.predict(x, out=of), m.run_quantized(xq, out=oq)
    a = m.device_ops()
    m.predict(x, out=of)
    b = m.device_ops()
    m.run_quantized(xq, out=oq)
    return b - a, m.device_ops() - b


@pytest.mark.parametrize("name", BOTH_ENDS_I8 + BOTH_ENDS_U8 + ONE_END)
def test_predict_adds_no_launch_where_both_ends_are_inside(O, name):
    """the test the two separate passes fail: with them predict is two launches more than run_quantized on an i8 model.  A u8
    model's run_quantized moves its bytes to the internal domain and back (two passes) and its predict needs neither: two fewer.
    pool_fc_chain dequantises, but reads int8 pixels 16 bytes at a time and keeps the quantise pass: one more; so does a model whose
    last launch is a Softmax's own"""
    import torch
    if ROUTING_SWITCHED:
        pytest.skip("the launch counts describe the default routing, not %s" % ", ".join(ROUTING_SWITCHED))
    c = _case(O, name)
    m, n = c.m, c.batches[0] if name.startswith("speech") else c.batches[-1]
    x, xq = c.xd[:n], c.xq[:n]
    assert x.data_ptr() % 16 == 0 and xq.data_ptr() % 16 == 0
    of = torch.empty((n, c.N), dtype=torch.float32, device="cuda")
    oq = torch.empty((n, c.N), dtype=m._tdtype(), device="cuda")
    dp, dq = _deltas(m, x, xq, of, oq)
    print(name, "predict", dp, "run_quantized", dq)
    assert dq >= 1
    want = dq + 1 if name in ONE_END else dq - 2 if name in BOTH_ENDS_U8 else dq
    assert dp == want, (name, dp, dq)
    c.check(of.cpu().numpy(), n, "out=")


@pytest.mark.parametrize("name", ["sine", "mlp-20-33-7-sm"])
def test_input_view_offset_by_four_bytes_is_one_launch_more(O, name):
    """an f32 input that is not 16-byte aligned keeps the quantise pass (the staging loads 16 bytes): exactly one launch more, same floats"""
    import torch
    c = _case(O, name)
    m, n = c.m, c.batches[-1]
    buf = torch.zeros(n * c.om.in_elems + 8, dtype=torch.float32, device="cuda")
    view = buf[1:1 + n * c.om.in_elems]
    view.copy_(c.xd[:n].reshape(-1))
    assert view.data_ptr() % 16 == 4
    of = torch.empty((n, c.N), dtype=torch.float32, device="cuda")
    oq = torch.empty((n, c.N), dtype=m._tdtype(), device="cuda")
    dp, _ = _deltas(m, c.xd[:n], c.xq[:n], of, oq)
    ref = of.clone()
    dpo, _ = _deltas(m, view.reshape(n, -1), c.xq[:n], of, oq)
    assert np.array_equal(_bits(of), _bits(ref))
    if not ROUTING_SWITCHED:
        assert dpo == dp + 1, (name, dp, dpo)


def test_floats_around_the_output_stay(case):
    """the f32 output inside a larger buffer filled with a pattern, at a 16-byte aligned offset and at an odd float: exactly
    batch x output_elems floats change, and a second call writes the same"""
    import torch
    m, N = case.m, case.N
    pat = np.float32(-1234.5)
    for n in case.batches:
        for off in (64, 3):
            buf = torch.full((off + n * N + 1024,), float(pat), dtype=torch.float32, device="cuda")
            out = buf[off:off + n * N]
            m.predict(case.xd[:n], out=out)
            b1 = buf.cpu().numpy().copy()
            m.predict(case.xd[:n], out=out)
            b2 = buf.cpu().numpy()
            assert (b1[:off] == pat).all() and (b1[off + n * N:] == pat).all(), (case.name, n, off)
            assert np.array_equal(b1.view(np.uint32), b2.view(np.uint32)), (case.name, n, off)
            case.check(b1[off:off + n * N], n, "guarded, offset %d" % off)


@pytest.mark.parametrize("name", ["sine", "speech"])
def test_overlapping_input_and_output_give_the_oracles_floats(O, name):
    """a model that is ONE launch would read and write the same memory: overlapping buffers keep the separate passes"""
    import torch
    c = _case(O, name)
    m, n = c.m, c.batches[0] if name == "speech" else c.batches[-1]
    E, N = c.om.in_elems, c.N
    for shift in (0, 4):                                       # the output at the input's start, and a few floats into it
        buf = torch.zeros(shift + n * max(E, N) + 64, dtype=torch.float32, device="cuda")
        xin = buf[:n * E]
        xin.copy_(c.xd[:n].reshape(-1))
        out = buf[shift:shift + n * N]
        m.predict(xin.reshape(n, -1), out=out)
        c.check(out.cpu().numpy(), n, "overlap, shift %d" % shift)


@pytest.mark.parametrize("name", ["speech", "pd64", "mlp-20-33-7-sm"])
def test_graph_replays_give_the_same_floats(O, name):
    import torch
    c = _case(O, name)
    m, n = c.m, c.batches[0]
    x = c.xd[:n].clone()
    ref = m.predict(x).clone()
    c.check(ref.cpu().numpy(), n, "eager")
    m.set_graph(True)
    try:
        out = torch.empty_like(ref)
        before, ops = m.graph_launches, []
        for it in range(4):                                    # eager, captured + replayed, replayed, replayed
            out.zero_()
            a = m.device_ops()
            m.predict(x, out=out)
            ops.append(m.device_ops() - a)
            assert np.array_equal(_bits(out), _bits(ref)), (name, it)
        assert m.graph_launches >= before + 2
        assert ops[1:] == [1, 1, 1], ops                       # (a replay counts as one)
    finally:
        m.set_graph(False)


def test_host_fed_predict_equals_the_device_fed_one(O):
    c = _case(O, "speech")
    n = 37
    got = c.m.predict(c.x[:n])
    c.check(got, n, "host-fed")
    assert np.array_equal(np.asarray(got).reshape(-1).view(np.uint32), _bits(c.m.predict(c.xd[:n])))
    c = _case(O, "mlp-20-33-7-sm")
    got = c.m.predict(c.x[:77])
    c.check(got, 77, "host-fed")


def test_host_fed_predict_in_two_chunks(O):
    """sine at a batch the staging cuts in two (64 MB of input per chunk): the chunks' slices of the staging buffers do not meet"""
    import torch
    c = _case(O, "sine")
    per = (64 << 20) // 4
    n = per + per // 2 + 1000
    base = c.x.reshape(-1)
    x = np.resize(base, n).astype(np.float32)
    got = np.asarray(c.m.predict(x.reshape(n, 1))).reshape(-1)
    dev = c.m.predict(torch.as_tensor(x).cuda().reshape(n, 1)).cpu().numpy().reshape(-1)
    assert np.array_equal(got.view(np.uint32), dev.view(np.uint32))
    assert np.array_equal(got[:base.size].view(np.uint32), dev[:base.size].view(np.uint32))
    c.check(got[:c.n], c.n, "host-fed, first rows of two chunks")


def test_dev_switch_brings_the_separate_passes_back():
    """MF_DEV=1 MF_NO_F32_BOUNDARY=1 (a child process: the switches are read once per process): predict is two launches more than
    run_quantized again, and the floats are the same as the default child's"""
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import microflow_rs_amd as mf
import tflite_writer as tw
m = mf.Model(tw.mlp(np.random.default_rng(41), [20, 33, 7], softmax=True))
m.prepare(1)
rng = np.random.default_rng(6)
x = torch.as_tensor(rng.normal(0, 2, (77, 20)).astype(np.float32)).cuda()
xq = torch.as_tensor(rng.integers(-128, 128, (77, 20)).astype(np.int8)).cuda()
of = torch.empty((77, 7), dtype=torch.float32, device="cuda")
oq = torch.empty((77, 7), dtype=torch.int8, device="cuda")
m.predict(x, out=of), m.run_quantized(xq, out=oq)
a = m.device_ops(); m.predict(x, out=of); b = m.device_ops(); m.run_quantized(xq, out=oq); c = m.device_ops()
print("OPS", b - a, c - b)
np.save(sys.argv[1], of.cpu().numpy())
''' % (ROOT, os.path.join(ROOT, "tools"))
    outs, ops = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for sw in (None, "1"):
            env = dict(os.environ)
            for k in [k for k in env if k.startswith("MF_")]:
                del env[k]
            if sw:
                env.update(MF_DEV="1", MF_NO_F32_BOUNDARY="1")
            path = os.path.join(tmp, "out%d.npy" % len(outs))
            r = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
            assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
            ops.append([int(v) for v in [l for l in r.stdout.splitlines() if l.startswith("OPS")][0].split()[1:]])
            outs.append(np.load(path))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert ops[0][0] == ops[0][1], ops
    assert ops[1][0] == ops[1][1] + 2, ops
