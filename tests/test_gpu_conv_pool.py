"""Conv2D + AveragePool2D stages as one conv_pool_rt launch (k_conv_pool.hip): routing, bit-exactness against the CPU oracle at the
smallest shapes where each mechanism of the kernel can go wrong, ragged batches, the bytes around the output, every way a LeNet can
be run, the switch, and the shapes that must keep the launches they had."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests.conftest import ROOT, ROUTING_SWITCHED

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))

FUSED = "(fused into the previous operator)"
U8 = 3
# name: (shape, N, K, conv_pool options, batch)
CASES = {
    "a-28x28x1-6-5x5": ((28, 28, 1), 6, 5, dict(act="relu"), 9),                                   # AL = 1; N % 4 != 0: byte stores
    "b-12x12x6-16-5x5": ((12, 12, 6), 16, 5, dict(act="none", pool_q=0.9), 9),                     # C % 4 != 0
    "c-16x16x3-32-3x3same-relu6": ((16, 16, 3), 32, 3, dict(padding="same", act="relu6", pool_q=1.1), 9),
    "d-u8-wzp-12x12x8-24-pool3x3s2same": ((12, 12, 8), 24, 3, dict(padding="same", act="none", elem=U8, wzp_nonzero=True, pool=(3, 3),
                                                                  pool_padding="same", pool_q=0.8), 9),  # overlapping windows; len 4 / 6 / 9
    "e-11x11x4-8-3x3-pool-valid": ((11, 11, 4), 8, 3, dict(act="relu", pool_q=0.7), 9),             # 9 x 9 -> 4 x 4: last row and column unused
    "f-16x16x16-32-3x3s2": ((16, 16, 16), 32, 3, dict(padding="same", stride=2, act="relu", pool_q=0.9), 9),  # AL = 16
    "g-8x8x64-16-full-range": ((8, 8, 64), 16, 3, dict(padding="same", act="relu", pool_q=0.9), 9),  # accumulators past 2^22: mode 0
    "h-same-quantisation-ties": ((12, 12, 4), 12, 3, dict(padding="same", act="none", pool_q="same"), 9),  # means on .5 ties
    "i-pool-relu": ((12, 12, 4), 8, 3, dict(padding="same", act="none", pool_act="relu", pool_q=0.6), 9),
    "i-pool-relu6": ((12, 12, 4), 8, 3, dict(padding="same", act="none", pool_act="relu6", pool_q=0.3), 9),
    "j-64x64x4-64-bands": ((64, 64, 4), 64, 3, dict(padding="same", act="relu", pool_q=0.9), 3),   # bands, disjoint windows
    "k-48x48x8-96-bands-pool3x3s2same": ((48, 48, 8), 96, 3, dict(padding="same", act="relu", pool=(3, 3), pool_padding="same", pool_q=0.8), 3),  # recomputed rows
    # routed by default where the issue's own shape falls into a class the measurements exclude (below): the same mechanisms
    "l-12x12x8-18-5x5-byte-stores": ((12, 12, 8), 18, 5, dict(act="relu", pool_q=0.9), 9),          # AL = 4; N % 4 != 0 on two tiles
    "m-u8-wzp-12x12x8-24-5x5-pool3x3s2same": ((12, 12, 8), 24, 5, dict(padding="same", act="none", elem=U8, wzp_nonzero=True, pool=(3, 3),
                                                                      pool_padding="same", pool_q=0.8), 9),
    "n-12x12x12-24-3x3-pool-relu6": ((12, 12, 12), 24, 3, dict(padding="same", act="relu6", pool_act="relu6", pool_q=0.5), 9),
}
# The route keeps a class only where one launch measured faster than the two it replaces by more than the spread of the repeats
# (profiles/r14): not with one input channel, fewer than 16 output channels, fewer than 2400 multiply-adds per output
# pixel (KH KW C N) or a plan beyond 80 KiB of LDS.  Those cases must keep their two launches; the kernel runs them under
# MF_DEV=1 MF_CONV_POOL_ALL=1 (test_excluded_classes_run_the_kernel_when_asked).
ROUTED = {n for n, (shape, N, K, kw, _) in CASES.items() if shape[2] != 1 and N >= 16 and K * K * shape[2] * N >= 2400 and n[0] not in "jk"}
assert sorted(n[0] for n in ROUTED) == ["b", "f", "g", "l", "m", "n"], sorted(ROUTED)
MAX_BATCH = {"a-28x28x1-6-5x5": 21, "b-12x12x6-16-5x5": 35}    # ragged batches: G = 9 -> 1, 8, 10, 21; G = 16 -> 1, 15, 17, 35


class Stage:
    """one case: the model, its oracle, random images (image 0 all-minimum, image 1 all-maximum) and the oracle's outputs for them,
    computed once (images are independent: a smaller batch is a prefix)"""

    def __init__(self, O, name, seed):
        import microflow_rs_amd as mf
        import tflite_writer as tw
        shape, N, K, kw, batch = CASES[name]
        self.name, self.batch = name, batch
        self.blob = tw.conv_pool(np.random.default_rng(seed), shape, N, K, **kw)
        self.m = mf.Model(self.blob)
        self.m.prepare(1)
        self.om = O.Model(self.blob)
        n = MAX_BATCH.get(name, batch)
        lo, hi = (0, 256) if self.m.dtype == np.uint8 else (-128, 128)
        self.x = np.random.default_rng(seed + 1).integers(lo, hi, (n, self.m.input_elems), dtype=np.int16).astype(self.m.dtype)
        self.x[0], self.x[1] = lo, hi - 1
        self.want = self.om.run_quantized_batch(self.x).reshape(n, -1)


_stages = {}


def _stage(O, name):
    if name not in _stages:
        _stages[name] = Stage(O, name, 200 + sorted(CASES).index(name))
    return _stages[name]


@pytest.fixture(params=sorted(CASES))
def stage(request, O):
    return _stage(O, request.param)


def _names(m):
    return [m.op(i)["kernel"] for i in range(m.num_ops)]


def test_stage_is_one_conv_pool_rt_launch(stage):
    """the test that fails without the group: the convolution reports it, the pool reports "fused"; fusion off shows their own kernels.
    The classes the measurements exclude keep two launches"""
    if ROUTING_SWITCHED:
        return
    m = stage.m
    names = _names(m)
    if stage.name not in ROUTED:
        assert not names[0].startswith("conv_pool_rt") and names[0] != FUSED and names[1].startswith("avgpool_"), names
        return
    assert names[0].startswith("conv_pool_rt<") and names[0].endswith(">") and ";G" in names[0] and names[1] == FUSED, names
    assert m.op_epilogue_mode(0) in (0, 1, 2)
    if stage.name.startswith("g-"):
        assert m.op_epilogue_mode(0) == 0, m.op_epilogue_mode(0)
    m.set_fusion(False)
    try:
        off = _names(m)
        assert not any(n.startswith("conv_pool_rt") or n == FUSED for n in off) and off[1].startswith("avgpool_"), off
    finally:
        m.set_fusion(True)


def test_every_image_equals_the_oracle_fused_layerwise_and_generic(stage):
    m, n = stage.m, stage.batch
    x, want = stage.x[:n], stage.want[:n]
    got = m.run_quantized(x).reshape(n, -1)
    assert np.array_equal(got, want), (int((got != want).sum()), np.flatnonzero((got != want).any(axis=1))[:8], np.flatnonzero(got[0] != want[0])[:16])
    m.set_fusion(False)
    try:
        assert np.array_equal(m.run_quantized(x).reshape(n, -1), want)
    finally:
        m.set_fusion(True)
    m.set_generic(True)
    try:
        assert np.array_equal(m.run_quantized(x).reshape(n, -1), want)
    finally:
        m.set_generic(False)


def test_the_convolution_alone_is_still_reachable(stage):
    """mf_model_run_until(last_op = the convolution) runs unfused and gives the oracle's layer tensor"""
    for k in (0, 1, 2):
        _, layers = stage.om.run_quantized(stage.x[k], layers=True)
        for i in (0, 1):
            got = np.asarray(stage.m.run_until(stage.x[k:k + 1], i)).reshape(-1)
            assert np.array_equal(got, layers[i].reshape(-1)), (k, i)


def test_ragged_batches(O):
    """1, G - 1, G + 1 and 2 G + 3 images of a whole-image case (G = 16)"""
    st = _stage(O, "b-12x12x6-16-5x5")
    if not ROUTING_SWITCHED:
        assert ";G16>" in _names(st.m)[0], _names(st.m)
    for n in (1, 15, 17, 35):
        got = st.m.run_quantized(st.x[:n]).reshape(n, -1)
        assert np.array_equal(got, st.want[:n]), (n, np.flatnonzero((got != st.want[:n]).any(axis=1)))


@pytest.mark.parametrize("name", ["l-12x12x8-18-5x5-byte-stores", "b-12x12x6-16-5x5", "a-28x28x1-6-5x5"])
def test_bytes_around_the_output_stay(O, name):
    """the output inside a larger device buffer filled with a sentinel, 64 guard bytes on either side, at byte offsets 0, 1 and 5 of a
    16-byte boundary: exactly batch x POH x POW x N bytes change (N % 4 != 0: byte stores; N % 4 == 0: dword stores; two launches)"""
    import torch
    st = _stage(O, name)
    m, n = st.m, st.batch
    dt = torch.uint8 if m.dtype == np.uint8 else torch.int8
    x = torch.as_tensor(st.x[:n]).cuda()
    size = n * st.want.shape[1]
    for off in (64, 65, 69):
        buf = torch.full((off + size + 64,), 0x5A, dtype=dt, device="cuda")
        assert buf.data_ptr() % 16 == 0
        m.run_quantized(x, out=buf[off:off + size])
        b = buf.cpu().numpy()
        assert (b[:off] == 0x5A).all() and (b[off + size:] == 0x5A).all(), off
        assert np.array_equal(b[off:off + size].reshape(n, -1), st.want[:n]), off


def test_input_view_offset_by_one_byte(O):
    """a device input that is not 16-byte aligned: same bytes (conv_pool_rt loads 16-byte words and is not given such a pointer)"""
    import torch
    st = _stage(O, "f-16x16x16-32-3x3s2")
    n = st.batch
    flat = st.x[:n].reshape(-1)
    buf = torch.zeros(flat.size + 64, dtype=torch.int8, device="cuda")
    view = buf[1:1 + flat.size]
    view.copy_(torch.as_tensor(flat))
    assert view.data_ptr() % 16 == 1
    assert np.array_equal(st.m.run_quantized(view).cpu().numpy().reshape(n, -1), st.want[:n])


# ---- every way a LeNet runs ---------------------------------------------------------------------------------------------
class LeNet:
    N = 37

    def __init__(self, O, elem):
        import microflow_rs_amd as mf
        import tflite_writer as tw
        self.blob = tw.lenet(np.random.default_rng(31 + elem), elem=elem, wzp_nonzero=elem == U8)
        self.m = mf.Model(self.blob)
        self.m.prepare(1)
        self.om = O.Model(self.blob)
        lo, hi = (0, 256) if elem == U8 else (-128, 128)
        self.x = np.random.default_rng(41).integers(lo, hi, (self.N, self.m.input_elems), dtype=np.int16).astype(self.m.dtype)
        self.x[0], self.x[1] = lo, hi - 1
        self.want = self.om.run_quantized_batch(self.x).reshape(self.N, -1)
        # (the Softmax at the end leaves few distinct bytes: the second stage's output and the last FullyConnected's, every image)
        lay = [self.om.run_quantized(v, layers=True)[1] for v in self.x]
        self.stage2 = np.stack([l[3].reshape(-1) for l in lay])
        self.logits = np.stack([l[7].reshape(-1) for l in lay])


_lenets = {}


@pytest.fixture(params=[9, U8], ids=["i8", "u8"])
def lenet(request, O):
    if request.param not in _lenets:
        _lenets[request.param] = LeNet(O, request.param)
    return _lenets[request.param]


def _launches(names):
    return sum(1 for n in names if n and n != FUSED)


def test_lenet_is_two_stages_and_the_head(lenet):
    """conv, pool, conv, pool, Reshape, three FullyConnected, Softmax: eight launches become the first stage's two (one input channel:
    a class the measurements exclude), the second stage's one and the FullyConnected chain's"""
    if ROUTING_SWITCHED:
        return
    m = lenet.m
    names = _names(m)
    assert m.num_ops == 9 and names[4] == "", names
    assert names[0].startswith("conv_rows_lds") and names[1] == "avgpool_generic", names
    assert names[2].startswith("conv_pool_rt<12x12x6-16;5x5;p2x2s2;G") and names[3] == FUSED, names
    assert _launches(names) == 3 + _launches(names[5:]) <= 5, names
    m.set_fusion(False)
    try:
        assert _launches(_names(m)) == 8, _names(m)
    finally:
        m.set_fusion(True)


def test_lenet_fused_layerwise_generic_and_until_every_operator(lenet):
    m, n = lenet.m, lenet.N
    got = m.run_quantized(lenet.x).reshape(n, -1)
    assert np.array_equal(got, lenet.want), np.flatnonzero((got != lenet.want).any(axis=1))
    assert np.array_equal(np.asarray(m.run_until(lenet.x, 3)).reshape(n, -1), lenet.stage2)
    assert np.array_equal(np.asarray(m.run_until(lenet.x, 7)).reshape(n, -1), lenet.logits)
    m.set_fusion(False)
    try:
        assert np.array_equal(m.run_quantized(lenet.x).reshape(n, -1), lenet.want)
    finally:
        m.set_fusion(True)
    m.set_generic(True)
    try:
        assert np.array_equal(m.run_quantized(lenet.x).reshape(n, -1), lenet.want)
    finally:
        m.set_generic(False)
    for k in (0, 1, 5):
        _, layers = lenet.om.run_quantized(lenet.x[k], layers=True)
        for i in range(m.num_ops):
            assert np.array_equal(np.asarray(m.run_until(lenet.x[k:k + 1], i)).reshape(-1), layers[i].reshape(-1)), (k, i)


def test_lenet_predict_equals_the_oracle(lenet):
    """f32 in, f32 out: the boundary passes around the stages (conv_pool_rt has no f32 entry or exit)"""
    m = lenet.m
    x = np.random.default_rng(43).uniform(-1.0, 1.0, (5,) + tuple(m.input_shape)).astype(np.float32)
    got = m.predict(x).reshape(5, -1)
    want = np.stack([np.asarray(lenet.om.predict(v)).reshape(-1) for v in x])
    assert np.array_equal(got, want)


def test_lenet_device_resident_graph_and_launch_count(lenet):
    import torch
    m, n = lenet.m, lenet.N
    x = torch.as_tensor(lenet.x).cuda()
    out = torch.empty((n, lenet.want.shape[1]), dtype=x.dtype, device="cuda")
    assert x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    counts = {}
    for fusion in (True, False):
        m.set_fusion(fusion)
        try:
            m.run_quantized(x, out=out)
            before = m.device_ops()
            m.run_quantized(x, out=out)
            counts[fusion] = (m.device_ops() - before, _launches(_names(m)))
            assert np.array_equal(out.cpu().numpy(), lenet.want), fusion
        finally:
            m.set_fusion(True)
    if not ROUTING_SWITCHED:
        # an i8 model's device run is its launches and nothing else; a u8 model's has the same two domain passes either way
        extra = 0 if m.dtype == np.int8 else counts[True][0] - counts[True][1]
        assert extra in (0, 2) and counts[True][0] == counts[True][1] + extra and counts[False][0] == counts[False][1] + extra, counts
    m.set_graph(True)
    try:
        before = m.graph_launches
        for it in range(4):                            # eager, captured + replayed, replayed, replayed
            out.zero_()
            m.run_quantized(x, out=out)
            assert np.array_equal(out.cpu().numpy(), lenet.want), it
        assert m.graph_launches >= before + 2
    finally:
        m.set_graph(False)


def test_no_conv_pool_switch_goes_back_to_the_operators(lenet):
    """MF_DEV=1 MF_NO_CONV_POOL=1 (a child process: the switches are read once per process): the same bytes, and only the two stages'
    names change, to the operators' own kernels"""
    elem = U8 if lenet.m.dtype == np.uint8 else 9
    code = r'''
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import microflow_rs_amd as mf
import tflite_writer as tw
m = mf.Model(tw.lenet(np.random.default_rng(31 + %d), elem=%d, wzp_nonzero=%r))
m.prepare(1)
x = np.load(sys.argv[1])
print("KERNELS", "|".join(m.op(i)["kernel"] for i in range(m.num_ops)))
m.set_fusion(False)
print("OWN", "|".join(m.op(i)["kernel"] for i in range(m.num_ops)))
m.set_fusion(True)
np.save(sys.argv[2], m.run_quantized(x).reshape(len(x), -1))
''' % (ROOT, os.path.join(ROOT, "tools"), elem, elem, elem == U8)
    outs, kernels, own = [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        xin = os.path.join(tmp, "x.npy")
        np.save(xin, lenet.x)
        for sw in (None, "1"):
            env = dict(os.environ)
            for k in [k for k in env if k.startswith("MF_")]:
                del env[k]
            if sw:
                env.update(MF_DEV="1", MF_NO_CONV_POOL="1")
            path = os.path.join(tmp, "out%d.npy" % len(outs))
            r = subprocess.run([sys.executable, "-c", code, xin, path], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
            assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
            kernels.append([l for l in r.stdout.splitlines() if l.startswith("KERNELS")][0].split(" ", 1)[1].split("|"))
            own.append([l for l in r.stdout.splitlines() if l.startswith("OWN")][0].split(" ", 1)[1].split("|"))
            outs.append(np.load(path))
    assert np.array_equal(outs[0], lenet.want) and np.array_equal(outs[1], lenet.want)
    on, off = kernels
    assert on[2].startswith("conv_pool_rt<") and on[3] == FUSED, on
    assert off[:4] == own[1][:4] == own[0][:4], (off, own)            # the operators' own kernels, what fusion off runs
    assert off[1] == "avgpool_generic" and off[3] == "avgpool_c4" and not any(n.endswith("_generic") for n in (off[0], off[2])), off
    assert off[:2] == on[:2] and off[4:] == on[4:], (on, off)         # only the routed stage's two names change


def test_excluded_classes_run_the_kernel_when_asked(O):
    """MF_DEV=1 MF_CONV_POOL_ALL=1 (a child process): every case the route excludes by measurement -- one input channel, N % 4 != 0 on
    one tile, few channels, both band cases -- is one conv_pool_rt launch and gives the oracle's bytes; ragged batches of a whole-image
    case (G = 9: 1, 8, 10, 21) and of a band case (1, 2); 64 guard bytes around a band case's output"""
    excluded = sorted(set(CASES) - ROUTED)
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import microflow_rs_amd as mf
import tflite_writer as tw
d = np.load(sys.argv[1], allow_pickle=False)
for name in sys.argv[2:]:
    m = mf.Model(bytes(d["blob_" + name]))
    m.prepare(1)
    x, want = d["x_" + name], d["want_" + name]
    names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    assert names[0].startswith("conv_pool_rt<") and names[1] == "(fused into the previous operator)", names
    for n in [int(v) for v in d["batches_" + name]]:
        got = m.run_quantized(x[:n]).reshape(n, -1)
        assert np.array_equal(got, want[:n]), (name, n, int((got != want[:n]).sum()))
    if name[0] in "ja":
        n, size = len(x), want.size
        buf = torch.full((64 + size + 64,), 0x5A, dtype=torch.int8, device="cuda")
        m.run_quantized(torch.as_tensor(x).cuda(), out=buf[64:64 + size])
        b = buf.cpu().numpy()
        assert (b[:64] == 0x5A).all() and (b[64 + size:] == 0x5A).all() and np.array_equal(b[64:64 + size].reshape(n, -1), want), name
    print("OK", name, names[0], flush=True)
''' % (ROOT, os.path.join(ROOT, "tools"))
    data = {}
    for name in excluded:
        st = _stage(O, name)
        data["blob_" + name] = np.frombuffer(st.blob, np.uint8)
        data["x_" + name], data["want_" + name] = st.x, st.want
        data["batches_" + name] = np.array({"a": (1, 8, 10, 21), "j": (1, 2, 3)}.get(name[0], (st.batch,)))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cases.npz")
        np.savez(path, **data)
        env = {k: v for k, v in os.environ.items() if not k.startswith("MF_")}
        env.update(MF_DEV="1", MF_CONV_POOL_ALL="1")
        r = subprocess.run([sys.executable, "-c", code, path] + excluded, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    ok = {l.split()[1]: l.split()[2] for l in r.stdout.splitlines() if l.startswith("OK ")}
    assert sorted(ok) == excluded, (sorted(ok), excluded)
    assert ";PB16;NB2>" in ok["j-64x64x4-64-bands"] and ";PB12;NB2>" in ok["k-48x48x8-96-bands-pool3x3s2same"] and ";G9>" in ok["a-28x28x1-6-5x5"], ok


# ---- what must keep its launches ------------------------------------------------------------------------------------------
def _pair_then_pool(rng):
    """depthwise 3x3 + Conv2D 1x1 + AveragePool2D 2x2: the Conv2D belongs to its pair"""
    import tflite_writer as tw
    in_q = (0.05, -3)
    C = 16
    sc = rng.uniform(0.002, 0.01, C).astype(np.float32)
    dw = dict(op="depthwise_conv_2d", weights=rng.integers(-128, 128, (1, 3, 3, C)), fscale=sc, fzp=np.zeros(C, np.int64), bias=rng.integers(-500, 500, C),
              bscale=(sc * np.float32(in_q[0])).astype(np.float32), bzp=np.zeros(C, np.int64), padding="same", strides=(1, 1), act="relu6",
              out_shape=(1, 16, 16, C), out_q=(float(np.float32(in_q[0] * float(sc.mean()) * 180.0)), -128))
    layers, _, _ = tw.conv_pool_layers(rng, (16, 16, C), dw["out_q"], 32, 1, padding="same", act="relu6", pool_q=0.9)
    return tw.build_model((1, 16, 16, C), in_q, [dw] + layers)


def _kept(name):
    import tflite_writer as tw
    rng = np.random.default_rng(9)
    if name == "global-pool-keeps-pool_fc_chain":      # the CIFAR model of tests/test_gpu_conv_gemm.py
        convs = [("conv", 32, 3, 1), ("conv", 64, 3, 2), ("conv", 128, 3, 1), ("conv", 128, 3, 2), ("conv", 256, 3, 1)]
        return tw.conv_net(np.random.default_rng(11), (32, 32, 3), convs, head=10)
    if name == "pair-keeps-its-group":
        return _pair_then_pool(rng)
    if name == "weights-do-not-fit":
        return tw.conv_pool(rng, (8, 8, 128), 256, 3, padding="same", act="relu", wmax=16, pool_q=0.9)
    if name == "one-image-beyond-half-the-lds":        # 32x32x32 -> 64: a 126 KiB plan, measured x0.74
        return tw.conv_pool(rng, (32, 32, 32), 64, 3, padding="same", act="relu", wmax=32, pool_q=0.9)
    if name == "few-multiply-adds-per-pixel":          # 32x32x3 -> 32 3x3, 864 per output pixel: the sweep's x0.78
        return tw.conv_pool(rng, (32, 32, 3), 32, 3, padding="same", act="relu", pool_q=0.9)
    if name == "rows-not-whole-dwords":
        return tw.conv_pool(rng, (9, 9, 3), 8, 3, padding="same", act="relu", pool_q=0.9)
    raise ValueError(name)


@pytest.mark.parametrize("name", ["global-pool-keeps-pool_fc_chain", "pair-keeps-its-group", "weights-do-not-fit", "rows-not-whole-dwords",
                                  "one-image-beyond-half-the-lds", "few-multiply-adds-per-pixel"])
def test_shapes_outside_the_group_keep_their_launches(O, name):
    import microflow_rs_amd as mf
    blob = _kept(name)
    m = mf.Model(blob)
    m.prepare(1)
    if not ROUTING_SWITCHED:
        got = _names(m)
        assert not any(n.startswith("conv_pool_rt") for n in got), got
        if name == "global-pool-keeps-pool_fc_chain":
            assert got[5].startswith("pool_fc_chain<") and got[4] != FUSED, got
        elif name == "pair-keeps-its-group":
            assert got[1] == FUSED and got[2].startswith("avgpool_"), got
        else:
            assert got[0] != FUSED and got[1].startswith("avgpool_"), got
    n = 5
    x = np.random.default_rng(8).integers(-128, 128, (n, m.input_elems)).astype(np.int8)
    x[0], x[1] = -128, 127
    assert np.array_equal(m.run_quantized(x).reshape(n, -1), O.Model(blob).run_quantized_batch(x).reshape(n, -1))
