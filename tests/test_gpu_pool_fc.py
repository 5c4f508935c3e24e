"""The classifier head AveragePool2D (whole image) -> Reshape -> FullyConnected layers (-> Softmax) as one pool_fc_chain launch
(k_pool_fc.hip): routing, bit-exactness against the CPU oracle every way the model can be run, the bytes around the output, and
the shapes that must keep today's launches."""
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
BATCHES = (1, 17, 333, 4099)
# (H, W, C, FullyConnected sizes, pool_head options)
CASES = [
    (2, 2, 256, (10,), dict(softmax=True, same_q=True)),        # means on .5 ties
    (3, 3, 256, (2,), dict(softmax=True)),                       # over fc_rowwave_softmax<2>; 9 pixels: a ragged block of four
    (7, 7, 64, (10,), dict(softmax=True)),
    (4, 4, 96, (12,), dict()),                                   # 6 channel groups: 2 pixel subsets, 4 idle columns
    (14, 14, 16, (20,), dict(softmax=True)),                     # one channel group, 16 pixel subsets
    (1, 1, 32, (5,), dict()),
    (5, 5, 320, (17, 10), dict(softmax=True)),                   # 20 channel groups: two passes; two layers
    (8, 8, 128, (100, 10), dict(elem=3, wzp_nonzero=True)),      # u8, weight zero points
    (7, 7, 1024, (10,), dict(softmax=True)),                     # a 50 KB image: larger than any LDS buffer
]
IDS = ["%dx%dx%d-%s%s" % (c[0], c[1], c[2], "-".join(map(str, c[3])), "".join("+" + k for k in sorted(c[4]))) for c in CASES]


class Head:
    """one case: the model, its oracle, BATCHES[-1] random images (image 0 all-minimum, image 1 all-maximum) and the oracle's
    outputs for them, computed once (images are independent: a smaller batch is a prefix)"""

    def __init__(self, O, case, seed):
        import microflow_rs_amd as mf
        import tflite_writer as tw
        H, W, C, sizes, kw = case
        self.case, self.sizes, self.softmax = case, sizes, bool(kw.get("softmax"))
        self.blob = tw.pool_head(np.random.default_rng(seed), (H, W, C), sizes, **kw)
        self.m = mf.Model(self.blob)
        self.m.prepare(1)
        self.om = O.Model(self.blob)
        lo, hi = (0, 256) if self.m.dtype == np.uint8 else (-128, 128)
        rng = np.random.default_rng(seed + 1)
        self.x = rng.integers(lo, hi, (BATCHES[-1], self.m.input_elems), dtype=np.int16).astype(self.m.dtype)
        self.x[0], self.x[1] = lo, hi - 1
        self.want = self.om.run_quantized_batch(self.x).reshape(BATCHES[-1], -1)
        self.N = self.want.shape[1]


_heads = {}


@pytest.fixture(params=range(len(CASES)), ids=IDS)
def head(request, O):
    i = request.param
    if i not in _heads:
        _heads[i] = Head(O, CASES[i], 100 + i)
    return _heads[i]


def test_head_is_one_pool_fc_chain_launch(head):
    """the pool operator reports the group, every operator behind it "fused"; fusion off shows the operators' own kernels"""
    if ROUTING_SWITCHED:
        return
    m = head.m
    names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    want0 = "pool_fc_chain<%d>%s" % (len(head.sizes), "+sm" if head.softmax else "")
    assert names[0] == want0, names
    assert names[1] == "" and all(n == FUSED for n in names[2:]), names        # (the Reshape launches nothing)
    assert m.op_epilogue_mode(0) in (0, 1, 2)
    m.set_fusion(False)
    try:
        off = [m.op(i)["kernel"] for i in range(m.num_ops)]
        assert off[0] == "avgpool_c4" and not any(n.startswith("pool_fc_chain") for n in off), off
    finally:
        m.set_fusion(True)


def test_every_row_equals_the_oracle_fused_layerwise_and_generic(head):
    m = head.m
    for n in BATCHES:
        x, want = head.x[:n], head.want[:n]
        got = m.run_quantized(x).reshape(n, -1)
        assert np.array_equal(got, want), (n, int((got != want).any(axis=1).sum()), np.flatnonzero((got != want).any(axis=1))[:8])
        m.set_fusion(False)
        try:
            assert np.array_equal(m.run_quantized(x).reshape(n, -1), want), n
        finally:
            m.set_fusion(True)
        m.set_generic(True)
        try:
            assert np.array_equal(m.run_quantized(x).reshape(n, -1), want), n
        finally:
            m.set_generic(False)


def test_run_until_inside_the_group_equals_the_oracles_layers(head):
    m = head.m
    for k in (0, 1, 5):
        _, layers = head.om.run_quantized(head.x[k], layers=True)
        for i in range(m.num_ops):                      # the pool, the Reshape's alias of it, every FullyConnected, the Softmax
            got = np.asarray(m.run_until(head.x[k:k + 1], i)).reshape(-1)
            assert np.array_equal(got, layers[i].reshape(-1)), (k, i)


def test_graph_replays_give_the_same_bytes(head):
    import torch
    m = head.m
    x = torch.as_tensor(head.x[:333]).cuda()
    ref = m.run_quantized(x).clone()
    assert np.array_equal(ref.cpu().numpy().reshape(333, -1), head.want[:333])
    m.set_graph(True)
    try:
        out = torch.empty_like(ref)
        before = m.graph_launches
        for it in range(4):                            # eager, captured + replayed, replayed, replayed
            out.zero_()
            m.run_quantized(x, out=out)
            assert torch.equal(out, ref), it
        assert m.graph_launches >= before + 2
    finally:
        m.set_graph(False)


def test_bytes_around_the_output_stay(head):
    """the output inside a larger device buffer filled with a sentinel, at a 16-byte-aligned offset (the launch stores into it) and
    at an odd one: exactly batch x N bytes change"""
    import torch
    m = head.m
    dt = torch.uint8 if m.dtype == np.uint8 else torch.int8
    for n in (17, 333):
        x = torch.as_tensor(head.x[:n]).cuda()
        for off in (32, 3):
            buf = torch.full((off + n * head.N + 4096,), 0x5A, dtype=dt, device="cuda")
            m.run_quantized(x, out=buf[off:off + n * head.N])
            b = buf.cpu().numpy()
            assert (b[:off] == 0x5A).all() and (b[off + n * head.N:] == 0x5A).all(), (n, off)
            assert np.array_equal(b[off:off + n * head.N].reshape(n, -1), head.want[:n]), (n, off)


def test_input_view_offset_by_one_byte(head):
    """a device input that is not 16-byte aligned: same bytes (pool_fc_chain loads 16-byte words and is not given such a pointer)"""
    import torch
    m = head.m
    n = 333
    flat = head.x[:n].reshape(-1)
    buf = torch.zeros(flat.size + 64, dtype=torch.uint8 if m.dtype == np.uint8 else torch.int8, device="cuda")
    view = buf[1:1 + flat.size]
    view.copy_(torch.as_tensor(flat))
    assert view.data_ptr() % 16 == 1
    got = m.run_quantized(view).cpu().numpy().reshape(n, -1)
    assert np.array_equal(got, head.want[:n])


# ---- heads that keep today's launches ------------------------------------------------------------------------------------
def _fc_layers(rng, K, sizes, q, softmax=True):
    layers = []
    for N in sizes:
        wsc = np.float32(rng.uniform(0.002, 0.02))
        osc = float(np.float32(max(q[0], 1e-3) * wsc * 60.0 * np.sqrt(K)))
        layers.append(dict(op="fully_connected", weights=rng.integers(-128, 128, (N, K)), wscale=[wsc], wzp=[0], bias=rng.integers(-2000, 2000, N),
                           bscale=[np.float32(q[0]) * wsc], bzp=[0], act="none", out_shape=(1, N), out_q=(osc, int(rng.integers(-100, 100)))))
        q, K = layers[-1]["out_q"], N
    if softmax:
        layers.append(dict(op="softmax", out_shape=(1, K), out_q=(1.0 / 256.0, -128)))
    return layers


def _negative(name):
    import tflite_writer as tw
    rng = np.random.default_rng(7)
    if name == "C24":
        return tw.pool_head(rng, (4, 4, 24), (10,), softmax=True), ["avgpool_c4", "", "fc_generic", "softmax_table"]
    if name == "weights-do-not-fit":
        return tw.pool_head(rng, (2, 2, 256), (1000,), softmax=True), ["avgpool_c4", "", "fc_rt", "softmax_table"]
    in_q = (0.05, 3)
    if name == "four-output-pixels":
        q = (0.04, -5)
        layers = [dict(op="average_pool_2d", filter=(2, 2), padding="valid", strides=(2, 2), act="none", out_shape=(1, 2, 2, 16), out_q=q),
                  dict(op="reshape", out_shape=(1, 64), out_q=q)] + _fc_layers(rng, 64, (10,), q)
        return tw.build_model((1, 4, 4, 16), in_q, layers), ["avgpool_c4", "", "fc_rt", "softmax_table"]
    if name == "non-finite-pool-constants":
        q = (0.0, -5)                                  # c0 = input scale / output scale = inf
        layers = [dict(op="average_pool_2d", filter=(2, 2), padding="valid", strides=(2, 2), act="none", out_shape=(1, 1, 1, 32), out_q=q),
                  dict(op="reshape", out_shape=(1, 32), out_q=q)] + _fc_layers(rng, 32, (10,), q)
        return tw.build_model((1, 2, 2, 32), in_q, layers), None
    raise ValueError(name)


@pytest.mark.parametrize("name", ["C24", "four-output-pixels", "weights-do-not-fit", "non-finite-pool-constants"])
def test_heads_outside_the_group_keep_their_launches(O, name):
    import microflow_rs_amd as mf
    blob, names = _negative(name)
    m = mf.Model(blob)
    m.prepare(1)
    if not ROUTING_SWITCHED:
        got = [m.op(i)["kernel"] for i in range(m.num_ops)]
        assert got[0] == "avgpool_c4" and not any(n.startswith("pool_fc_chain") or n == FUSED for n in got), got
        assert names is None or got == names, got
    rng = np.random.default_rng(8)
    x = rng.integers(-128, 128, (333, m.input_elems)).astype(np.int8)
    x[0], x[1] = -128, 127
    assert np.array_equal(m.run_quantized(x).reshape(333, -1), O.Model(blob).run_quantized_batch(x).reshape(333, -1))


def test_no_pool_fc_switch_goes_back_to_the_operators():
    """MF_DEV=1 MF_NO_POOL_FC=1 (a child process: the switches are read once per process): the head's operators run their own
    launches with the same bytes as pool_fc_chain in the other child"""
    code = r'''
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import microflow_rs_amd as mf
import tflite_writer as tw
m = mf.Model(tw.pool_head(np.random.default_rng(5), (5, 5, 320), (17, 10), softmax=True))
m.prepare(1)
x = np.random.default_rng(6).integers(-128, 128, (333, m.input_elems)).astype(np.int8)
print("KERNELS", "|".join(m.op(i)["kernel"] for i in range(m.num_ops)))
np.save(sys.argv[1], m.run_quantized(x).reshape(333, -1))
''' % (ROOT, os.path.join(ROOT, "tools"))
    outs, kernels = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for sw in (None, "1"):
            env = dict(os.environ)
            for k in [k for k in env if k.startswith("MF_")]:
                del env[k]
            if sw:
                env.update(MF_DEV="1", MF_NO_POOL_FC="1")
            path = os.path.join(tmp, "out%d.npy" % len(outs))
            r = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
            assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
            kernels.append([l for l in r.stdout.splitlines() if l.startswith("KERNELS")][0].split(" ", 1)[1].split("|"))
            outs.append(np.load(path))
    assert np.array_equal(outs[0], outs[1])
    on, off = kernels
    assert on == ["pool_fc_chain<2>+sm", "", FUSED, FUSED, FUSED], on
    assert off[0] == "avgpool_c4" and off[2] != FUSED and not any(n.startswith("pool_fc_chain") for n in off), off
