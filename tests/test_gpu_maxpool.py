"""MaxPool2D on the GPU (maxpool_generic and maxpool_c4, k_generic.hip): every operator case against the numpy restatement of the
contract (tests/maxpool_ref.py: the oracle knows no max pool) and against the shape-generic kernel of the same handle, the bytes
around the output, and a LeNet written with max pools in every way a model can be run, against expected tensors computed segment by
segment (the oracle for each run of reference operators, the restatement for the pools between them)."""
import os
import sys

import numpy as np
import pytest

from tests.conftest import ROOT, ROUTING_SWITCHED
from tests import maxpool_ref as R

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))

U8 = 3
# (H, W), filter, strides, padding, (OH, OW)
GEOMETRIES = {
    "2x2s2-valid-6x6": ((6, 6), (2, 2), (2, 2), "valid", (3, 3)),
    "3x3s2-same-7x9": ((7, 9), (3, 3), (2, 2), "same", (4, 5)),          # border windows lose taps on every side
    "3x3s1-same-5x5": ((5, 5), (3, 3), (1, 1), "same", (5, 5)),
    "2x3s1x2-same-6x7": ((6, 7), (2, 3), (1, 2), "same", (6, 4)),
}
ACTS = {"none": 0, "relu": 1, "relu6": 3}
BATCH = 5


def _quantisations(u8):
    """equal (what converters emit; the input zero point the below-zero-point image needs: 100 / 228), and unequal (0.05, 3) ->
    (0.07, -5) in i8, the same + 128 in u8"""
    off = 128 if u8 else 0
    return {"equal": ((0.05, 100 + off), (0.05, 100 + off)), "unequal": ((0.05, 3 + off), (0.07, -5 + off))}


def _images(dt, H, W, C, seed):
    """the two extreme images, one entirely below the input zero point and below 0 in the i8 domain (a zero- or zero-point-filled halo
    would win every border window of it), two random ones"""
    lo = 0 if dt == np.uint8 else -128
    rng = np.random.default_rng(seed)
    x = rng.integers(lo, lo + 256, (BATCH, H, W, C), dtype=np.int16)
    x[0], x[1] = lo, lo + 255
    x[2] = rng.integers(lo, lo + 128, (H, W, C))
    return x.astype(dt)


@pytest.mark.parametrize("dt", [np.int8, np.uint8], ids=["i8", "u8"])
@pytest.mark.parametrize("C", [1, 3, 4, 8, 20])
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_operator_equals_the_restatement_and_its_generic_kernel(geo, C, dt):
    import torch
    import microflow_rs_amd as mf
    from microflow_rs_amd import _lib
    (H, W), filt, strides, padding, out_hw = GEOMETRIES[geo]
    u8 = dt == np.uint8
    x = _images(dt, H, W, C, 7 * C + len(geo))
    tdt = torch.uint8 if u8 else torch.int8
    xd = torch.as_tensor(x).cuda()
    size = BATCH * out_hw[0] * out_hw[1] * C
    for qname, (in_q, out_q) in _quantisations(u8).items():
        assert (x[2].astype(int) < in_q[1]).all() and (x[2].astype(int) - (128 if u8 else 0) < 0).all()
        c0, c1 = R.pool_constants(in_q[0], in_q[1], out_q[0], out_q[1])
        for act, code in ACTS.items():
            want = R.max_pool_2d(x, filt, strides, padding, out_hw, c0, c1, act, out_q[0], out_q[1])
            opts = mf.ops.MaxPool2DOptions(mf.FusedActivation(code), mf.TensorViewPadding(0 if padding == "same" else 1), strides)
            op = mf.ops.prepare_max_pool_2d((H, W, C), filt, out_q[0], out_q[1], opts, (c0, c1), out_hw, dtype=dt)
            if not ROUTING_SWITCHED:
                assert op.kernel == ("maxpool_c4" if C % 4 == 0 else "maxpool_generic"), op.kernel
            got = op(x)
            assert got.dtype == dt and np.array_equal(got, want), (qname, act, np.argwhere(got != want)[:8].tolist())
            if qname == "equal" and act == "none":   # the plain window max, and image 2's border windows hold real taps only
                assert (got[2].astype(int) < in_q[1]).all()
            # the output inside a larger buffer: 64 guard bytes on either side stay
            buf = torch.full((64 + size + 64,), 0x5A, dtype=tdt, device="cuda")
            _lib.check(_lib.lib().mf_op_run(op._h, xd.data_ptr(), BATCH, buf.data_ptr() + 64, torch.cuda.current_stream().cuda_stream))
            b = buf.cpu().numpy()
            assert (b[:64] == 0x5A).all() and (b[64 + size:] == 0x5A).all() and np.array_equal(b[64:64 + size], want.reshape(-1)), (qname, act)
            op.set_generic(True)
            assert op.kernel == "maxpool_generic"
            assert np.array_equal(op(x), want), (qname, act, "generic")
            op.set_generic(False)


@pytest.mark.parametrize("dt", [np.int8, np.uint8], ids=["i8", "u8"])
def test_equal_quantisation_is_the_window_max_of_every_byte(dt):
    """256 images, image v holding v in every window and nothing above it: both kernels return v everywhere"""
    import microflow_rs_amd as mf
    lo = 0 if dt == np.uint8 else -128
    vals = np.arange(lo, lo + 256)
    x = np.minimum(np.random.default_rng(3).integers(lo, lo + 256, (256, 4, 4, 4)), vals[:, None, None, None])
    x[:, ::2, 1::2, :] = vals[:, None, None, None]
    x = x.astype(dt)
    for zp in (lo + 100, lo, lo + 255):
        c0, c1 = R.pool_constants(0.0235294122, zp, 0.0235294122, zp)
        opts = mf.ops.MaxPool2DOptions(mf.FusedActivation(0), mf.TensorViewPadding(1), (2, 2))
        op = mf.ops.prepare_max_pool_2d((4, 4, 4), (2, 2), 0.0235294122, zp, opts, (c0, c1), (2, 2), dtype=dt)
        want = np.broadcast_to(vals[:, None, None, None], (256, 2, 2, 4)).astype(dt)
        assert np.array_equal(op(x), want), zp
        assert np.array_equal(op.set_generic(True)(x), want), zp


def test_a_misaligned_buffer_takes_the_byte_wise_kernel():
    """an input one byte off a 16-byte boundary: maxpool_c4 loads dwords and is not given such a pointer"""
    import torch
    import microflow_rs_amd as mf
    from microflow_rs_amd import _lib
    (H, W), filt, strides, padding, out_hw = GEOMETRIES["3x3s2-same-7x9"]
    x = _images(np.int8, H, W, 8, 5)
    c0, c1 = R.pool_constants(0.05, 3, 0.07, -5)
    want = R.max_pool_2d(x, filt, strides, padding, out_hw, c0, c1, "none", 0.07, -5)
    op = mf.ops.prepare_max_pool_2d((H, W, 8), filt, 0.07, -5, mf.ops.MaxPool2DOptions(mf.FusedActivation(0), mf.TensorViewPadding(0), strides),
                                    (c0, c1), out_hw)
    buf = torch.zeros(x.size + 64, dtype=torch.int8, device="cuda")
    buf[1:1 + x.size].copy_(torch.as_tensor(x.reshape(-1)))
    out = torch.empty(want.size, dtype=torch.int8, device="cuda")
    assert (buf.data_ptr() + 1) % 16 == 1
    _lib.check(_lib.lib().mf_op_run(op._h, buf.data_ptr() + 1, BATCH, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    assert np.array_equal(out.cpu().numpy(), want.reshape(-1))


# ---- a LeNet written with max pools ---------------------------------------------------------------------------------------------
class LeNet:
    N = 6

    def __init__(self, O, elem):
        import microflow_rs_amd as mf
        import tflite_writer as tw
        shape, in_q, layers = tw.lenet_layers(np.random.default_rng(61 + elem), elem=elem, wzp_nonzero=True, pool="max")
        self.in_q = in_q
        self.blob = tw.build_model(shape, in_q, layers, elem)
        self.m = mf.Model(self.blob)
        self.m.prepare(1)
        self.dt = self.m.dtype
        lo = 0 if elem == U8 else -128
        self.x = np.random.default_rng(62).integers(lo, lo + 256, (self.N, self.m.input_elems), dtype=np.int16).astype(self.dt)
        self.x[0], self.x[1] = lo, lo + 255
        self.run = R.segments(tw, O, shape, in_q, layers, elem)
        self.layers = self.run(self.x)                       # every operator's expected output, computed once
        self.want = self.layers[-1]
        self.O = O


_lenets = {}


@pytest.fixture(params=[9, U8], ids=["i8", "u8"])
def lenet(request, O):
    if request.param not in _lenets:
        _lenets[request.param] = LeNet(O, request.param)
    return _lenets[request.param]


def _names(m):
    return [m.op(i)["kernel"] for i in range(m.num_ops)]


def test_lenet_kernels(lenet):
    """the first stage keeps two launches (one input channel: excluded by measurement; its pool has C = 6: byte-wise), the
    second is one conv_maxpool_rt launch; layer by layer its pool (C = 16) runs maxpool_c4; no average-pool group takes a max pool"""
    if ROUTING_SWITCHED:
        return
    m = lenet.m
    names = _names(m)
    assert [o["kind"] for o in m.ops] == [3, 17, 3, 17, 22, 9, 9, 9, 25]
    assert names[1] == "maxpool_generic" and names[2].startswith("conv_maxpool_rt<12x12x6-16;5x5;p2x2s2;G") and names[3] == FUSED, names
    assert not any(n.startswith(("conv_pool_rt<", "pool_fc_chain<", "avgpool_")) for n in names), names
    m.set_fusion(False)
    try:
        off = _names(m)
    finally:
        m.set_fusion(True)
    assert off[1] == "maxpool_generic" and off[3] == "maxpool_c4" and not off[2].startswith("conv_maxpool_rt"), off
    for o, n in zip(m.ops, off):
        if o["kind"] == 17 and o["in_shape"][3] % 4 == 0:
            assert not n.endswith("_generic"), off


def test_lenet_every_way_it_runs(lenet):
    m, n = lenet.m, lenet.N
    assert len(lenet.layers) == m.num_ops
    got = m.run_quantized(lenet.x).reshape(n, -1)
    assert np.array_equal(got, lenet.want), np.flatnonzero((got != lenet.want).any(axis=1))
    for i in range(m.num_ops):
        got = np.asarray(m.run_until(lenet.x, i)).reshape(n, -1)
        assert np.array_equal(got, lenet.layers[i]), (i, int((got != lenet.layers[i]).sum()))
    m.set_fusion(False)
    try:
        assert np.array_equal(m.run_quantized(lenet.x).reshape(n, -1), lenet.want)
    finally:
        m.set_fusion(True)
    m.set_generic(True)
    try:
        assert _names(m)[3] == "maxpool_generic"
        assert np.array_equal(m.run_quantized(lenet.x).reshape(n, -1), lenet.want)
        assert np.array_equal(np.asarray(m.run_until(lenet.x, 3)).reshape(n, -1), lenet.layers[3])
    finally:
        m.set_generic(False)


def test_lenet_graph_replay(lenet):
    import torch
    m, n = lenet.m, lenet.N
    x = torch.as_tensor(lenet.x).cuda()
    out = torch.empty((n, lenet.want.shape[1]), dtype=x.dtype, device="cuda")
    m.set_graph(True)
    try:
        before = m.graph_launches
        for it in range(4):                                  # eager, captured + replayed, replayed, replayed
            out.zero_()
            m.run_quantized(x, out=out)
            assert np.array_equal(out.cpu().numpy(), lenet.want), it
        assert m.graph_launches >= before + 2
    finally:
        m.set_graph(False)


def test_lenet_predict_bit_for_bit(lenet):
    """f32 in, f32 out: quantize (src/quantize.rs:16-18, the oracle's), the segments, dequantize scale * (f32(q) - f32(zp))"""
    m, O = lenet.m, lenet.O
    x = np.random.default_rng(63).uniform(-1.0, 1.0, (4,) + tuple(m.input_shape)).astype(np.float32)
    xq = O.quantize_array(x, lenet.in_q[0], lenet.in_q[1], lenet.dt).reshape(4, -1)
    q = lenet.run(xq)[-1]
    want = np.float32(m.output_scale) * (q.astype(np.float32) - np.float32(m.output_zero_point))
    got = m.predict(x).reshape(4, -1)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(m.predict_quantized(xq).reshape(4, -1).view(np.uint32), want.view(np.uint32))


# ---- what must not move: the average-pool models report the kernels they reported ------------------------------------------------
FUSED = "(fused into the previous operator)"


def test_average_pool_models_keep_their_kernels():
    """recorded from the parent commit"""
    import microflow_rs_amd as mf
    import tflite_writer as tw
    if ROUTING_SWITCHED:
        return
    rng = np.random.default_rng
    models = {
        "lenet": tw.lenet(rng(5)),
        "stage": tw.conv_pool(rng(7), (12, 12, 6), 16, 5),
        "stage-u8-pool3x3": tw.conv_pool(rng(8), (48, 48, 8), 96, 3, padding="same", pool=(3, 3), pool_padding="same", pool_q=0.8, elem=tw.UINT8,
                                         wzp_nonzero=True),
    }
    got = {}
    for k, blob in models.items():
        m = mf.Model(blob)
        m.prepare(1)
        got[k] = _names(m)
    assert got == PARENT_KERNELS, got


PARENT_KERNELS = {
    "lenet": ["conv_rows_lds", "avgpool_generic", "conv_pool_rt<12x12x6-16;5x5;p2x2s2;G16>", FUSED, "", "fc_chain<3>+sm", FUSED, FUSED, FUSED],
    "stage": ["conv_pool_rt<12x12x6-16;5x5;p2x2s2;G16>", FUSED],
    "stage-u8-pool3x3": ["conv_gemm_rt<wzp>", "avgpool_c4"],
}


# ---- Conv2D + MaxPool2D stages as one conv_maxpool_rt launch (k_conv_maxpool.hip) -------------------------------------------------
# one case per plan kind, at the smallest shapes of tests/test_gpu_conv_pool.py: (shape, N, K, conv_pool options, batch)
STAGES = {
    "b-12x12x6-16-5x5": ((12, 12, 6), 16, 5, dict(act="none", pool_q=0.9), 9),                       # G images per step; C % 4 != 0
    "w-16x16x32-64-3x3same": ((16, 16, 32), 64, 3, dict(padding="same", act="relu", pool_q=0.9, wmax=32), 9),
    "k-48x48x8-96-bands-pool3x3s2same": ((48, 48, 8), 96, 3, dict(padding="same", act="relu", pool=(3, 3), pool_padding="same", pool_q=0.8), 3),  # the shared row at the band edge
    "j-64x64x4-64-bands": ((64, 64, 4), 64, 3, dict(padding="same", act="relu", pool_q=0.9), 3),
}
RAGGED = 37


def _routed(shape, N, K):
    """the classes fused_conv_pool_create keeps for a MaxPool2D, restated"""
    return ROUTED_RULE(shape[2], N, K)


class MaxStage:
    def __init__(self, O, name, seed):
        import microflow_rs_amd as mf
        import tflite_writer as tw
        shape, N, K, kw, batch = STAGES[name]
        self.name, self.batch = name, batch
        rng = np.random.default_rng(seed)
        in_q = (float(np.float32(rng.uniform(0.02, 0.08))), int(rng.integers(-108, 108)))
        layers, _, _ = tw.conv_pool_layers(rng, shape, in_q, N, K, pool_op="max", **kw)
        self.blob = tw.build_model((1,) + shape, in_q, layers)
        self.m = mf.Model(self.blob)
        self.m.prepare(1)
        n = RAGGED if name[0] == "b" else batch
        self.x = np.random.default_rng(seed + 1).integers(-128, 128, (n, self.m.input_elems), dtype=np.int16).astype(np.int8)
        self.x[0], self.x[1] = -128, 127
        self.conv, self.want = R.segments(tw, O, (1,) + shape, in_q, layers, 9)(self.x)
        self.routed = _routed(shape, N, K) and name[0] not in "jk"       # (the band cases plan beyond 80 KiB)


_stages = {}


def _stage(O, name):
    if name not in _stages:
        _stages[name] = MaxStage(O, name, 300 + sorted(STAGES).index(name))
    return _stages[name]


@pytest.mark.parametrize("name", sorted(STAGES))
def test_stage_routing_and_bytes_every_way(O, name):
    """the default route shows conv_maxpool_rt< exactly for the classes DESIGN 4.19 lists; the bytes are the expected ones as one
    launch, with fusion off, shape-generic, up to the convolution alone, on a ragged batch and from an unaligned input pointer"""
    import torch
    st = _stage(O, name)
    m, n = st.m, st.batch
    names = _names(m)
    if not ROUTING_SWITCHED:
        if st.routed:
            assert names[0].startswith("conv_maxpool_rt<") and names[0].endswith(">") and names[1] == FUSED, names
        else:
            assert not names[0].startswith("conv_") or not names[0].startswith(("conv_maxpool_rt", "conv_pool_rt")), names
            assert names[1].startswith("maxpool_"), names
        assert not any(v.startswith("conv_pool_rt<") for v in names), names
    x, want = st.x[:n], st.want[:n]
    got = m.run_quantized(x).reshape(n, -1)
    assert np.array_equal(got, want), (int((got != want).sum()), np.flatnonzero((got != want).any(axis=1))[:8])
    assert np.array_equal(np.asarray(m.run_until(x, 0)).reshape(n, -1), st.conv[:n])
    m.set_fusion(False)
    try:
        if not ROUTING_SWITCHED:
            assert _names(m)[1] in ("maxpool_c4", "maxpool_generic") and not _names(m)[0].startswith("conv_maxpool_rt"), _names(m)
        assert np.array_equal(m.run_quantized(x).reshape(n, -1), want)
    finally:
        m.set_fusion(True)
    m.set_generic(True)
    try:
        assert np.array_equal(m.run_quantized(x).reshape(n, -1), want)
    finally:
        m.set_generic(False)
    if name[0] == "b":
        for k in (1, 15, 17, RAGGED):
            assert np.array_equal(m.run_quantized(st.x[:k]).reshape(k, -1), st.want[:k]), k
    flat = x.reshape(-1)
    buf = torch.zeros(flat.size + 64, dtype=torch.int8, device="cuda")
    view = buf[1:1 + flat.size]
    view.copy_(torch.as_tensor(flat))
    assert view.data_ptr() % 16 == 1                     # the group loads 16-byte words: such a pointer takes the operators' launches
    assert np.array_equal(m.run_quantized(view).cpu().numpy().reshape(n, -1), want)


_CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, %r)
import microflow_rs_amd as mf
d = np.load(sys.argv[1], allow_pickle=False)
for name in sys.argv[2:]:
    m = mf.Model(bytes(d["blob_" + name]))
    m.prepare(1)
    x, want = d["x_" + name], d["want_" + name]
    names = [m.op(i)["kernel"] for i in range(m.num_ops)]
    for n in [int(v) for v in d["batches_" + name]]:
        got = m.run_quantized(x[:n]).reshape(n, -1)
        assert np.array_equal(got, want[:n]), (name, n, int((got != want[:n]).sum()))
    n, size = len(x), want.size
    buf = torch.full((64 + size + 64,), 0x5A, dtype=torch.int8, device="cuda")
    m.run_quantized(torch.as_tensor(x).cuda(), out=buf[64:64 + size])
    b = buf.cpu().numpy()
    assert (b[:64] == 0x5A).all() and (b[64 + size:] == 0x5A).all() and np.array_equal(b[64:64 + size].reshape(n, -1), want), name
    print("OK", name, "|".join(names), flush=True)
''' % ROOT


def _child(O, env_extra):
    import subprocess
    import tempfile
    data = {}
    for name in sorted(STAGES):
        st = _stage(O, name)
        data["blob_" + name] = np.frombuffer(st.blob, np.uint8)
        data["x_" + name], data["want_" + name] = st.x, st.want
        data["batches_" + name] = np.array((1, 15, 17, RAGGED) if name[0] == "b" else (1, 2, st.batch))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cases.npz")
        np.savez(path, **data)
        env = {k: v for k, v in os.environ.items() if not k.startswith("MF_")}
        env.update(env_extra)
        r = subprocess.run([sys.executable, "-c", _CHILD, path] + sorted(STAGES), capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    ok = {l.split()[1]: l.split(" ", 2)[2].split("|") for l in r.stdout.splitlines() if l.startswith("OK ")}
    assert sorted(ok) == sorted(STAGES), sorted(ok)
    return ok


def test_every_plan_kind_runs_the_kernel_when_asked(O):
    """MF_DEV=1 MF_CONV_POOL_ALL=1 (a child process: the switches are read once per process): every case, the ones the route excludes
    by measurement too, is one conv_maxpool_rt launch with the expected bytes; ragged batches (G = 16: 1, 15, 17, 37; bands: 1, 2, 3);
    64 guard bytes around every output"""
    ok = _child(O, dict(MF_DEV="1", MF_CONV_POOL_ALL="1"))
    for name, names in ok.items():
        assert names[0].startswith("conv_maxpool_rt<") and names[1] == FUSED, (name, names)
    assert ";G16>" in ok["b-12x12x6-16-5x5"][0] and ";PB16;NB2>" in ok["j-64x64x4-64-bands"][0], ok
    assert ";PB12;NB2>" in ok["k-48x48x8-96-bands-pool3x3s2same"][0] and ";p3x3s2;" in ok["k-48x48x8-96-bands-pool3x3s2same"][0], ok


def test_no_conv_pool_switch_gives_the_two_launches_back(O):
    """MF_DEV=1 MF_NO_CONV_POOL=1: no group, the operators' own kernels, the same bytes"""
    ok = _child(O, dict(MF_DEV="1", MF_NO_CONV_POOL="1"))
    for name, names in ok.items():
        assert not names[0].startswith(("conv_maxpool_rt", "conv_pool_rt")) and names[1] in ("maxpool_c4", "maxpool_generic"), (name, names)


def ROUTED_RULE(C, N, K):
    """not with one input channel, fewer than 16 output channels or fewer than 2400 multiply-adds per output pixel (KH KW C N); nor
    with a plan beyond 80 KiB of LDS, which of STAGES the two band cases are (profiles/r17)"""
    return C != 1 and N >= 16 and K * K * C * N >= 2400
