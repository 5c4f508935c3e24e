"""conv_rows_bytes (k_rt.hip): one-channel Conv2D / DepthwiseConv2D whose image rows are not whole dwords (W % 4 != 0: 10 or 13
MFCCs, 43 mel bins) on conv_rows_lds's tile and compute loop behind a byte-granular staging.  Bit-exact against the CPU oracle and
against the shape-generic kernel, the bytes around input and output, the shapes that must keep their kernels, the DS-CNN keyword
spotter (tools/tflite_writer.ds_cnn) every way a model can be run, and the MF_NO_CONV_ROWS_BYTES switch."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests.conftest import ROOT, ROUTING_SWITCHED

pytestmark = pytest.mark.gpu
f32 = np.float32

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def mf():
    import torch
    assert torch.cuda.is_available()
    import microflow_rs_amd as m
    return m


def _consts(rng, n, taps):
    c0 = rng.uniform(-30, 30, n).astype(f32)
    return c0, (rng.uniform(0.5, 1.5, n) * 40.0 / (5476.0 * np.sqrt(taps))).astype(f32)


def _out_hw(H, W, KH, KW, sh, sw, pad):
    if pad == 0:
        return -(-H // sh), -(-W // sw)
    return (H - KH) // sh + 1, (W - KW) // sw + 1


def make(mf, O, rng, kind, H, W, C, N, KH, KW, sh, sw, pad, wz, u8):
    """the operator of tests/test_gpu_rt.py::test_conv_rows_vs_oracle: activation drawn from 0 / 1 / 3, input zero point over the
    whole range; returns it with the oracle of one image"""
    dt = np.uint8 if u8 else np.int8
    lo, hi = (0, 256) if u8 else (-128, 128)
    OH, OW = _out_hw(H, W, KH, KW, sh, sw, pad)
    izp, oscale, ozp, act = int(rng.integers(lo, hi)), 0.0235294122, int(rng.integers(lo, lo + 100)), int(rng.choice([0, 1, 3]))
    zp = (rng.integers(-25, 25, N) + (128 if u8 else 0)).astype(dt) if wz else np.full(N, 128 if u8 else 0, dt)
    c0, c1 = _consts(rng, N, KH * KW * C)
    if kind == "conv":
        f = rng.integers(lo, hi, (N, KH, KW, C)).astype(dt)
        opts = mf.ops.Conv2DOptions(mf.FusedActivation(act), mf.TensorViewPadding(pad), (sh, sw))
        op = mf.ops.prepare_conv_2d((H, W, C), f, zp, izp, oscale, ozp, opts, (c0, c1), (OH, OW))
        ref = lambda v: O.conv_2d(v, f, zp, izp, oscale, ozp, act, pad, (sh, sw), (OH, OW), c0, c1)  # noqa: E731
    else:
        w = rng.integers(lo, hi, (KH, KW, N)).astype(dt)
        opts = mf.ops.DepthwiseConv2DOptions(mf.FusedActivation(act), mf.TensorViewPadding(pad), (sh, sw))
        op = mf.ops.prepare_depthwise_conv_2d((H, W, C), w, zp, izp, oscale, ozp, opts, (c0, c1), (OH, OW))
        ref = lambda v: O.depthwise_conv_2d(v, w, zp, izp, oscale, ozp, act, pad, (sh, sw), (OH, OW), c0, c1)  # noqa: E731
    return op, ref


def inputs(rng, batch, H, W, C, u8):
    lo, hi = (0, 256) if u8 else (-128, 128)
    x = rng.integers(lo, hi, (batch, H, W, C)).astype(np.uint8 if u8 else np.int8)
    x[0] = hi - 1
    return x


def name_of(kind, wz):
    return ("dw_rows_lds" if kind == "dw" else "conv_rows_lds") + ("<bytes,wzp>" if wz else "<bytes>")


CASES = [
    # kind, H, W, N, KH, KW, sh, sw, pad (0 SAME / 1 VALID), batch
    ("conv", 5, 5, 4, 3, 3, 1, 1, 0, 11),         # odd image size: image bases take all four byte shifts; a ragged last step
    ("conv", 7, 3, 8, 3, 3, 1, 1, 0, 9),          # rows shorter than a dword
    ("conv", 9, 13, 12, 4, 13, 2, 1, 1, 6),       # a filter as wide as the image: four dword groups per window row
    ("conv", 49, 10, 64, 10, 4, 2, 2, 0, 9),      # the DS-CNN stem; N at the kernel's limit
    ("dw", 13, 11, 5, 5, 7, 1, 3, 0, 7),          # byte stores (N % 8 != 0); depthwise weights
    ("dw", 49, 13, 8, 10, 8, 2, 2, 0, 9),         # the 13-MFCC sibling of speech's first operator
    ("conv", 67, 63, 5, 3, 3, 1, 1, 0, 31),       # 7 images per step, odd bytes per step: step bases take all four shifts
    ("conv", 131, 129, 8, 3, 3, 2, 2, 0, 5),      # one image per step
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("wz", [False, True], ids=["nowzp", "wzp"])
@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
def test_operators_vs_oracle_and_generic(mf, O, case, wz, u8):
    kind, H, W, N, KH, KW, sh, sw, pad, batch = case
    rng = np.random.default_rng(hash(case) % (2 ** 32) + 2 * int(u8) + int(wz))
    op, ref = make(mf, O, rng, kind, H, W, 1, N, KH, KW, sh, sw, pad, wz, u8)
    assert ROUTING_SWITCHED or op.kernel == name_of(kind, wz), op.kernel
    x = inputs(rng, batch, H, W, 1, u8)
    want = np.stack([ref(v) for v in x])
    got = op(x)
    assert np.array_equal(got, want), (op.kernel, np.argwhere(got != want)[:5])
    op.set_generic(True)
    assert ROUTING_SWITCHED or op.kernel.endswith("_generic"), op.kernel
    assert np.array_equal(op(x), want)


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[6]], ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
def test_neighbours_of_input_and_output(mf, O, case, u8):
    """the batch inside a larger device buffer filled with the type's extreme value, at 16-byte-aligned offsets (the fast path's
    contract), the output inside a sentinel-filled buffer: the plain call's bytes, and the sentinel intact around the output"""
    import torch
    from microflow_rs_amd import _lib
    kind, H, W, N, KH, KW, sh, sw, pad, batch = case
    rng = np.random.default_rng(5 + int(u8))
    op, ref = make(mf, O, rng, kind, H, W, 1, N, KH, KW, sh, sw, pad, True, u8)
    assert ROUTING_SWITCHED or op.kernel == name_of(kind, True), op.kernel
    OH, OW = _out_hw(H, W, KH, KW, sh, sw, pad)
    xn = inputs(rng, batch, H, W, 1, u8)
    tdt = torch.uint8 if u8 else torch.int8
    want = op(xn).reshape(-1)
    assert np.array_equal(want.reshape(batch, OH, OW, N)[batch - 1], ref(xn[batch - 1]))
    nin, n = xn.size, want.size
    for extreme in ((255, 0) if u8 else (127, -128)):
        for ioff, ooff in ((16, 16), (48, 32)):
            src = torch.full((ioff + nin + 4096,), extreme, dtype=tdt, device="cuda")
            src[ioff:ioff + nin] = torch.as_tensor(xn.reshape(-1)).cuda()
            buf = torch.full((ooff + n + 4096,), 0x5A, dtype=tdt, device="cuda")
            stream = torch.cuda.current_stream().cuda_stream
            _lib.check(_lib.lib().mf_op_run(op._h, src.data_ptr() + ioff, batch, buf.data_ptr() + ooff, stream))
            b = buf.cpu().numpy()
            assert (b[:ooff] == 0x5A).all() and (b[ooff + n:] == 0x5A).all(), (extreme, ioff, ooff)
            assert np.array_equal(b[ooff:ooff + n], want), (extreme, ioff, ooff)


def test_shapes_outside_the_route_keep_their_kernels(mf, O):
    """rows that are not whole dwords with three channels, more than 64 outputs, a window row of more than 64 bytes: the generic
    kernels, as before; whole-dword rows: plain conv_rows_lds"""
    rng = np.random.default_rng(77)
    kept = [(("conv", 6, 7, 3, 5, 3, 3, 1, 1, 0), "conv2d_generic"), (("dw", 31, 31, 1, 80, 5, 5, 1, 1, 0), "dwconv_generic"),
            (("conv", 12, 10, 1, 8, 3, 65, 1, 1, 0), "conv2d_generic"), (("conv", 49, 12, 1, 64, 10, 4, 2, 2, 0), "conv_rows_lds")]
    for (kind, H, W, C, N, KH, KW, sh, sw, pad), want_kernel in kept:
        op, ref = make(mf, O, rng, kind, H, W, C, N, KH, KW, sh, sw, pad, False, False)
        assert ROUTING_SWITCHED or op.kernel == want_kernel, (kind, H, W, C, N, op.kernel)
        x = inputs(rng, 3, H, W, C, False)
        assert np.array_equal(op(x), np.stack([ref(v) for v in x])), (kind, H, W, C, N)


# ---- the DS-CNN keyword spotter ---------------------------------------------------------------------------------------------------
class Net:
    def __init__(self, O, mf, u8, **kw):
        import tflite_writer as tw
        rng = np.random.default_rng(41 + int(u8))
        self.blob = tw.ds_cnn(rng, elem=tw.UINT8 if u8 else tw.INT8, wzp_nonzero=u8, **kw)
        self.m = mf.Model(self.blob)
        self.m.prepare(1)
        self.om = O.Model(self.blob)
        self.lo, self.hi = (0, 256) if u8 else (-128, 128)
        self.x = rng.integers(self.lo, self.hi, (9, self.m.input_elems), dtype=np.int16).astype(self.m.dtype)
        self.x[0], self.x[1] = self.lo, self.hi - 1
        self.names = [self.m.op(i)["kernel"] for i in range(self.m.num_ops)]


_nets = {}


@pytest.fixture(params=[False, True], ids=["i8", "u8-wzp"])
def net(request, O, mf):
    if request.param not in _nets:
        _nets[request.param] = Net(O, mf, request.param)
    return _nets[request.param]


def test_ds_cnn_against_the_oracle_every_way_it_runs(net):
    import torch
    m = net.m
    want = net.om.run_quantized_batch(net.x).reshape(9, -1)
    if not ROUTING_SWITCHED:
        assert net.names[0] == "conv_rows_lds<bytes" + (",wzp>" if m.dtype == np.uint8 else ">"), net.names
        assert not any(n.endswith("_generic") for n in net.names), net.names
    assert np.array_equal(m.run_quantized(net.x).reshape(9, -1), want)
    _, layers = net.om.run_quantized(net.x[2], layers=True)
    for i in range(m.num_ops):
        assert np.array_equal(np.asarray(m.run_until(net.x[2:3], i)).reshape(-1), layers[i].reshape(-1)), i
    m.set_fusion(False)
    try:
        off = [m.op(i)["kernel"] for i in range(m.num_ops)]
        assert ROUTING_SWITCHED or off[0] == net.names[0], off
        assert np.array_equal(m.run_quantized(net.x).reshape(9, -1), want)
    finally:
        m.set_fusion(True)
    m.set_generic(True)
    try:
        assert np.array_equal(m.run_quantized(net.x).reshape(9, -1), want)
    finally:
        m.set_generic(False)
    x = torch.as_tensor(net.x).cuda()
    ref = m.run_quantized(x).clone()
    assert np.array_equal(ref.cpu().numpy().reshape(9, -1), want)
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


def _predict_check(nt):
    """predict on f32 input: the oracle's floats bit for bit, and exactly one launch more than run_quantized of the same handle -- the
    separate quantise pass (conv_rows_bytes has no f32 entry)"""
    import torch
    m = nt.m
    rng = np.random.default_rng(23)
    q = rng.integers(nt.lo, nt.hi, (3, m.input_elems)).astype(np.float32)
    x = ((q - np.float32(m.input_zero_point)) * np.float32(m.input_scale) + rng.uniform(-0.4, 0.4, q.shape).astype(np.float32) * np.float32(m.input_scale)).astype(np.float32)
    want = np.stack([nt.om.predict(x[i].reshape(m.input_shape)).reshape(-1) for i in range(3)]).astype(np.float32)
    xd = torch.as_tensor(x.reshape((3,) + tuple(m.input_shape))).cuda()
    got = m.predict(xd).cpu().numpy().reshape(3, -1).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if ROUTING_SWITCHED:
        return
    xq = torch.as_tensor(nt.x[:3]).cuda()
    outq = torch.empty((3, m.output_elems), dtype=torch.uint8 if m.dtype == np.uint8 else torch.int8, device="cuda")
    outf = torch.empty((3, m.output_elems), dtype=torch.float32, device="cuda")
    m.run_quantized(xq, out=outq)
    before = m.device_ops()
    m.run_quantized(xq, out=outq)
    quantized = m.device_ops() - before
    m.predict(xd, out=outf)
    before = m.device_ops()
    m.predict(xd, out=outf)
    # (a u8 handle's run_quantized carries two passes predict does not have: u8 -> the internal i8 domain in front and back behind)
    launches = quantized - (2 if m.dtype == np.uint8 else 0)
    assert m.device_ops() - before == launches + 1, (m.device_ops() - before, quantized)


def test_ds_cnn_predict_keeps_the_separate_quantise_pass(net):
    _predict_check(net)


def test_one_image_per_step_stem_has_no_f32_entry(O, mf):
    """131 x 129 x 1: one image per step, where conv_rows_lds takes the floats itself; conv_rows_bytes does not
    (16 filters: the head is the pool + FullyConnected + Softmax launch that writes the floats, as in the 49 x 10 model)"""
    if "big" not in _nets:
        _nets["big"] = Net(O, mf, False, shape=(131, 129), filters=16, blocks=1, classes=4, stem=(3, 3, (2, 2)))
    nt = _nets["big"]
    assert ROUTING_SWITCHED or nt.names[0] == "conv_rows_lds<bytes>", nt.names
    _predict_check(nt)


def test_switch_gives_the_generic_kernels_back():
    """MF_DEV=1 MF_NO_CONV_ROWS_BYTES=1 in a child process (the switches are read once per process): the same bytes, and only the
    operators this route takes change their names -- to *_generic"""
    code = r'''
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import microflow_rs_amd as mf
import tflite_writer as tw
from tests.test_gpu_conv_rows_bytes import CASES, make, inputs
O = None                                               # (the operators' oracles are not called here)
outs, names = [], []
for case in CASES[:6]:
    kind, H, W, N, KH, KW, sh, sw, pad, batch = case
    rng = np.random.default_rng(3)
    op, _ = make(mf, O, rng, kind, H, W, 1, N, KH, KW, sh, sw, pad, True, False)
    names.append(op.kernel)
    outs.append(op(inputs(rng, batch, H, W, 1, False)).reshape(-1))
rng = np.random.default_rng(3)
op, _ = make(mf, O, rng, "conv", 49, 12, 1, 64, 10, 4, 2, 2, 0, False, False)
names.append(op.kernel)
outs.append(op(inputs(rng, 9, 49, 12, 1, False)).reshape(-1))
m = mf.Model(tw.ds_cnn(np.random.default_rng(9)))
m.prepare(1)
names += [m.op(i)["kernel"] for i in range(m.num_ops)]
x = np.random.default_rng(6).integers(-128, 128, (9, m.input_elems)).astype(np.int8)
outs.append(m.run_quantized(x).reshape(-1))
print("KERNELS", "|".join(names))
np.save(sys.argv[1], np.concatenate(outs))
''' % (ROOT, os.path.join(ROOT, "tools"))
    outs, kernels = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for sw in ({}, dict(MF_DEV="1", MF_NO_CONV_ROWS_BYTES="1")):
            env = dict(os.environ)
            for k in [k for k in env if k.startswith("MF_")]:
                del env[k]
            env.update(sw)
            path = os.path.join(tmp, "out%d.npy" % len(outs))
            r = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
            assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
            kernels.append([l.split(" ", 1)[1].split("|") for l in r.stdout.splitlines() if l.startswith("KERNELS")][0])
            outs.append(np.load(path))
    assert np.array_equal(outs[0], outs[1])
    on, off = kernels
    moved = [i for i in range(len(on)) if on[i] != off[i]]
    assert moved == [0, 1, 2, 3, 4, 5, 7], (on, off)                # the six operators and the model's stem; not 49 x 12
    assert all("_rows_lds<bytes" in on[i] and off[i].endswith("_generic") for i in moved), (on, off)
    assert on[6] == "conv_rows_lds"
