"""The ADD operator on the device against its contract restated in numpy (tests/add_ref.py): every one of the 65 536 (a, b) pairs for
four quantisations x three activations x both element types, under both operand orders and on both kernels; sizes around the
16-byte group with guard bytes on either side of the output; unaligned pointers, in place on either operand, and the refused calls."""
import numpy as np
import pytest

from tests import add_ref as A
from tests.conftest import ROUTING_SWITCHED

pytestmark = pytest.mark.gpu

ACTS = ("none", "relu", "relu6")
# (a, b, output) as (scale, zero point) of an i8 tensor; u8 moves every zero point by 128
QUANTS = {
    "equal": ((0.05, 3), (0.05, 3), (0.05, 3)),            # ca = cb = 1: a + b - z
    "halves": ((0.05, 3), (0.05, -7), (0.1, -5)),          # ca = cb = 0.5 exactly: every odd difference a tie, both signs
    "unequal": ((0.05, 3), (0.031, -7), (0.07, -5)),
    "saturating": ((0.1, 3), (0.1, -7), (0.02, -5)),       # ca = cb = 5: most pairs leave T's range
}


def _quants(name, dt):
    off = 128 if dt == np.uint8 else 0
    return tuple((s, z + off) for s, z in QUANTS[name])


def _options(act):
    from microflow_rs_amd import ops
    from microflow_rs_amd.tensor import FusedActivation
    return ops.AddOptions({"none": FusedActivation.NONE, "relu": FusedActivation.RELU, "relu6": FusedActivation.RELU6}[act])


def _all_pairs(dt):
    lo = 0 if dt == np.uint8 else -128
    vals = (np.arange(256) + lo).astype(dt)
    a = np.repeat(vals[:, None], 256, axis=1).reshape(256, 4, 4, 16)   # image i: its byte everywhere
    b = np.tile(vals[None, :], (256, 1)).reshape(256, 4, 4, 16)        # every image: all 256 values
    return a, b


@pytest.mark.parametrize("dt", [np.int8, np.uint8], ids=["i8", "u8"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("name", list(QUANTS))
def test_all_65536_pairs(name, act, dt):
    from microflow_rs_amd import ops
    qa, qb, qo = _quants(name, dt)
    a, b = _all_pairs(dt)
    want = A.add(a, b, qa, qb, qo, act)
    if name == "equal" and act == "none":   # the closed form
        lo, hi = (0, 255) if dt == np.uint8 else (-128, 127)
        assert np.array_equal(want, np.clip(a.astype(np.int32) + b.astype(np.int32) - qo[1], lo, hi).astype(dt))
    op = ops.prepare_add((4, 4, 16), qa, qb, qo, _options(act), dtype=dt)
    if not ROUTING_SWITCHED:
        assert op.kernel in ("add_c16", "add_c16<fma>")
    got = op(a, b)
    assert got.dtype == dt and got.shape == want.shape
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    op.set_generic(True)
    assert op.kernel == "add_generic"
    gen = op(a, b)
    op.set_generic(False)
    assert np.array_equal(gen, want), int((gen != want).sum())
    # the other operand order: its own operator, its own expected bytes (the f32 sum is not commutative)
    want_r = A.add(b, a, qb, qa, qo, act)
    op_r = ops.prepare_add((4, 4, 16), qb, qa, qo, _options(act), dtype=dt)
    got_r = op_r(b, a)
    assert np.array_equal(got_r, want_r), int((got_r != want_r).sum())
    op_r.set_generic(True)
    assert np.array_equal(op_r(b, a), want_r)


def _run2(op, a, b, out, batch):
    import torch
    from microflow_rs_amd import _lib
    st = _lib.lib().mf_op_run2(op._h, a.data_ptr(), b.data_ptr(), batch, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


GUARD = 64


@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("elems", [1, 3, 4, 15, 16, 17, 20, 48, 1000])
def test_sizes_and_guard_bytes(elems, batch):
    import torch
    from microflow_rs_amd import _lib, ops
    qa, qb, qo = QUANTS["unequal"]
    rng = np.random.default_rng(elems * 7 + batch)
    n = elems * batch
    a = rng.integers(-128, 128, (batch, elems)).astype(np.int8)
    b = rng.integers(-128, 128, (batch, elems)).astype(np.int8)
    want = A.add(a, b, qa, qb, qo, "relu")
    op = ops.prepare_add(elems, qa, qb, qo, _options("relu"))
    if not ROUTING_SWITCHED:
        assert op.kernel in ("add_c16", "add_c16<fma>")
    ta, tb = torch.as_tensor(a).cuda(), torch.as_tensor(b).cuda()
    buf = torch.full((GUARD + n + GUARD,), 0x5A, dtype=torch.int8, device="cuda")
    out = buf[GUARD:GUARD + n]
    assert ta.data_ptr() % 16 == 0 and tb.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    for generic in (False, True):
        buf.fill_(0x5A)
        op.set_generic(generic)
        assert _run2(op, ta, tb, out, batch) == _lib.MF_OK
        host = buf.cpu().numpy()
        assert np.array_equal(host[GUARD:GUARD + n].reshape(batch, elems), want), (generic, elems, batch)
        assert (host[:GUARD] == 0x5A).all() and (host[GUARD + n:] == 0x5A).all(), (generic, elems, batch)


def test_pointers_in_place_and_refused_calls():
    import torch
    from microflow_rs_amd import _lib, ops
    from microflow_rs_amd.ops import AveragePool2DOptions
    qa, qb, qo = QUANTS["unequal"]
    elems, batch = 1000, 3
    n = elems * batch
    rng = np.random.default_rng(5)
    a = rng.integers(-128, 128, n).astype(np.int8)
    b = rng.integers(-128, 128, n).astype(np.int8)
    want = A.add(a, b, qa, qb, qo, "none")
    op = ops.prepare_add(elems, qa, qb, qo, _options("none"))

    def staged(x, off):
        t = torch.zeros(n + 32, dtype=torch.int8, device="cuda")
        assert t.data_ptr() % 16 == 0
        t[off:off + n] = torch.as_tensor(x).cuda()
        return t[off:off + n]

    # a pointer one byte off a 16-byte boundary, on each of a, b and the output in turn
    for offs in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        ta, tb, out = staged(a, offs[0]), staged(b, offs[1]), staged(np.zeros(n, np.int8), offs[2])
        assert _run2(op, ta, tb, out, batch) == _lib.MF_OK
        assert np.array_equal(out.cpu().numpy(), want), offs
    # in place on a, in place on b (aligned and not)
    for off in (0, 1):
        ta, tb = staged(a, off), staged(b, off)
        assert _run2(op, ta, tb, ta, batch) == _lib.MF_OK
        assert np.array_equal(ta.cpu().numpy(), want) and np.array_equal(tb.cpu().numpy(), b)
        ta = staged(a, off)
        assert _run2(op, ta, tb, tb, batch) == _lib.MF_OK
        assert np.array_equal(tb.cpu().numpy(), want) and np.array_equal(ta.cpu().numpy(), a)
    # a partial overlap of the output with either input is refused, and nothing is written
    big = torch.zeros(2 * n, dtype=torch.int8, device="cuda")
    tb = staged(b, 0)
    for shift in (16, 1, n - 1):
        assert _run2(op, big[:n], tb, big[shift:shift + n], batch) == _lib.MF_ERR_INVALID_ARG
        assert _run2(op, tb, big[shift:shift + n], big[:n], batch) == _lib.MF_ERR_INVALID_ARG
    assert int(big.count_nonzero()) == 0
    # one input through mf_op_run on an ADD, two through mf_op_run2 on a pool
    stream = torch.cuda.current_stream().cuda_stream
    assert _lib.lib().mf_op_run(op._h, tb.data_ptr(), batch, big.data_ptr(), stream) == _lib.MF_ERR_INVALID_ARG
    pool = ops.prepare_average_pool_2d((4, 4, 4), (2, 2), 0.05, 0, AveragePool2DOptions(strides=(2, 2)), (1.0, 0.0), (2, 2))
    x = torch.zeros(64, dtype=torch.int8, device="cuda")
    assert _run2(pool, x, x, big, 1) == _lib.MF_ERR_INVALID_ARG
    with pytest.raises(TypeError):
        op(a.reshape(batch, elems))
    with pytest.raises(TypeError):
        pool(x.reshape(1, 4, 4, 4), x.reshape(1, 4, 4, 4))


def test_the_python_surface():
    from microflow_rs_amd import ops
    from microflow_rs_amd.tensor import Tensor4D
    qa, qb, qo = _quants("unequal", np.uint8)
    rng = np.random.default_rng(9)
    a = rng.integers(0, 256, (2, 3, 5, 7)).astype(np.uint8)
    b = rng.integers(0, 256, (2, 3, 5, 7)).astype(np.uint8)
    y = ops.add(Tensor4D(a, [qa[0]], [qa[1]]), Tensor4D(b, [qb[0]], [qb[1]]), [qo[0]], [qo[1]], _options("relu6"), ops.preprocess_add(qa[0], qb[0], qo[0]))
    assert isinstance(y, Tensor4D) and np.array_equal(y.buffer, A.add(a, b, qa, qb, qo, "relu6"))
    assert ops.preprocess_add(qa[0], qb[0], qo[0]) == A.constants(qa[0], qb[0], qo[0])
