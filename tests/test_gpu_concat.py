"""The CONCATENATION operator on the device against its contract restated in numpy (tests/concat_ref.py): shapes that take the byte
kernel, dword words (where the sizes force them although one is a multiple of 16), 8- and 16-byte words, and a slice far wider than
the other; four batches, both element types, slices that are copied and slices that are requantised, inputs in which all 256 byte
values occur; concat_c4 against concat_generic against the reference, with guard bytes on either side of the output; pointers off
the 16-byte boundary; and the refused calls."""
import numpy as np
import pytest

from tests import concat_ref as CR
from tests.conftest import ROUTING_SWITCHED

pytestmark = pytest.mark.gpu

# (rows, Ca, Cb) -> the kernel that runs on 16-byte aligned pointers
SHAPES = {
    (1, 1, 1): "concat_generic",
    (7, 3, 5): "concat_generic",
    (3, 4, 12): "concat_c4",            # dwords
    (5, 16, 20): "concat_c4",           # dwords, although Ca is a multiple of 16
    (2, 8, 24): "concat_c4<v8>",
    (5, 16, 48): "concat_c4<v16>",
    (49, 64, 64): "concat_c4<v16>",     # a 7x7 fire output
    (4, 256, 16): "concat_c4<v16>",     # one slice far wider than the other
}
BATCHES = (1, 3, 67, 300)
# (a, b, output) as (scale, zero point) of an i8 tensor; u8 moves every zero point by 128.  Unequal scales: ratios in [0.4, 1.5], |z| <= 20
QUANTS = {
    "identity": ((0.05, 3), (0.05, 3), (0.05, 3)),                  # both slices are copies
    "a-only": ((0.03, -7), (0.05, 3), (0.05, 3)),                   # ca = 0.6
    "b-only": ((0.05, 3), (0.075, 12), (0.05, 3)),                  # cb = 1.5: about two thirds of uniform bytes stay inside the range
    "both": ((0.031, -20), (0.07, 20), (0.05, -5)),                 # 0.62 and 1.4
    "ties": ((0.03125, 5), (0.09375, -9), (0.0625, 1)),             # exactly 0.5 and 1.5: every odd difference is a tie
}
GUARD = 64


def _quants(name, dt):
    off = 128 if dt == np.uint8 else 0
    return tuple((s, z + off) for s, z in QUANTS[name])


def _inputs(shape, dt, seed):
    """[300, rows, Ca] and [300, rows, Cb]: random bytes, every one of the 256 values at the front of each"""
    rows, Ca, Cb = shape
    lo = 0 if dt == np.uint8 else -128
    rng = np.random.default_rng(seed)
    out = []
    for Cc in (Ca, Cb):
        t = rng.integers(lo, lo + 256, (BATCHES[-1], rows, Cc), dtype=np.int16)
        t.reshape(-1)[:256] = np.arange(256) + lo
        out.append(t.astype(dt))
    for t in out:
        assert len(np.unique(t)) == 256
    return out


def _run2(op, a, b, out, batch):
    import torch
    from microflow_rs_amd import _lib
    st = _lib.lib().mf_op_run2(op._h, a.data_ptr(), b.data_ptr(), batch, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("dt", [np.int8, np.uint8], ids=["i8", "u8"])
@pytest.mark.parametrize("name", list(QUANTS))
@pytest.mark.parametrize("shape", list(SHAPES), ids=["x".join(str(v) for v in s) for s in SHAPES])
def test_concat_c4_against_concat_generic_against_the_reference(shape, name, dt):
    import torch
    from microflow_rs_amd import _lib, ops
    rows, Ca, Cb = shape
    qa, qb, qo = _quants(name, dt)
    a, b = _inputs(shape, dt, 100 * rows + Ca + Cb)
    want = CR.concat(a, b, qa, qb, qo)
    lo, hi = (0, 255) if dt == np.uint8 else (-128, 127)
    # the reference alone: a copied slice is its input; at least half of a requantised slice lies strictly inside T's range
    for sl, x, qi in ((want[..., :Ca], a, qa), (want[..., Ca:], b, qb)):
        if np.float32(qi[0]) == np.float32(qo[0]) and qi[1] == qo[1]:
            assert np.array_equal(sl, x)
        else:
            assert np.mean((sl.astype(np.int32) > lo) & (sl.astype(np.int32) < hi)) >= 0.5
    op = ops.prepare_concatenation(rows, Ca, Cb, qa, qb, qo, dtype=dt)
    assert (op.in_tail, op.in2_tail, op.out_tail) == ((rows, Ca), (rows, Cb), (rows, Ca + Cb))
    L = _lib.lib()
    assert (L.mf_op_input_elems(op._h), L.mf_op_input2_elems(op._h), L.mf_op_output_elems(op._h)) == (rows * Ca, rows * Cb, rows * (Ca + Cb))
    if not ROUTING_SWITCHED:
        assert op.kernel == SHAPES[shape]
    ta, tb = torch.as_tensor(a).cuda(), torch.as_tensor(b).cuda()
    tdt = torch.uint8 if dt == np.uint8 else torch.int8
    for batch in BATCHES:
        n = batch * rows * (Ca + Cb)
        buf = torch.full((GUARD + n + GUARD,), 0x5A, dtype=tdt, device="cuda")
        out = buf[GUARD:GUARD + n]
        assert ta.data_ptr() % 16 == 0 and tb.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
        for generic in (False, True):
            buf.fill_(0x5A)
            op.set_generic(generic)
            assert op.kernel == ("concat_generic" if generic else SHAPES[shape]) or ROUTING_SWITCHED
            assert _run2(op, ta, tb, out, batch) == _lib.MF_OK
            host = buf.cpu().numpy()
            got = host[GUARD:GUARD + n].reshape(batch, rows, Ca + Cb)
            bad = np.argwhere(got != want[:batch])
            assert bad.shape[0] == 0, (generic, batch, int(bad.shape[0]), bad[:6].tolist())
            assert (host[:GUARD] == 0x5A).all() and (host[GUARD + n:] == 0x5A).all(), (generic, batch)
        op.set_generic(False)


@pytest.mark.parametrize("shape", [(7, 3, 5), (5, 16, 48), (4, 256, 16)], ids=["7x3x5", "5x16x48", "4x256x16"])
def test_pointers_off_the_boundary_overlap_and_refused_calls(shape):
    import torch
    from microflow_rs_amd import _lib, ops
    rows, Ca, Cb = shape
    qa, qb, qo = QUANTS["both"]
    batch = 3
    a, b = (t[:batch] for t in _inputs(shape, np.int8, 5))
    want = CR.concat(a, b, qa, qb, qo).reshape(-1)
    na, nb, no = a.size, b.size, want.size
    op = ops.prepare_concatenation(rows, Ca, Cb, qa, qb, qo)

    def staged(x, off, n):
        t = torch.zeros(n + 32, dtype=torch.int8, device="cuda")
        assert t.data_ptr() % 16 == 0
        if x is not None:
            t[off:off + n] = torch.as_tensor(x.reshape(-1)).cuda()
        return t[off:off + n]

    # base pointers one byte off a 16-byte boundary (the byte kernel), and 4 and 8 bytes off (narrower words), on each of a, b and
    # the output in turn; the generic route on every one of them
    for offs in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (4, 4, 4), (8, 8, 8), (4, 0, 8), (0, 8, 0)):
        for generic in (False, True):
            op.set_generic(generic)
            ta, tb, out = staged(a, offs[0], na), staged(b, offs[1], nb), staged(None, offs[2], no)
            assert _run2(op, ta, tb, out, batch) == _lib.MF_OK
            assert np.array_equal(out.cpu().numpy(), want), (offs, generic)
    op.set_generic(False)
    # any overlap of the output with an input is refused -- the pitches differ: nothing can be done in place -- and nothing is written
    big = torch.zeros(3 * no, dtype=torch.int8, device="cuda")
    ta, tb = staged(a, 0, na), staged(b, 0, nb)
    for shift in (0, 16, 1, na - 1):
        assert _run2(op, big[shift:shift + na], tb, big[:no], batch) == _lib.MF_ERR_INVALID_ARG
    for shift in (0, 16, 1, nb - 1, no - 1):
        assert _run2(op, ta, big[shift:shift + nb], big[:no], batch) == _lib.MF_ERR_INVALID_ARG
    assert _run2(op, big[no:no + na], tb, big[:no], batch) == _lib.MF_OK          # directly behind the output: no overlap
    assert int(big[no:].count_nonzero()) == 0
    # one input through mf_op_run on a CONCATENATION
    stream = torch.cuda.current_stream().cuda_stream
    assert _lib.lib().mf_op_run(op._h, tb.data_ptr(), batch, big.data_ptr(), stream) == _lib.MF_ERR_INVALID_ARG
    with pytest.raises(TypeError):
        op(a)
    with pytest.raises(ValueError):
        op(a, b[:2])


def test_the_python_surface():
    from microflow_rs_amd import ops
    from microflow_rs_amd.tensor import Tensor2D, Tensor4D
    qa, qb, qo = _quants("both", np.uint8)
    rng = np.random.default_rng(9)
    a = rng.integers(0, 256, (2, 3, 5, 8)).astype(np.uint8)
    b = rng.integers(0, 256, (2, 3, 5, 4)).astype(np.uint8)
    y = ops.concatenation(Tensor4D(a, [qa[0]], [qa[1]]), Tensor4D(b, [qb[0]], [qb[1]]), [qo[0]], [qo[1]], ops.ConcatenationOptions(axis=3),
                          ops.preprocess_concatenation(qa[0], qb[0], qo[0]))
    assert isinstance(y, Tensor4D) and y.buffer.shape == (2, 3, 5, 12) and np.array_equal(y.buffer, CR.concat(a, b, qa, qb, qo))
    y = ops.concatenation(Tensor2D(a[0, 0], [qa[0]], [qa[1]]), Tensor2D(b[0, 0], [qb[0]], [qb[1]]), [qo[0]], [qo[1]])
    assert isinstance(y, Tensor2D) and np.array_equal(y.buffer, CR.concat(a[0, 0], b[0, 0], qa, qb, qo))
    with pytest.raises(ValueError):
        ops.concatenation(Tensor4D(a, [qa[0]], [qa[1]]), Tensor4D(b, [qb[0]], [qb[1]]), [qo[0]], [qo[1]], ops.ConcatenationOptions(axis=1))
