"""conv_stream_rt (k_conv_stream.hip), selected per launch by the row count: bit-exact against conv2d_generic and the CPU oracle at a
ragged row count just above the threshold; the bytes around the output; the labels; the refusals."""
import numpy as np
import pytest

from tests.conftest import ROUTING_SWITCHED
from tests.test_gpu_conv_gemm import _inputs, _out_hw, check, make_conv, mf  # noqa: F401  (mf: the module fixture)

pytestmark = pytest.mark.gpu

# H, W, C, N, K, stride, SAME, rows the launch must at least have (0: the threshold; 49 152: the 256 x 256 tile), extreme operands
# (under a routing switch -- scripts/switch_matrix.sh -- the selection assertions are skipped and the parity checks run on what launches)
CASES = [(3, 3, 128, 128, 3, 1, True, 0, False),      # one k step per tap; OH OW = 9 never divides a tile
         (5, 4, 256, 128, 3, 2, True, 0, False),      # two k steps per tap, odd H at stride 2
         (4, 4, 128, 256, 3, 1, False, 49152, False),  # no padded tap, the 256-column tile
         (3, 3, 256, 128, 1, 1, True, 0, False),      # a plain GEMM on X
         (4, 4, 128, 128, 1, 2, True, 0, False),
         (2, 2, 1024, 128, 3, 1, True, 0, False),     # K' > 8192 (conv2d_generic today), every window mostly padding
         (4, 4, 512, 512, 3, 1, True, 0, True),       # |acc| up to 4608 x 255 x 128: epilogue mode 0
         (4, 4, 256, 1024, 1, 1, True, 8128, False)]  # 64 x 8 tiles of 128: the XCD-aware tile order (511 images, M = 8176)


def stream_batch(op, OHW, floor=0):
    """images of the first power-of-two row count >= 64 (and >= floor) at which a launch runs conv_stream_rt; None: none up to 65 536"""
    for rows in (64 << i for i in range(11)):
        batch = -(-max(rows, floor) // OHW)
        if op.kernel_at(batch).startswith("conv_stream_rt"):
            return batch
    return None


@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d-N%d-%dx%ds%d%s" % (c[:5] + c[4:6] + ("S" if c[6] else "V",)))
def test_conv_stream_vs_oracle_and_generic(mf, O, case, u8):
    H, W, C, N, K, s, same, floor, extreme = case
    rng = np.random.default_rng(abs(hash(case)) % (2 ** 32) + int(u8))
    lo, hi = (0, 256) if u8 else (-128, 128)
    f = None
    if extreme:                                        # the filter and inputs of test_conv_gemm_accumulators_beyond_2_25
        f = rng.integers(lo, hi, (N, K, K, C)).astype(np.uint8 if u8 else np.int8)
        f[0], f[1] = lo, hi - 1
        f[2, :, :, ::2], f[2, :, :, 1::2] = lo, hi - 1
    op, ref = make_conv(mf, O, rng, H, W, C, N, K, K, s, s, same, False, 0 if extreme else 1, u8, f=f, izp=lo if extreme else None)
    OH, OW = _out_hw(H, W, K, K, s, s, same)
    batch = stream_batch(op, OH * OW, floor)
    assert ROUTING_SWITCHED or batch is not None, op.kernel
    batch = (batch or 456) + 3                         # a ragged M whose last image straddles a tile
    M = batch * OH * OW
    name = op.kernel_at(batch)
    tile = int(name[len("conv_stream_rt<"):-1]) if name.startswith("conv_stream_rt<") else 128
    assert M % 128 and (ROUTING_SWITCHED or tile == {0: tile, 49152: 256, 8128: 128}[floor]), (M, name)
    assert ROUTING_SWITCHED or floor != 8128 or (-(-M // 128)) % 8 == 0   # (whole 8 x 8 patches of tiles)
    x = _inputs(rng, batch, H, W, C, u8)
    if extreme:
        x[1] = lo
    straddle = [i for i in range(batch) if i * OH * OW // tile != ((i + 1) * OH * OW - 1) // tile]
    straddle = straddle or [tile // (OH * OW) - 1, tile // (OH * OW)]   # (OH OW divides the tile: the images either side of a tile border)
    check(op, ref, x, [0, 1, straddle[0], straddle[-1], batch - 1])


def test_conv_stream_leaves_the_bytes_around_the_output(mf, O):
    import torch
    from microflow_rs_amd import _lib
    rng = np.random.default_rng(9)
    op, ref = make_conv(mf, O, rng, 3, 3, 128, 128, 3, 3, 1, 1, True, False, 0, False)
    batch = (stream_batch(op, 9) or 456) + 3
    n = batch * 9 * 128
    assert (batch * 9) % 128 and (ROUTING_SWITCHED or op.kernel_at(batch).startswith("conv_stream_rt"))
    x = torch.as_tensor(_inputs(rng, batch, 3, 3, 128, False)).cuda()
    want = op(x).cpu().numpy().reshape(-1)
    for off in (16, 48):                               # 16-byte-aligned offsets keep the fast path
        buf = torch.full((off + n + 4096,), 0x5A, dtype=torch.int8, device="cuda")
        _lib.check(_lib.lib().mf_op_run(op._h, x.data_ptr(), batch, buf.data_ptr() + off, torch.cuda.current_stream().cuda_stream))
        b = buf.cpu().numpy()
        assert (b[:off] == 0x5A).all() and (b[off + n:] == 0x5A).all(), off
        assert np.array_equal(b[off:off + n], want)


def test_conv_stream_keeps_the_prepare_time_label(mf, O):
    rng = np.random.default_rng(10)
    for (H, C, N), label in (((3, 128, 128), "conv_gemm_rt"), ((2, 1024, 128), "conv2d_generic")):
        op, _ = make_conv(mf, O, rng, H, H, C, N, 3, 3, 1, 1, True, False, 1, False)
        batch = stream_batch(op, H * H)
        assert ROUTING_SWITCHED or batch is not None
        assert ROUTING_SWITCHED or (op.kernel == label and op.kernel_at(1) == label and op.kernel_at(7) == label), (op.kernel, op.kernel_at(1))
        assert op.set_generic(True).kernel_at(batch or 456) == "conv2d_generic" and op.set_generic(False).kernel == op.kernel_at(1)


def test_conv_stream_never_takes_filter_zero_points_or_ragged_n(mf, O):
    rng = np.random.default_rng(11)
    for N, wz in ((128, True), (130, False)):
        op, _ = make_conv(mf, O, rng, 3, 3, 128, N, 3, 3, 1, 1, True, wz, 1, False)
        assert stream_batch(op, 9) is None and op.kernel_at(1 << 16) == op.kernel
