"""conv_stream_sp24 (k_conv_stream_sparse.hip): deep Conv2D with a 2:4-sparse filter on the sparse matrix instruction, selected per launch
where conv_stream_rt is: bit-exact against conv2d_generic and the CPU oracle at a ragged row count just above the threshold; what keeps
conv_stream_rt; the bytes around the output; the MF_NO_CONV_SPARSE switch; one generated model."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT, ROUTING_SWITCHED
from tests.test_gpu_conv_gemm import _inputs, _out_hw, check, make_conv, mf  # noqa: F401  (mf: the module fixture)

sys.path.insert(0, os.path.join(ROOT, "tools"))
pytestmark = pytest.mark.gpu

# H, W, C, N, K, stride, SAME, rows the launch must at least have (49 152: the 256 x 256 tile), extreme operands
CASES = [(3, 3, 128, 128, 3, 1, True, 0, False),       # one k tile per tap; padded taps read the zero-point line; OH OW = 9 divides no tile
         (5, 4, 256, 128, 3, 2, True, 0, False),       # two k tiles per tap: the image's k order against the tap counters; odd H at stride 2
         (4, 4, 128, 256, 3, 1, False, 49152, False),  # the 256 x 256 tile with 8 waves
         (3, 3, 256, 128, 1, 1, True, 0, False),       # the plain GEMM
         (2, 2, 1024, 128, 3, 1, True, 0, False),      # K' = 9216: conv2d_generic's label, the OpImpl::NONE call site; mostly padding
         (4, 4, 512, 512, 3, 1, True, 0, True)]        # kept weights -128 / 127, an all-minimum image: |acc| beyond 2^25, epilogue mode 0
IDS = lambda c: "%dx%dx%d-N%d-%dx%ds%d%s" % (c[:5] + c[4:6] + ("S" if c[6] else "V",))  # noqa: E731


def pruned(rng, N, K, C, u8, extreme=False):
    """a 2:4 filter [N][K][K][C]: most groups of four with two non-zero bytes at random places, a share with one (the first four groups:
    each place alone) and a share with none; u8: around the "zero" byte 128.  extreme: kept bytes -128 / 127, and whole same-sign rows --
    both kept bytes of every group -128 in output channels 0 and 1, 127 in 2 and 3"""
    G, r = N * K * K * C // 4, K * K * C // 4
    v = np.where(rng.random((G, 4)) < 0.5, -128, 127) if extreme else rng.integers(-128, 127, (G, 4))
    v = v + (v >= 0) * (not extreme)
    keep = np.argsort(rng.random((G, 4)), axis=1) < rng.choice([2, 1, 0], G, p=[0.7, 0.15, 0.15])[:, None]
    if extreme:
        keep[:4 * r] = np.argsort(rng.random((4 * r, 4)), axis=1) < 2
        v[:2 * r], v[2 * r:4 * r] = -128, 127
    keep[:4] = np.eye(4, dtype=bool)
    f = (v * keep).reshape(N, K, K, C)
    return (f + 128).astype(np.uint8) if u8 else f.astype(np.int8)


def sparse_batch(op, OHW, floor=0, prefix="conv_stream_sp24<"):
    """images of the first power-of-two row count >= 64 (and >= floor) at which a launch runs the kernel; None: none up to 65 536"""
    for rows in (64 << i for i in range(11)):
        batch = -(-max(rows, floor) // OHW)
        if op.kernel_at(batch).startswith(prefix):
            return batch
    return None


def run_case(mf, O, case, u8, batch=None):
    H, W, C, N, K, s, same, floor, extreme = case
    rng = np.random.default_rng(sum(case[:6]) * 2 + int(u8))
    lo = 0 if u8 else -128
    f = pruned(rng, N, K, C, u8, extreme)
    # (extreme: the all-minimum image x[1] with izp at the minimum meets the same-sign rows with -128 at EVERY tap, padded ones included)
    assert not extreme or np.abs((f.astype(np.int64) - 128 * u8).reshape(N, -1).sum(1)).max() * 128 > 2 ** 25
    op, ref = make_conv(mf, O, rng, H, W, C, N, K, K, s, s, same, False, 0 if extreme else 1, u8, f=f, izp=lo if extreme else None)
    OH, OW = _out_hw(H, W, K, K, s, s, same)
    if batch is None:
        batch = sparse_batch(op, OH * OW, floor)
        assert ROUTING_SWITCHED or batch is not None, op.kernel_at(1 << 16)   # (the parent commit answers conv_stream_rt<...>)
        batch = (batch or 456) + 3                       # a ragged M whose last image straddles a tile
    name = op.kernel_at(batch)
    tile = int(name[name.index("<") + 1:-1]) if name.startswith("conv_stream_") else 128
    assert (batch * OH * OW) % 128 and (ROUTING_SWITCHED or tile == (256 if floor else tile)), name
    assert ROUTING_SWITCHED or K * K * C <= 8192 or op.kernel == "conv2d_generic", op.kernel
    x = _inputs(rng, batch, H, W, C, u8)
    if extreme:
        x[1] = lo
    edge = [i for i in range(batch) if i * OH * OW // tile != ((i + 1) * OH * OW - 1) // tile] or [tile // (OH * OW) - 1, tile // (OH * OW)]
    return op, x, batch, name, check(op, ref, x, [0, 1, edge[0], edge[-1], batch - 1])


@pytest.mark.parametrize("u8", [False, True], ids=["i8", "u8"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_conv_sparse_vs_oracle_and_generic(mf, O, case, u8):
    run_case(mf, O, case, u8)


def test_what_is_not_sparse_keeps_its_kernel(mf, O):
    rng = np.random.default_rng(21)
    f = pruned(rng, 128, 3, 128, False)
    f[-1, -1, -1, -4:] = (0, 5, -7, 9)                   # ONE group of three non-zeros, in the last row's last k tile
    op, ref = make_conv(mf, O, rng, 3, 3, 128, 128, 3, 3, 1, 1, True, False, 1, False, f=f)
    batch = sparse_batch(op, 9, prefix="conv_stream_rt<")
    assert sparse_batch(op, 9) is None and (ROUTING_SWITCHED or batch is not None)
    batch = (batch or 456) + 3
    check(op, ref, _inputs(rng, batch, 3, 3, 128, False), [0, batch - 1])
    for N, wz in ((128, True), (130, False)):            # filter zero points, ragged N: neither stream kernel
        op, _ = make_conv(mf, O, rng, 3, 3, 128, N, 3, 3, 1, 1, True, wz, 1, False, f=pruned(rng, N, 3, 128, False))
        assert sparse_batch(op, 9, prefix="conv_stream_") is None and op.kernel_at(1 << 16) == op.kernel
    op, _ = make_conv(mf, O, rng, 3, 3, 128, 128, 3, 3, 1, 1, True, False, 1, False, f=pruned(rng, 128, 3, 128, False))
    batch = sparse_batch(op, 9)
    assert ROUTING_SWITCHED or (batch is not None and op.kernel_at(1) == op.kernel and not op.kernel.startswith("conv_stream"))
    assert op.set_generic(True).kernel_at(batch or 456) == "conv2d_generic" and op.set_generic(False).kernel == op.kernel_at(1)


def test_conv_sparse_leaves_the_bytes_around_the_output(mf, O):
    import torch
    from microflow_rs_amd import _lib
    op, x, batch, name, want = run_case(mf, O, CASES[0], False)   # (a ragged M on conv_stream_sp24: asserted there)
    x, want, n = torch.as_tensor(x).cuda(), want.reshape(-1), want.size
    for off in (16, 48):                                 # 16-byte-aligned offsets keep the fast path
        buf = torch.full((off + n + 4096,), 0x5A, dtype=torch.int8, device="cuda")
        _lib.check(_lib.lib().mf_op_run(op._h, x.data_ptr(), batch, buf.data_ptr() + off, torch.cuda.current_stream().cuda_stream))
        b = buf.cpu().numpy()
        assert (b[:off] == 0x5A).all() and (b[off + n:] == 0x5A).all() and np.array_equal(b[off:off + n], want), off


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import microflow_rs_amd as mf
from oracle import oracle
from tests.test_gpu_conv_sparse import CASES, run_case
oracle.build()
*_, name, got = run_case(mf, oracle, CASES[0], False, int(sys.argv[3]))
np.save(sys.argv[2], got)
print(name)
"""


def test_switch_sends_sparse_filters_back_to_conv_stream_rt(mf, O, tmp_path):
    """MF_DEV=1 MF_NO_CONV_SPARSE=1 (a fresh child process: the switches are read once) runs conv_stream_rt on the same filter and batch,
    same bytes"""
    _, _, batch, name, want = run_case(mf, O, CASES[0], False)
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("MF_")}, MF_DEV="1", MF_NO_CONV_SPARSE="1")
    path = str(tmp_path / "dense.npy")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path, str(batch)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (ROUTING_SWITCHED or name.startswith("conv_stream_sp24<")) and r.stdout.split()[-1].startswith("conv_stream_rt<"), (name, r.stdout)
    assert np.array_equal(np.load(path), want)


def test_generated_model_with_pruned_deep_convolutions(O):
    """4x4x128 -> 3x3 128 -> 1x1 256, both filters 2:4 (tflite_writer prune24=): run_quantized against the oracle model on sampled images,
    and against itself on the generic kernels, unfused, and under hipGraph (eager, captured, replayed)"""
    import torch
    import microflow_rs_amd as mf
    import tflite_writer as tw
    blob = tw.conv_net(np.random.default_rng(17), (4, 4, 128), [("conv", 128, 3, 1), ("conv", 256, 1, 1)], act_scale=6.0 / 255, prune24=(0, 1))
    batch = 32768 // 16 + 3                               # rows beyond both layers' thresholds (C = 128: 16 384; a 32 KiB 1x1 filter: 32 768)
    m, om = mf.Model(blob), O.Model(blob)
    m.prepare(batch)
    # (neither layer inside a fused group: both launch through the operator's own per-launch choice, which kernel_at names above)
    names = [m.op(i)["kernel"] for i in range(2)]
    assert ROUTING_SWITCHED or (names[0] == "conv_gemm_rt" and names[1] and "fused" not in names[1]), names
    xq = np.random.default_rng(3).integers(-128, 128, (batch, m.input_elems)).astype(m.dtype)
    x = torch.as_tensor(xq).cuda()
    ref = m.run_quantized(x).clone()
    pick = [0, 1, 7, 8, batch // 2, batch - 1]
    assert np.array_equal(ref.cpu().numpy().reshape(batch, -1)[pick], om.run_quantized_batch(xq[pick]).reshape(len(pick), -1))
    assert len(np.unique(ref.cpu().numpy())) > 20
    for setter in (m.set_generic, lambda on: m.set_fusion(not on), m.set_graph):
        setter(True)
        for it in range(3):
            assert torch.equal(m.run_quantized(x), ref), (setter, it)
        setter(False)
