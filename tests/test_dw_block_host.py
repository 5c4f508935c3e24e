"""The block-form operands of the stride-1 pair phase (microflow_rs_amd/csrc/wimage.cpp build_dw_blk_weights and
build_pw_iso_weights; k_quad.hip BlkPhase) without a GPU.  tests/cpp/dw_blk_dump.cpp, compiled with the host compiler under the
address and undefined-behaviour sanitizers, writes the operands for random filters; the matrix instruction is emulated in numpy with
the operand maps the kernel uses -- D[m][n] = sum over lane groups g and bytes j of A[lane (m, g)][j] * B[lane (n, g)][j] -- and
the products are compared with the direct sums."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "microflow_rs_amd", "csrc")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("dw_blk")
    exe = str(tmp / "dw_blk_dump")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(CSRC, "wimage.cpp"),
                           os.path.join(ROOT, "tests", "cpp", "dw_blk_dump.cpp"), "-o", exe])

    def run(kind, n, w):
        src, dst = str(tmp / "w.bin"), str(tmp / "o.bin")
        w.astype(np.int8).tofile(src)
        out = subprocess.run([exe, kind, str(n), src, dst], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stdout + out.stderr
        return np.fromfile(dst, dtype=np.int8)
    return run


def mfma(a, b):
    """a, b: [64 lanes][KB bytes] int8 operands of a 16 x 16 x (4 KB) instruction -> D[16 rows m][16 columns n]"""
    a = a.astype(np.int64).reshape(4, 16, -1)   # [g][m][j]
    b = b.astype(np.int64).reshape(4, 16, -1)   # [g][n][j]
    return np.einsum("gmj,gnj->mn", a, b)


@pytest.mark.parametrize("C", [8, 32])
def test_block_depthwise_equals_the_direct_sums(dump, C):
    rng = np.random.default_rng(1234 + C)
    H, W, zp = 6, 8, -37
    w = rng.integers(-128, 128, size=(3, 3, C), dtype=np.int64)
    x = rng.integers(-128, 128, size=(H, W, C), dtype=np.int64)
    tile = np.full((H + 2, W + 2, C), zp, dtype=np.int64)      # one-pixel halo at the input zero point
    tile[1:-1, 1:-1] = x
    direct = np.zeros((H, W, C), dtype=np.int64)
    for ty in range(3):
        for tx in range(3):
            direct += tile[ty:ty + H, tx:tx + W] * w[ty, tx]
    A = dump("dw", C, w).reshape(C // 4, 64, 16)
    blocks = [(by, bx) for by in range(H // 2) for bx in range(W // 2)]
    assert len(blocks) <= 16
    seen = set()
    for q in range(C // 4):
        B = np.zeros((64, 16), dtype=np.int8)
        for n, (by, bx) in enumerate(blocks):
            for g in range(4):  # patch row g = image row 2 by - 1 + g = tile row 2 by + g; x 2 bx - 1 .. 2 bx + 2 = tile x 2 bx .. 2 bx + 3
                B[16 * g + n] = tile[2 * by + g, 2 * bx:2 * bx + 4, 4 * q:4 * q + 4].reshape(16)
        D = mfma(A[q], B)
        for n, (by, bx) in enumerate(blocks):
            for s in range(4):
                y, xx = 2 * by + (s >> 1), 2 * bx + (s & 1)
                assert (D[4 * s:4 * s + 4, n] == direct[y, xx, 4 * q:4 * q + 4]).all(), (q, by, bx, s)
                seen.add((y, xx))
    assert seen == {(y, xx) for y in range(H) for xx in range(W)}     # every pixel: the four corners, all four sub-pixels
    # the operand is block diagonal in the channel: a row (pixel s, channel i) has no weight on another channel's bytes
    for q in range(C // 4):
        a = A[q].reshape(4, 16, 4, 4)                                   # [g][m][patch x][channel j]
        for m in range(16):
            assert not a[:, m, :, [j for j in range(4) if j != (m & 3)]].any()


@pytest.mark.parametrize("N", [16, 32])
def test_isolating_pointwise_operands(dump, N):
    rng = np.random.default_rng(99 + N)
    w = rng.integers(-128, 128, size=(N, 8), dtype=np.int64)
    A = dump("pw", N, w).reshape(4, N // 16, 64, 8)
    B = rng.integers(-128, 128, size=(64, 8), dtype=np.int64)        # lane (n, g): the 8 channels of pixel g of block n
    for s in range(4):
        other = B.copy()
        for g in range(4):
            if g != s:
                other[16 * g:16 * g + 16] = rng.integers(-128, 128, size=(16, 8))
        for t in range(N // 16):
            D = mfma(A[s, t], B.astype(np.int8))
            want = B[16 * s:16 * s + 16] @ w[16 * t:16 * t + 16].T    # [n][m]
            assert (D == want.T).all(), (s, t)
            assert (mfma(A[s, t], other.astype(np.int8)) == D).all(), (s, t)   # the other three pixels' bytes do not matter
            assert not A[s, t].reshape(4, 16, 8)[[g for g in range(4) if g != s]].any()
