"""The block-form depthwise of ops 5..6 (k_quad.hip Blk32Phase) without a GPU: the operand of wimage.cpp build_dw_blk_weights against
a numpy model of the gather from the DMA-staged NHWC tile.  tests/cpp/dw_blk_dump.cpp (host compiler, address and undefined-behaviour
sanitizers) writes the operand; the tile is laid out byte for byte as the kernel's staging does it -- row pitch, left pad, the
16-byte chunks of a pixel swapped by tile row -- and every lane's K-bytes are fetched with the kernel's own address arithmetic: four
8-byte reads per wave (two channel quads at once) and the register swap that sorts them into two operands.  The products must be the
nine-tap sums of the row form on random tiles, for every unit, wave and lane.
C = 32 is the launch's own geometry (24 x 24, pitch 800, chunk ^= bit 2 of the tile row).  C = 64 (ops 9..10, 12 x 12) has no
block-form phase yet: its operand is checked through the same gather on an unswizzled NHWC tile, one 4-byte read per pixel and quad."""
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
    tmp = tmp_path_factory.mktemp("dw_blk57")
    exe = str(tmp / "dw_blk_dump")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(CSRC, "wimage.cpp"),
                           os.path.join(ROOT, "tests", "cpp", "dw_blk_dump.cpp"), "-o", exe])

    def run(n, w):
        src, dst = str(tmp / "w.bin"), str(tmp / "o.bin")
        w.astype(np.int8).tofile(src)
        out = subprocess.run([exe, "dw", str(n), src, dst], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stdout + out.stderr
        return np.fromfile(dst, dtype=np.int8)
    return run


def mfma(a, b):
    """a, b: [64 lanes][16 bytes] int8 operands of a 16 x 16 x 64 instruction -> D[16 rows m][16 columns n]"""
    a = a.astype(np.int64).reshape(4, 16, -1)
    b = b.astype(np.int64).reshape(4, 16, -1)
    return np.einsum("gmj,gnj->mn", a, b)


def direct_sums(x, w, zp):
    H, W, C = x.shape
    tile = np.full((H + 2, W + 2, C), zp, dtype=np.int64)
    tile[1:-1, 1:-1] = x
    out = np.zeros((H, W, C), dtype=np.int64)
    for ty in range(3):
        for tx in range(3):
            out += tile[ty:ty + H, tx:tx + W] * w[ty, tx]
    return out


def staged_tile(x, zp, row, lp, swz):
    """the LDS tile as the staging leaves it: halo bytes at the zero point, image row y at tile row y + 1 behind the left pad, and
    16-byte chunk c of a pixel at chunk position c ^ swz(tile row) (the DMA lane fetches the other chunk of the SOURCE row)"""
    H, W, C = x.shape
    tile = np.full((H + 2) * row + lp, zp, dtype=np.int8)
    for y in range(H):
        src = x[y].astype(np.int8).reshape(-1)                   # W * C bytes, W * C / 16 lanes of 16 bytes
        for lane in range(W * C // 16):
            s = lane ^ swz(y + 1)
            d = (y + 1) * row + lp + 16 * lane
            tile[d:d + 16] = src[16 * s:16 * s + 16]
    return tile


def test_block_depthwise_32_through_the_staged_tile(dump):
    H = W = 24
    C, ROW, LP, zp = 32, 800, 32, -77
    swz = lambda r: (r >> 2) & 1                                   # noqa: E731  (Blk32Phase::swz)
    rng = np.random.default_rng(5757)
    w = rng.integers(-128, 128, size=(3, 3, C), dtype=np.int64)
    x = rng.integers(-128, 128, size=(H, W, C), dtype=np.int64)
    direct = direct_sums(x, w, zp)
    A = dump(C, w).reshape(C // 4, 64, 16)
    tile = staged_tile(x, zp, ROW, LP, swz)
    assert tile.size == (H + 2) * ROW + 32                        # Blk32Phase::TILE: the last row's right halo pixel lies behind it
    seen = np.zeros((H, W, C), dtype=bool)
    for wave in range(4):
        for u in range(9):
            uy, ux = u // 3, u % 3
            X = np.zeros((64, 16), dtype=np.int8)                  # operand of quad 2 wave
            Y = np.zeros((64, 16), dtype=np.int8)                  # operand of quad 2 wave + 1
            for lane in range(64):
                n, g = lane & 15, lane >> 4
                by, bx, = n >> 2, n & 3
                r = 2 * by + g
                tbase = r * ROW + 64 * bx + 16 * ((wave >> 1) ^ swz(r)) + 8 * (wave & 1)
                off = uy * 8 * ROW + ux * 256
                rd = [tile[tbase + off + 32 * xx:tbase + off + 32 * xx + 8] for xx in range(4)]   # four ds_read_b64
                regs = [[rd[0][:4], rd[0][4:]], [rd[1][:4], rd[1][4:]], [rd[2][:4], rd[2][4:]], [rd[3][:4], rd[3][4:]]]
                regs[0][1], regs[1][0] = regs[1][0], regs[0][1]    # v_swap_b32
                regs[2][1], regs[3][0] = regs[3][0], regs[2][1]
                X[lane] = np.concatenate(regs[0] + regs[2])
                Y[lane] = np.concatenate(regs[1] + regs[3])
            for q, B in ((2 * wave, X), (2 * wave + 1, Y)):
                D = mfma(A[q], B)
                for n in range(16):
                    by, bx = 4 * uy + (n >> 2), 4 * ux + (n & 3)
                    for s in range(4):
                        y, xx = 2 * by + (s >> 1), 2 * bx + (s & 1)
                        assert (D[4 * s:4 * s + 4, n] == direct[y, xx, 4 * q:4 * q + 4]).all(), (wave, u, n, s, q)
                        seen[y, xx, 4 * q:4 * q + 4] = True
    assert seen.all()                                              # every output byte of the image, once per owner


def test_block_depthwise_64_through_an_nhwc_tile(dump):
    H = W = 12
    C, LP, zp = 64, 64, 19
    ROW = LP + W * C + LP
    rng = np.random.default_rng(6464)
    w = rng.integers(-128, 128, size=(3, 3, C), dtype=np.int64)
    x = rng.integers(-128, 128, size=(H, W, C), dtype=np.int64)
    direct = direct_sums(x, w, zp)
    A = dump(C, w).reshape(C // 4, 64, 16)
    tile = staged_tile(x, zp, ROW, LP, lambda r: 0)
    tile = np.concatenate([tile, np.full(ROW, zp, dtype=np.int8)])
    blocks = [(by, bx) for by in range(H // 2) for bx in range(W // 2)]   # 36 blocks: two units and a quarter
    seen = np.zeros((H, W, C), dtype=bool)
    for q in range(C // 4):
        for u in range(3):
            B = np.zeros((64, 16), dtype=np.int8)
            cols = [blocks[min(16 * u + n, len(blocks) - 1)] for n in range(16)]   # dead columns read a valid block
            for lane in range(64):
                (by, bx), g = cols[lane & 15], lane >> 4
                base = (2 * by + g) * ROW + LP + (2 * bx - 1) * C + 4 * q
                B[lane] = np.concatenate([tile[base + C * xx:base + C * xx + 4] for xx in range(4)])       # four ds_read_b32
            D = mfma(A[q], B)
            for n in range(16):
                if 16 * u + n >= len(blocks):
                    continue
                by, bx = cols[n]
                for s in range(4):
                    y, xx = 2 * by + (s >> 1), 2 * bx + (s & 1)
                    assert (D[4 * s:4 * s + 4, n] == direct[y, xx, 4 * q:4 * q + 4]).all(), (q, u, n, s)
                    seen[y, xx, 4 * q:4 * q + 4] = True
    assert seen.all()
