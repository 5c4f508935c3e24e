#!/usr/bin/env python3
"""LDS bank model of the block-form phase A of ops 5..6 (k_quad.hip Blk32Phase: 24 x 24 x 32 -> 32, stride 1), a sibling of blk_banks.py.
Pure arithmetic (lds_banks.py), no GPU.

  tile A : the DMA-staged NHWC tile.  A lane's K-bytes are four pixels x (two channel quads = 8 bytes): four ds_read_b64.  All 32
           lanes of a half read the SAME 8 bytes of their 16-byte chunk, so 32 lanes can cover at most 16 of the 32 bank pairs:
           2-way (4 cycles) is the floor; four ds_read_b32 per quad at one dword position reach 8 of 32 banks (4-way, 8 cycles).
           Knobs: the row pitch and a chunk swizzle by tile row (source side: the DMA lane picks the other 16-byte chunk).
  MID    : the depthwise result, NHWC, 8 bytes per (pixel, wave): one ds_write_b64 per unit; the pointwise reads 8 bytes per lane
           (16 pixels = 2 rows x 8) with ds_read_b64.  Knobs: the row pad and an XOR on the 8-byte unit index by pixel bits.
  tile B : the pointwise result at pair B's own layout (the row form stores the same 8 bytes per lane at the same places).

    python scripts/model/blk57_banks.py            the shipped layout
    python scripts/model/blk57_banks.py --sweep    tile-A pitches / swizzles and every MID pad / XOR"""
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lds_banks import cycles, ideal  # noqa: E402

H = W = 24
C = 32
A_ROW, A_SWZ_BIT = 800, 2            # tile A: row pitch (left pad 32 + 768: a row's right halo pixel is the next row's left one), chunk ^= bit 2 of the tile row
M_PAD, M_FX, M_FY = 16, (4, 0), (0, 4)   # MID: row pad; unit ^= (parity of x & M_FX[i]) ^ (parity of y & M_FY[i]) in bit i
B_ROW, B_LP = 864, 32


def par(v):
    return bin(v).count("1") & 1


def swz_a(r, bit):
    return (r >> bit) & 1 if bit >= 0 else 0


def tile_a_reads(row=A_ROW, bit=A_SWZ_BIT, wave=0, unit=(1, 1), width=8):
    """the four patch pixels of a lane (width 8: both quads of the wave at once; 4: one quad)"""
    out = []
    for xx in range(4):
        addrs = []
        for lane in range(64):
            n, g = lane & 15, lane >> 4
            by, bx = 4 * unit[0] + (n >> 2), 4 * unit[1] + (n & 3)
            r = 2 * by + g
            addrs.append(r * row + 64 * bx + 32 * xx + 16 * ((wave >> 1) ^ swz_a(r, bit)) + 8 * (wave & 1))
        out.append(cycles(addrs, "read_b64" if width == 8 else "read_b32"))
    return out


def mid_unit(x, y, u, fx, fy):
    return u ^ (par(x & fx[0]) ^ par(y & fy[0])) ^ ((par(x & fx[1]) ^ par(y & fy[1])) << 1)


def mid_stores(pad=M_PAD, fx=M_FX, fy=M_FY, wave=0, unit=(1, 1)):
    mrow = W * C + pad
    addrs = []
    for lane in range(64):
        n, g = lane & 15, lane >> 4
        y, x = 2 * (4 * unit[0] + (n >> 2)) + (g >> 1), 2 * (4 * unit[1] + (n & 3)) + (g & 1)
        addrs.append(y * mrow + x * 32 + 8 * mid_unit(x, y, wave, fx, fy))
    return cycles(addrs, "write_b64")


def mid_reads(pad=M_PAD, fx=M_FX, fy=M_FY, wave=0, grp=(1, 1)):
    mrow = W * C + pad
    addrs = []
    for lane in range(64):
        n, g = lane & 15, lane >> 4
        y, x = 6 * wave + 2 * grp[0] + (n >> 3), 8 * grp[1] + (n & 7)
        addrs.append(y * mrow + x * 32 + 8 * mid_unit(x, y, g, fx, fy))
    return cycles(addrs, "read_b64")


def tile_b_stores(wave=0, grp=(1, 1)):
    addrs = []
    for lane in range(64):
        n, g = lane & 15, lane >> 4
        y, x = 6 * wave + 2 * grp[0] + (n >> 3), 8 * grp[1] + (n & 7)
        addrs.append((y + 1) * B_ROW + B_LP + x * 32 + 16 * ((g >> 1) ^ ((x >> 1) & 1)) + 8 * (g & 1))
    return cycles(addrs, "write_b64")


def mid_cost(pad, fx, fy):
    st = max(mid_stores(pad, fx, fy, w, u) for w in range(4) for u in ((0, 0), (1, 2)))
    ld = max(mid_reads(pad, fx, fy, w, g) for w in range(4) for g in ((0, 0), (2, 1)))
    return st, ld


if __name__ == "__main__":
    if "--sweep" in sys.argv:
        for row in (800, 832, 864, 896, 928, 960, 992, 1024, 1056):
            for bit in (-1, 0, 1, 2, 3):
                worst = max(max(tile_a_reads(row, bit, w, u)) for w in range(4) for u in ((0, 0), (1, 2)))
                print("tile A pitch %4d, chunk ^= tile-row bit %2d: worst ds_read_b64 %2d cycles (ideal %d; floor here 4)" % (row, bit, worst, ideal("read_b64")))
        best = []
        masks = range(8)
        for pad in range(0, 129, 16):
            for fx0, fx1, fy0, fy1 in itertools.product(masks, masks, masks, masks):
                st, ld = mid_cost(pad, (fx0, fx1), (fy0, fy1))
                best.append((st + ld, bin(fx0 | fx1 << 3 | fy0 << 6 | fy1 << 9).count("1"), pad, (fx0, fx1), (fy0, fy1), st, ld))
        best.sort()
        for b in best[:12]:
            print("MID pad %3d, x masks %s, y masks %s: ds_write_b64 %2d cycles (ideal %d), ds_read_b64 %d (ideal %d)" % (b[2], b[3], b[4], b[5], ideal("write_b64"), b[6], ideal("read_b64")))
    else:
        ra = [tile_a_reads(wave=w) for w in range(4)]
        print("tile A pitch %d, chunk ^= tile-row bit %d: ds_read_b64 per patch pixel %s cycles (ideal %d, floor 4)" % (A_ROW, A_SWZ_BIT, ra, ideal("read_b64")))
        print("  the same bytes as ds_read_b32 per quad: %s (ideal %d)" % (tile_a_reads(width=4), ideal("read_b32")))
        print("  the row form's pitch 832 without the row swizzle: %s" % tile_a_reads(832, -1))
        st, ld = mid_cost(M_PAD, M_FX, M_FY)
        print("MID pad %d, x masks %s, y masks %s: ds_write_b64 %d cycles (ideal %d), ds_read_b64 %d (ideal %d)" % (M_PAD, M_FX, M_FY, st, ideal("write_b64"), ld, ideal("read_b64")))
        print("tile B: ds_write_b64 %s cycles (ideal %d; the row form's stores are the same)" % ([tile_b_stores(w) for w in range(4)], ideal("write_b64")))
        per_wave = 9 * (sum(ra[0]) + st) + 9 * (ld + tile_b_stores())
        print("phase A per wave and image: %d LDS-array cycles in 9 x (4 reads + 1 store) + 9 x (1 read + 1 store)" % per_wave)
