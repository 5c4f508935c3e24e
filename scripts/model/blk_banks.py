#!/usr/bin/env python3
"""LDS bank model of the block-form pair phase (k_quad.hip BlkPhase) for ops 1..2 of the five-operator launch: the two ds_read_b64 of a
patch row from the channel-quad-planar tile A, the stem's dword stores into it, and the four dword stores of a unit into tile B.
Pure arithmetic (lds_banks.py), no GPU.

    python scripts/model/blk_banks.py            the shipped pitches
    python scripts/model/blk_banks.py --sweep    every tile-A row pitch from 200 to 448 and every tile-B row pad"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lds_banks import cycles, ideal  # noqa: E402

H = W = 48
B_LP, B_C = 16, 16


def tile_a_reads(row, wave=3, unit=1, quad=0):
    """both 8-byte halves of the lane's 16-byte patch row"""
    plane = (H + 2) * row
    out = []
    for half in (0, 8):
        addrs = []
        for lane in range(64):
            n, g = lane & 15, lane >> 4
            by, bcx = 2 * wave + (n >> 3), n & 7
            addrs.append(quad * plane + (2 * by + g) * row + 8 * bcx + 64 * unit + half)
        out.append(cycles(addrs, "read_b64"))
    return out


def stem_stores(row, lp=4, rp=5):
    """the stem's three tile types of one row pair: lane (col, g) stores pixel 2 j + (g >> 1), channel quad g & 1"""
    plane = (H + 2) * row
    out = []
    for t in range(3):
        addrs = []
        for lane in range(64):
            col, g = lane & 15, lane >> 4
            oy1, j1 = (1, col - 8) if col >= 8 else (0, 16 + col)
            r, j = ((1, col), (1 + oy1, j1), (2, 8 + col))[t]
            addrs.append(rp * 2 * row + (g & 1) * plane + r * row + lp + 8 * j + 4 * (g >> 1))
        out.append(cycles(addrs, "write_b32"))
    return out


def tile_b_stores(rowpad, wave=3, unit=1):
    row = B_LP + W * B_C + B_LP + rowpad
    out = []
    for s in range(4):
        addrs = []
        for lane in range(64):
            n, g = lane & 15, lane >> 4
            by, bcx = 2 * wave + (n >> 3), n & 7
            addrs.append((2 * by + 1 + (s >> 1)) * row + B_LP + 32 * bcx + 4 * g + 256 * unit + 16 * (s & 1))
        out.append(cycles(addrs, "write_b32"))
    return out


if __name__ == "__main__":
    if "--sweep" in sys.argv:
        for row in range(200, 449, 8):
            print("tile A row pitch %3d: reads %s (ideal %d each), stem stores %s" % (row, tile_a_reads(row), ideal("read_b64"), stem_stores(row)))
        for pad in range(0, 129, 16):
            print("tile B row pad %3d: stores %s (ideal %d each)" % (pad, tile_b_stores(pad), ideal("write_b32")))
    else:
        print("tile A row pitch 320: reads %s (ideal %d each), stem stores %s (ideal %d each)" % (tile_a_reads(320), ideal("read_b64"), stem_stores(320), ideal("write_b32")))
        print("tile A row pitch 200: reads %s" % tile_a_reads(200))
        print("tile B row pad 32: stores %s (ideal %d each; a store's cycles are set by its data transfer, 4: 2-way is free, 4-way costs 2 x)" % (tile_b_stores(32), ideal("write_b32")))
