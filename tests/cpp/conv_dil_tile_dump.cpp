// conv_dil_tile_dump -- conv_dil_rt's tile row (wimage.cpp: conv_dil_tile, conv_dil_column) staged and read on the CPU the way the kernel
// does: every image column to its plane and position inside a halo, then every tap of every window read at (window start) + kx C.
// Prints "PL PP LP ROW"; exit 3: a tap's bytes are not its input column's (or the halo's), 4: a read leaves the row or is misaligned.
//   conv_dil_tile_dump W C KW sw dw OW padl
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../microflow_rs_amd/csrc/wimage.hpp"

using namespace mf::wimage;

int main(int argc, char **argv) {
    if (argc != 8) return 2;
    int v[7];
    for (int i = 0; i < 7; ++i) v[i] = atoi(argv[1 + i]);
    const int W = v[0], C = v[1], KW = v[2], sw = v[3], dw = v[4], OW = v[5], padl = v[6];
    const ConvDilTile t = conv_dil_tile(W, C, KW, sw, dw, OW, padl);
    std::vector<int> row((size_t)t.ROW, -1); // -1: the halo; else column x of the image
    for (int x = 0; x < W; ++x)
        for (int c = 0; c < C; ++c) {
            const long long o = conv_dil_column(t, C, dw, x + padl) + c;
            if (o < 0 || o >= t.ROW || row[(size_t)o] != -1) return 4; // (two columns on one byte)
            row[(size_t)o] = x;
        }
    for (int ox = 0; ox < OW; ++ox) {
        const long long base = conv_dil_column(t, C, dw, ox * sw);
        if (base % (C % 16 == 0 ? 16 : 4) != 0 || base + t.KWCP > t.ROW) return 4;
        for (int kx = 0; kx < KW; ++kx)
            for (int c = 0; c < C; ++c) {
                const int x = ox * sw - padl + kx * dw;
                if (row[(size_t)(base + (long long)kx * C + c)] != (x >= 0 && x < W ? x : -1)) return 3;
            }
    }
    printf("%d %lld %d %lld\n", t.PL, t.PP, t.LP, t.ROW);
    return 0;
}
