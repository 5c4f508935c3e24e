// tconv_phase_dump -- tconv_phase_rt's host-built operands (wimage.cpp: build_tconv_image / _kc / _table) multiplied on the CPU the way
// the kernel reads them: one image staged into a tile with an input-zero-point halo, every phase of every base pixel as the product of
// the phase's weight image with the table's gather of the tile.  Writes the i32 accumulators [OH][OW][N] to the output file;
// tests/test_tconv_host.py compares them with tests/tconv_ref.py.  Every tile read is checked against the tile's bounds.
//   tconv_phase_dump H W C N KH KW sh sw OH OW izp NTS in.bin out.bin      (in.bin: x [H][W][C] then w [N][KH][KW][C], int8)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../microflow_rs_amd/csrc/wimage.hpp"

using namespace mf::wimage;

int main(int argc, char **argv) {
    if (argc != 15) return 2;
    int v[12];
    for (int i = 0; i < 12; ++i) v[i] = atoi(argv[1 + i]);
    const int H = v[0], W = v[1], C = v[2], N = v[3], KH = v[4], KW = v[5], sh = v[6], sw = v[7], OH = v[8], OW = v[9], izp = v[10], NTS = v[11];
    std::vector<int8_t> x((size_t)H * W * C), w((size_t)N * KH * KW * C);
    FILE *fi = fopen(argv[13], "rb");
    if (!fi || fread(x.data(), 1, x.size(), fi) != x.size() || fread(w.data(), 1, w.size(), fi) != w.size()) return 3;
    fclose(fi);
    const int padt = std::max(0, (H - 1) * sh + KH - OH) / 2, padl = std::max(0, (W - 1) * sw + KW - OW) / 2;
    const TconvTile t = tconv_tile(W, C, KH, KW, sh, sw, OH, OW, padt, padl); // (the plan's geometry, one whole image per tile)
    const int NBY = t.NBY, NBX = t.NBX, TYM = t.TYM, LP = t.LP, ROW = (int)t.ROW, RB = NBY + TYM - 1, NT = (N + 15) / 16;
    std::vector<int8_t> tile((size_t)RB * ROW, (int8_t)izp);
    for (int y = 0; y < H; ++y) std::copy(x.begin() + (size_t)y * W * C, x.begin() + (size_t)(y + 1) * W * C, tile.begin() + (size_t)(y + TYM - 1) * ROW + LP);
    const std::vector<TconvPhase> ph = tconv_phases(KH, KW, C, sh, sw);
    const std::vector<int8_t> img = build_tconv_image(w.data(), N, KH, KW, C, sh, sw, NTS);
    const std::vector<int32_t> kc = build_tconv_kc(w.data(), N, KH, KW, C, sh, sw, izp, NT * 16);
    const std::vector<int> tab = build_tconv_table(KH, KW, C, sh, sw, ROW);
    int KSUM = 0;
    for (const TconvPhase &p : ph) KSUM += p.KS;
    if (tab.size() != (size_t)32 + (size_t)KSUM * 4 || img.size() != (size_t)NT * KSUM * 1024) return 4;
    std::vector<int32_t> acc((size_t)OH * OW * N, 0);
    std::vector<char> seen((size_t)OH * OW, 0);
    for (int by = 0; by < NBY; ++by)
        for (int bx = 0; bx < NBX; ++bx)
            for (size_t pi = 0; pi < ph.size(); ++pi) {
                const int oy = by * sh + ph[pi].py - padt, ox = bx * sw + ph[pi].px - padl;
                if (oy < 0 || oy >= OH || ox < 0 || ox >= OW) continue;
                seen[(size_t)oy * OW + ox] = 1;
                const int KS = tab[2 * pi], kpre = tab[2 * pi + 1], wbase = (by + TYM - 1) * ROW + LP + bx * C;
                if (KS != ph[pi].KS) return 5;
                for (int n = 0; n < N; ++n) {
                    const int nt = n / 16, nt0 = nt / NTS * NTS, nts = std::min(NTS, NT - nt0); // the slice of tile nt
                    const int8_t *wt = img.data() + ((size_t)nt0 * KSUM + (size_t)nts * kpre + (size_t)(nt - nt0) * KS) * 1024;
                    long long a = kc[pi * (size_t)NT * 16 + n];
                    for (int ks = 0; ks < KS; ++ks)
                        for (int g = 0; g < 4; ++g) {
                            const int off = wbase + tab[32 + (kpre + ks) * 4 + g];
                            if (off < 0 || off + 16 > RB * ROW || off % 4 != 0 || (C % 16 == 0 && off % 16 != 0)) return 6;
                            for (int i = 0; i < 16; ++i) a += (long long)wt[((size_t)ks * 64 + g * 16 + (n & 15)) * 16 + i] * tile[(size_t)off + i];
                        }
                    acc[((size_t)oy * OW + ox) * N + n] = (int32_t)a;
                }
            }
    for (char s : seen)
        if (!s) return 7; // every output pixel belongs to exactly one (base, phase)
    FILE *fo = fopen(argv[14], "wb");
    if (!fo || fwrite(acc.data(), 4, acc.size(), fo) != acc.size()) return 8;
    fclose(fo);
    return 0;
}
