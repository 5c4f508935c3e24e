// conv_rows_lds's plan for image rows that are not whole dwords (k_rt.hip: k::conv_rows_plan, ConvRowsArgs::BYTES()) and the staging
// map of the conv_rows_bytes launch (conv_rows_bytes_map.hpp -- the text the kernel runs) without a GPU, linked against the built
// library.
//   conv_rows_bytes_plan plan H W C N KH KW sh sw same    ->  "rows G TILE lds BYTES step_bytes"  or  "none"
//   conv_rows_bytes_plan stage H W N KH KW sh sw same batch
//       stages a whole batch, step by step, through rows_bytes_elem / rows_bytes_src / rows_bytes_keep / rows_bytes_merge into a host
//       copy of the tiles, exactly as k_conv_rows_body.inc does (512 threads x 16 elements, the element registers kept from step to
//       step, aligned dword loads only), and compares the tiles byte for byte with what they must hold
//       ->  "ok G steps shifts bases"   (shifts: bit s set = byte shift s occurred on a dword that exists; bases: bit s set = a step
//       started at a byte with (address & 3) == s)
//       exit 1 and a line on stderr at the first difference, at a sentinel byte in a tile, or at a load wholly outside the batch
//   conv_rows_bytes_plan stage_pads H W C N KH KW sh sw padt padl OH OW batch
//       the same with any channel count and an explicit window placement: the plan of k::conv_rows_plan_pads(..., bytes_any_c = true),
//       what the PAD + convolution group asks for (rows W C bytes long, the image at tile row shy, tile byte XO)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "conv_rows_bytes_map.hpp"

using namespace mf::k;

static bool make_plan(ConvRowsArgs &r, int H, int W, int C, int N, int KH, int KW, int sh, int sw, bool same) {
    const int OH = same ? (H + sh - 1) / sh : (H - KH) / sh + 1, OW = same ? (W + sw - 1) / sw : (W - KW) / sw + 1;
    return conv_rows_plan(r, H, W, C, N, KH, KW, sh, sw, OH, OW, same);
}

static uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh)); } // v_alignbyte_b32

static int stage(ConvRowsArgs p, int batch);

int main(int argc, char **argv) {
    if (argc == 15 && !strcmp(argv[1], "stage_pads")) {
        int a[13];
        for (int i = 0; i < 13; ++i) a[i] = atoi(argv[2 + i]);
        ConvRowsArgs p{};
        if (a[6] < 1 || a[7] < 1 || a[12] < 1 || !conv_rows_plan_pads(p, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[10], a[11], a[8], a[9], true) ||
            !p.BYTES()) {
            fprintf(stderr, "no BYTES plan\n");
            return 1;
        }
        return stage(p, a[12]);
    }
    if (argc == 11 && !strcmp(argv[1], "plan")) {
        int a[9];
        for (int i = 0; i < 9; ++i) a[i] = atoi(argv[2 + i]);
        if (a[6] < 1 || a[7] < 1 || (!a[8] && (a[0] < a[4] || a[1] < a[5]))) return 2;
        ConvRowsArgs r{};
        if (!make_plan(r, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8] != 0)) {
            printf("none\n");
            return 0;
        }
        printf("rows %d %d %d %d %d\n", r.G, r.TILE, conv_rows_lds_bytes(r), r.BYTES() ? 1 : 0, r.G * r.H * r.ROWB);
        return 0;
    }
    if (!(argc == 11 && !strcmp(argv[1], "stage"))) return 2;
    const int H = atoi(argv[2]), W = atoi(argv[3]), N = atoi(argv[4]), KH = atoi(argv[5]), KW = atoi(argv[6]), sh = atoi(argv[7]), sw = atoi(argv[8]);
    const bool same = atoi(argv[9]) != 0;
    const int batch = atoi(argv[10]);
    ConvRowsArgs p{};
    if (sh < 1 || sw < 1 || batch < 1 || !make_plan(p, H, W, 1, N, KH, KW, sh, sw, same) || !p.BYTES()) {
        fprintf(stderr, "no BYTES plan\n");
        return 1;
    }
    return stage(p, batch);
}

static int stage(ConvRowsArgs p, int batch) {
    const int H = p.H, W = p.W, ROWB = p.ROWB;
    constexpr int NTHR = 512, MAXE = 16, GUARD = 16;
    constexpr uint8_t SENT = 0x5a, IZP = 0xc3;           // neither is an image byte below
    p.izp4 = 0x01010101u * IZP;
    const long total = (long)batch * H * ROWB;
    // [GUARD sentinel bytes][the batch, 16-byte aligned][GUARD sentinel bytes]
    std::vector<uint8_t> store((size_t)total + 2 * GUARD + 16, SENT);
    uint8_t *in = store.data();
    while (((uintptr_t)in & 15) != 0) ++in;
    in += GUARD;
    static const uint8_t EXTREME[] = {0x80, 0x7f, 0xff, 0x00, 0x01, 0x81, 0x7e};
    uint32_t lcg = 12345u + (uint32_t)(H * 131 + W);
    for (long i = 0; i < total; ++i) {
        lcg = lcg * 1664525u + 1013904223u;
        in[i] = EXTREME[(lcg >> 16) % 7];
    }
    long outside = 0;
    auto load = [&](long d) {                            // aligned dword d of `in`
        if (4 * d + 4 <= 0 || 4 * d >= total) ++outside;
        uint32_t w;
        memcpy(&w, in + 4 * d, 4);
        return w;
    };
    const int G = p.G, IMGB = H * p.ROWB, nsteps = (batch + G - 1) / G;
    std::vector<uint8_t> tile((size_t)G * p.TILE, IZP), want;
    std::vector<uint32_t> el((size_t)NTHR * MAXE), lo(el.size()), hi(el.size());
    for (size_t i = 0; i < el.size(); ++i) el[i] = rows_bytes_elem(p, (int)i);   // slot tid + NTHR * e
    unsigned shifts = 0, bases = 0;
    for (int st = 0; st < nsteps; ++st) {
        // fetch(st)
        const size_t sb = (size_t)st * G * IMGB;
        const long src = (long)(sb >> 2);
        const uint32_t low2 = (uint32_t)sb & 3u;
        bases |= 1u << low2;
        const int lim = (G < batch - st * G ? G : batch - st * G) * IMGB;
        for (size_t i = 0; i < el.size(); ++i) {
            const RowsBytesSrc m = rows_bytes_src(el[i], low2, p.ROWB);
            const bool ok = el[i] != ROWS_BYTES_NONE && rows_bytes_first(el[i]) < lim;
            lo[i] = load(src + (ok ? m.d0 : 0));
            hi[i] = load(src + (ok && m.two ? m.d0 + 1 : 0));
            if (el[i] != ROWS_BYTES_NONE) el[i] = rows_bytes_keep(el[i], m.shift);
            if (ok) shifts |= 1u << m.shift;
        }
        // the tile write
        for (size_t i = 0; i < el.size(); ++i) {
            const uint32_t got = rows_bytes_merge(alignbyte(hi[i], lo[i], rows_bytes_kept(el[i])), rows_bytes_real(el[i], p.ROWB), p.izp4);
            const uint32_t w = rows_bytes_first(el[i]) < lim ? got : p.izp4;
            if (el[i] != ROWS_BYTES_NONE) {
                if (rows_bytes_tile(el[i]) + 4 > (int)tile.size()) {
                    fprintf(stderr, "step %d slot %zu: tile offset %d outside the tiles\n", st, i, rows_bytes_tile(el[i]));
                    return 1;
                }
                memcpy(tile.data() + rows_bytes_tile(el[i]), &w, 4);
            }
        }
        // what the tiles must hold: every image byte in its place, the input zero point everywhere else
        want.assign(tile.size(), IZP);
        for (int g = 0; g < G && st * G + g < batch; ++g)
            for (int y = 0; y < H; ++y)
                memcpy(want.data() + (size_t)g * p.TILE + (size_t)(y + p.shy) * p.TWP + p.XO, in + ((size_t)(st * G + g) * H + y) * ROWB, (size_t)ROWB);
        for (size_t i = 0; i < tile.size(); ++i) {
            if (tile[i] == SENT) {
                fprintf(stderr, "step %d: sentinel at tile byte %zu\n", st, i);
                return 1;
            }
            if (tile[i] != want[i]) {
                fprintf(stderr, "step %d: tile byte %zu is %02x, not %02x\n", st, i, tile[i], want[i]);
                return 1;
            }
        }
    }
    if (outside) {
        fprintf(stderr, "%ld loads of a dword wholly outside the batch\n", outside);
        return 1;
    }
    printf("ok %d %d %u %u\n", G, nsteps, shifts, bases);
    return 0;
}
