// Prints one line per host weight layout (microflow_rs_amd/csrc/wimage.cpp) and shape: `name shape bytes fnv1a64`.
// tests/test_wimage_host.py builds this with the address and undefined-behaviour sanitizers and compares the lines
// with tests/golden/wimage_layouts.txt.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../microflow_rs_amd/csrc/wimage.hpp"

using namespace mf::wimage;

static std::vector<int8_t> weights(size_t n, uint64_t seed) { // fixed LCG (Knuth's MMIX constants), top byte of the state
    std::vector<int8_t> w(n);
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
    for (size_t i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        w[i] = (int8_t)(s >> 56);
    }
    return w;
}
static uint64_t fnv1a64(const void *p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t *)p)[i]) * 0x100000001b3ull;
    return h;
}
static void line(const char *name, const char *shape, const void *p, size_t bytes) {
    printf("%s %s %zu %016llx\n", name, shape, bytes, (unsigned long long)fnv1a64(p, bytes));
}
template <typename T> static void line(const char *name, const char *shape, const std::vector<T> &v) {
    line(name, shape, v.data(), v.size() * sizeof(T));
}
#define SHAPE(...) (snprintf(shape, sizeof shape, __VA_ARGS__), shape)

int main() {
    char shape[96];
    for (int K : {8, 16, 32, 64, 128})
        for (int N : {16, 64, 128}) line("pw", SHAPE("K%d,N%d", K, N), build_pw_weights(weights((size_t)N * K, 1).data(), K, N));
    for (int C : {8, 16, 32}) {
        const std::vector<int8_t> dense = build_dw_mm_weights(weights((size_t)9 * C, 2).data(), C);
        line("dw_mm", SHAPE("C%d", C), dense);
        line("dw_sp", SHAPE("C%d", C), build_dw_sp_weights(dense, C == 8 ? 1 : C / 16));
    }
    {
        const int rt[4][5] = {{3, 3, 16, 3, 1}, {5, 5, 24, 7, 1}, {3, 3, 4, 3, 4}, {7, 7, 2, 13, 8}}; // KH, KW, C, KS, P
        for (const int *s : rt)
            line("dw_mm_rt", SHAPE("%dx%d,C%d,KS%d,P%d", s[0], s[1], s[2], s[3], s[4]),
                 build_dw_mm_rt_weights(weights((size_t)s[0] * s[1] * s[2], 3).data(), s[0], s[1], s[2], s[3], s[4]));
    }
    for (int C : {2, 4, 8})
        for (int S : {1, 2}) line("dw_mm_sp", SHAPE("C%d,S%d", C, S), build_dw_mm_weights_sp(weights((size_t)9 * C, 4).data(), C, S));
    {
        const int rr[4][2] = {{8, 8}, {8, 16}, {16, 16}, {32, 32}}; // K, N
        for (const int *s : rr) line("pw_rr", SHAPE("K%d,N%d", s[0], s[1]), build_pw_rr_weights(weights((size_t)s[0] * s[1], 5).data(), s[0], s[1]));
    }
    {
        const int rt[4][4] = {{12, 4, 4, 0}, {40, 20, 2, 0}, {80, 24, 1, 1}, {144, 16, 1, 1}}; // K, N, group, ones
        for (const int *s : rt) {
            const std::vector<int8_t> img = build_pw_rt_weights(weights((size_t)s[0] * s[1], 6).data(), s[0], s[1], s[2], s[3] != 0);
            line("pw_rt", SHAPE("K%d,N%d,G%d,ones%d", s[0], s[1], s[2], s[3]), img);
            if (!s[3]) continue;
            // the shared ones tile is what follows pw_rt's weight tiles (and conv_mm_rt's: K = KH KW C = 144)
            const int KS = (s[0] * s[2] + 63) / 64;
            std::vector<int8_t> ones((size_t)KS * 1024, 0);
            fill_ones_tile(ones.data(), s[0] * s[2], KS);
            line("ones_tile", SHAPE("K%d,KS%d", s[0] * s[2], KS), ones);
            line("pw_rt_tail", SHAPE("K%d,KS%d", s[0] * s[2], KS), img.data() + img.size() - ones.size(), ones.size());
        }
    }
    line("pw_rt_reg", "K32,N16,G2,TB2,NBLK1", build_pw_rt_reg_weights(weights(16 * 32, 7).data(), 32, 16, 2, 2, 1));
    line("pw_rt_reg", "K64,N200,G1,TB4,NBLK4", build_pw_rt_reg_weights(weights(200 * 64, 7).data(), 64, 200, 1, 4, 4));
    line("pw_plain", "K64,N16", build_pw_plain_weights(weights(16 * 64, 8).data(), 64, 16));
    line("pw_plain", "K128,N32", build_pw_plain_weights(weights(32 * 128, 8).data(), 128, 32));
    {
        const std::vector<int8_t> w = weights(9 * 8, 9);
        uint32_t wrow[3][8], wmm[64][2];
        build_stem_rows(w.data(), 8, wrow), build_stem_mm(w.data(), 8, &wmm[0][0], 2);
        line("stem_rows", "N8", wrow, sizeof wrow);
        line("stem_mm", "N8", wmm, sizeof wmm);
    }
    for (int N : {4, 8}) {
        uint32_t wmm[64][4];
        build_stem_mm(weights((size_t)9 * N, 10).data(), N, &wmm[0][0], 4);
        line("stem_rt_mm", SHAPE("N%d", N), wmm, sizeof wmm);
    }
    line("dw_c1_pack", "3x3,N8", build_dw_c1_pack(weights(3 * 3 * 8, 11).data(), 3, 3, 8, 1));
    line("dw_c1_pack", "10x8,N5", build_dw_c1_pack(weights(10 * 8 * 5, 11).data(), 10, 8, 5, 2));
    // conv_rows_lds: KG = dwords of a filter row, NP = output channels padded
    line("conv_rows_pack", "conv,3x3,C3,N6", build_conv_rows_pack(weights(6 * 3 * 3 * 3, 12).data(), false, 3, 3, 3, 6, 3, 8));
    line("conv_rows_mask", "conv,KW3,C3", build_conv_rows_mask(9, 3));
    line("conv_rows_pack", "dw,5x5,C1,N12", build_conv_rows_pack(weights(5 * 5 * 12, 12).data(), true, 5, 5, 1, 12, 2, 12));
    line("conv_rows_mask", "dw,KW5,C1", build_conv_rows_mask(5, 2));
    return 0;
}
