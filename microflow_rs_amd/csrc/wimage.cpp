// wimage.cpp -- weight images: the operand layouts the host builds for the kernels.  Host code on bytes and ints only
// (see wimage.hpp); the comments here are the description of the operand maps the kernels rely on.
#include "wimage.hpp"

#include <cstring>

namespace mf {
namespace wimage {

// operand A of v_mfma_i32_16x16x64_i8 for pw_mfma<K,N>: [blk][q][tt][ks][lane][16 bytes]
std::vector<int8_t> build_pw_weights(const int8_t *w /*[N][K]*/, int K, int N) {
    const int NB = N < 64 ? N : 64, TB = NB / 16, NSPLIT = N / NB;
    const int KS = K < 64 ? 1 : K / 64, Q = K < 64 ? 64 / K : 1;
    std::vector<int8_t> out((size_t)NSPLIT * Q * TB * KS * 64 * 16, 0);
    for (int blk = 0; blk < NSPLIT; ++blk)
        for (int q = 0; q < Q; ++q)
            for (int tt = 0; tt < TB; ++tt)
                for (int ks = 0; ks < KS; ++ks)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int r = lane & 15, g = lane >> 4; // A row, k-block of this lane
                        // row r = 4*gr + j of tile tt is channel base + gr*(NB/4) + 4*tt + j
                        const int gr = r >> 2, j = r & 3;
                        const int ch = blk * NB + gr * (NB / 4) + 4 * tt + j;
                        int8_t *dst = &out[(((((size_t)blk * Q + q) * TB + tt) * KS + ks) * 64 + lane) * 16];
                        for (int i = 0; i < 16; ++i) {
                            int k = -1;
                            if (K >= 64) k = ks * 64 + g * 16 + i;
                            else if (K == 32) k = ((g >> 1) == q) ? (g & 1) * 16 + i : -1;
                            else if (K == 16) k = (g == q) ? i : -1;
                            else if (K == 8) k = (g == (q >> 1) && (i >> 3) == (q & 1)) ? (i & 7) : -1;
                            dst[i] = k >= 0 ? w[(size_t)ch * K + k] : (int8_t)0;
                        }
                    }
    return out;
}

// Depthwise 3x3 weights [3][3][C] as operand A of v_mfma_i32_16x16x64_i8 for dwpw_mm (k_fused_mm.hip):
// [group q][filter row ty][lane][16 bytes].  A lane holds row r = lane & 15 of the 16 x 64 block-diagonal
// matrix, K-block g = lane >> 4.
//   C >= 16: row r = channel 16q + r; block g = tap column tx = g (g == 3: padding), its 16 K-bytes are
//            the 16 channels of that tap's pixel -> the only non-zero byte is c' == r: w[ty][g][16q + r].
//   C == 8 : row r = (output pixel parity r >> 3, channel r & 7); block g = input pixel pair
//            (2x-2+2g, 2x-1+2g), byte (pp, c'): non-zero for c' == channel and tap column
//            tx = 2g + pp - 1 - parity in 0..2.
std::vector<int8_t> build_dw_mm_weights(const int8_t *w /*[3][3][C]*/, int C) {
    const int NQ = C == 8 ? 1 : C / 16;
    std::vector<int8_t> out((size_t)NQ * 3 * 64 * 16, 0);
    for (int q = 0; q < NQ; ++q)
        for (int ty = 0; ty < 3; ++ty)
            for (int lane = 0; lane < 64; ++lane) {
                const int r = lane & 15, g = lane >> 4;
                int8_t *dst = &out[(((size_t)q * 3 + ty) * 64 + lane) * 16];
                if (C == 8) {
                    const int par = r >> 3, c = r & 7;
                    for (int pp = 0; pp < 2; ++pp) {
                        const int tx = 2 * g + pp - 1 - par;
                        if (g < 3 && tx >= 0 && tx <= 2) dst[pp * 8 + c] = w[(ty * 3 + tx) * 8 + c];
                    }
                } else if (g < 3) {
                    dst[r] = w[(ty * 3 + g) * C + 16 * q + r];
                }
            }
    return out;
}

// The same taps for the structured-sparse matrix instruction (k_quad.hip).  A 3x3 depthwise operand A is block diagonal: a row has at
// most two non-zero bytes in any 16-byte chunk, never two in one group of four -- 2:4 sparse with room to spare -- and
// v_smfmac_i32_16x16x128_i8 multiplies a 2:4-sparse 16 x 128 A in the time v_mfma_i32_16x16x64_i8 takes for a dense 16 x 64
// (scripts/ubench/mfma_rates.hip: 16.7 against 17 cycles).  Eight of the nine (filter row, chunk column) blocks of
// build_dw_mm_weights go into ONE sparse instruction, the ninth into a v_mfma_i32_16x16x32_i8: two matrix instructions per unit
// instead of three.  Operand layout as measured by scripts/ubench/smfmac_probe.hip (profiles/r06/h_smfmac_probe.txt):
//   B lane (column, group lb) holds 32 bytes = two 16-byte chunks (half 0 / 1); A lane (row, group ga) holds 16 stored bytes:
//   stored byte s = 8 ha + 2 grp + j is element j of group grp (four dense bytes) of the chunk that B lane group lb = 2 (ga & 1) + ha
//   holds in half ga >> 1, and bits 2 s + 1 : 2 s of the index register say which of the four dense bytes it is.
// Chunk of (lb, half) as (filter row, chunk column): half 0 of lane groups 0..3 = (0,0) (0,1) (0,2) (1,0), half 1 = (1,1) (1,2) (2,0) (2,1);
// the ninth is (2,2).
// Returns [q][lane][32 bytes] = {stored A (16), index (4), ninth block as operand A of v_mfma_i32_16x16x32_i8 (8: lane group g' holds
// bytes 8 g' .. 8 g' + 7 of the chunk, groups 2 and 3 zero), 4 bytes padding}; empty if a group of four holds more than two non-zeros.
const int DW_SP_CHUNK[4][2][2] = {{{0, 0}, {1, 1}}, {{0, 1}, {1, 2}}, {{0, 2}, {2, 0}}, {{1, 0}, {2, 1}}};
std::vector<int8_t> build_dw_sp_weights(const std::vector<int8_t> &dense /* build_dw_mm_weights */, int NQ) {
    std::vector<int8_t> out((size_t)NQ * 64 * 32, 0);
    auto block = [&](int q, int ty, int gch, int r) { return &dense[((((size_t)q * 3 + ty) * 64) + (size_t)(gch * 16 + r)) * 16]; };
    for (int q = 0; q < NQ; ++q)
        for (int lane = 0; lane < 64; ++lane) {
            const int r = lane & 15, ga = lane >> 4;
            int8_t *dst = &out[((size_t)q * 64 + lane) * 32];
            uint32_t idx = 0;
            for (int ha = 0; ha < 2; ++ha) {
                const int lb = 2 * (ga & 1) + ha, half = ga >> 1;
                const int8_t *blk = block(q, DW_SP_CHUNK[lb][half][0], DW_SP_CHUNK[lb][half][1], r);
                for (int grp = 0; grp < 4; ++grp) {
                    int pos[4], n = 0;
                    for (int b = 0; b < 4; ++b)
                        if (blk[4 * grp + b] != 0) pos[n++] = b;
                    if (n > 2) return {};
                    if (n == 0) pos[0] = 0, pos[1] = 1;
                    if (n == 1) pos[1] = (pos[0] + 1) & 3;
                    for (int j = 0; j < 2; ++j) {
                        const int sb = 8 * ha + 2 * grp + j;
                        dst[sb] = j < n ? blk[4 * grp + pos[j]] : (int8_t)0;
                        idx |= (uint32_t)pos[j] << (2 * sb);
                    }
                }
            }
            memcpy(dst + 16, &idx, 4);
            if (ga < 2) memcpy(dst + 20, block(q, 2, 2, r) + 8 * ga, 8);
        }
    return out;
}

// The block form of the same taps (k_quad.hip BlkPhase): ONE v_mfma_i32_16x16x64_i8 per channel quad computes a 2 x 2 output block
// per column.  Column n is output block (by, bx); its 64 K-bytes are the block's 4 x 4 input patch -- rows 2 by - 1 .. 2 by + 2,
// x 2 bx - 1 .. 2 bx + 2 -- of one channel quad: lane group g supplies patch row g, byte 4 xx + j = patch pixel xx, channel 4 q + j.
// Row m = 4 s + i is output pixel s = (sy, sx) = (s >> 1, s & 1) of the block, channel 4 q + i: lane (m, g) holds
// w[g - sy][xx - sx][4 q + i] in byte 4 xx + i where both differences are in 0..2, zero elsewhere.  The result lane (n, g') then
// holds the four channels of pixel g' of block n.  [quad q][lane][16 bytes]; C a multiple of 4.
std::vector<int8_t> build_dw_blk_weights(const int8_t *w /*[3][3][C]*/, int C) {
    const int NQ4 = C / 4;
    std::vector<int8_t> out((size_t)NQ4 * 64 * 16, 0);
    for (int q = 0; q < NQ4; ++q)
        for (int lane = 0; lane < 64; ++lane) {
            const int m = lane & 15, g = lane >> 4, s = m >> 2, i = m & 3, ty = g - (s >> 1);
            if (ty < 0 || ty > 2) continue;
            for (int xx = 0; xx < 4; ++xx) {
                const int tx = xx - (s & 1);
                if (tx >= 0 && tx <= 2) out[((size_t)q * 64 + lane) * 16 + 4 * xx + i] = w[(ty * 3 + tx) * C + 4 * q + i];
            }
        }
    return out;
}

// Pointwise weights [N][8] behind the block form: the depthwise result of a lane is the 8 channels of ONE pixel -- pixel g of block n
// in lane (n, g) -- so the B operand of v_mfma_i32_16x16x32_i8 holds four different pixels in its four K slices.  Operand s of the
// four "isolating" operands carries the weights in K-bytes 8 s .. 8 s + 7 only (lane group s; zero in the other three groups), so
// that instruction s sees pixel s alone: row m of tile t is output channel 16 t + m, byte b input channel b.
// [sub-pixel s][tile t][lane][8 bytes]; N a multiple of 16.
std::vector<int8_t> build_pw_iso_weights(const int8_t *w /*[N][8]*/, int N) {
    const int NT = N / 16;
    std::vector<int8_t> out((size_t)4 * NT * 64 * 8, 0);
    for (int s = 0; s < 4; ++s)
        for (int t = 0; t < NT; ++t)
            for (int m = 0; m < 16; ++m)
                memcpy(&out[(((size_t)s * NT + t) * 64 + 16 * s + m) * 8], w + (size_t)(16 * t + m) * 8, 8);
    return out;
}

// Depthwise weights [KH][KW][C] as operand A of conv_mm_rt's depthwise mode (k_rt.hip) and of dw_gemm_rt (k_dw_gemm.hip): [16-channel
// group][k step][lane] x 16 bytes; lane (row r, group g) of step ks holds tap t = 4 ks + g: its only non-zero byte is byte r = w[t][16 q
// + r] (zero for the channels 16 q + r >= C of a last, partial group).  P > 1 (dw_gemm_rt, C <= 8): one group, row r is channel r % C
// of the P adjacent pixels, byte r = w[t][r % C] for r < P C.
std::vector<int8_t> build_dw_mm_rt_weights(const int8_t *w, int KH, int KW, int C, int KS /* >= (KH KW + 3) / 4: padded with zero steps */,
                                           int P) {
    const int NQ = (C + 15) / 16, T = KH * KW;
    std::vector<int8_t> out((size_t)NQ * KS * 1024, 0);
    for (int q = 0; q < NQ; ++q)
        for (int ks = 0; ks < KS; ++ks)
            for (int lane = 0; lane < 64; ++lane) {
                const int r = lane & 15, t = 4 * ks + (lane >> 4);
                const int c = P > 1 ? (r < P * C ? r % C : -1) : (16 * q + r < C ? 16 * q + r : -1);
                if (t < T && c >= 0) out[(((size_t)q * KS + ks) * 64 + lane) * 16 + r] = w[(size_t)t * C + c];
            }
    return out;
}

// The same operand for FEWER than 16 channels (chain_rt, k_chain.hip): P = 16 / C horizontally adjacent pixels are one 16-channel
// "superpixel", stride S in superpixels.  Row r = (output pixel p = r / C of superpixel X, channel r % C); block g = input superpixel
// S X - 1 + g, whose byte (pp, c') is input pixel P (S X - 1 + g) + pp: non-zero for c' == channel and the tap column
// tx = P (g - 1) + pp - S p + 1 in 0..2 (output pixel P X + p reads input pixels S (P X + p) + tx - 1).
std::vector<int8_t> build_dw_mm_weights_sp(const int8_t *w /*[3][3][C]*/, int C, int S) {
    const int P = 16 / C;
    std::vector<int8_t> out((size_t)3 * 64 * 16, 0);
    for (int ty = 0; ty < 3; ++ty)
        for (int lane = 0; lane < 64; ++lane) {
            const int r = lane & 15, g = lane >> 4, p = r / C, c = r % C;
            int8_t *dst = &out[((size_t)ty * 64 + lane) * 16];
            for (int pp = 0; pp < P; ++pp) {
                const int tx = P * (g - 1) + pp - S * p + 1;
                if (g < 3 && tx >= 0 && tx <= 2) dst[pp * C + c] = w[(ty * 3 + tx) * C + c];
            }
        }
    return out;
}

// Pointwise weights [N][K] as operands A of v_mfma_i32_16x16x32_i8 for dwpw_rr (k_fused_mm.hip), whose B operand
// is the depthwise result as it sits in registers: [16-row tile m][lane][8 bytes].  Lane (r = lane & 15,
// g = lane >> 4) holds K-bytes 8g .. 8g+7 of MFMA row r.
//   rows : row 4g' + i of tile m is output channel (N/4) g' + 4m + i, so that lane g' of the result owns N/4
//          consecutive output bytes.  K = 8: rows are (pixel parity g' >> 1, channel 8 (g' & 1) + 4m + i).
//   K    : byte b < 4 is input channel 4g + b (K = 8: channel 4 (g & 1) + b of the pixel with parity g >> 1, used
//          only by the rows of that pixel); byte b >= 4 is channel 16 + 4g + b - 4 when K = 32, else unused.
std::vector<int8_t> build_pw_rr_weights(const int8_t *w /*[N][K]*/, int K, int N) {
    const bool pair = K == 8;
    const int NT = (pair ? 2 * N : N) / 16;
    std::vector<int8_t> out((size_t)NT * 64 * 8, 0);
    for (int m = 0; m < NT; ++m)
        for (int lane = 0; lane < 64; ++lane) {
            const int r = lane & 15, g = lane >> 4;
            const int gr = r >> 2, i = r & 3;
            const int n = pair ? 8 * (gr & 1) + 4 * m + i : (N / 4) * gr + 4 * m + i;
            int8_t *dst = &out[((size_t)m * 64 + lane) * 8];
            for (int b = 0; b < 8; ++b) {
                int k = -1;
                if (pair) {
                    if (b < 4 && (g >> 1) == (gr >> 1)) k = 4 * (g & 1) + b;
                } else if (b < 4) {
                    k = 4 * g + b;
                } else if (K == 32) {
                    k = 16 + 4 * g + (b - 4);
                }
                dst[b] = k >= 0 && n < N ? w[(size_t)n * K + k] : (int8_t)0; // (K = 8 with N < 16: the rows past N stay zero)
            }
        }
    return out;
}

// Operand A of v_mfma_i32_16x16x64_i8 for pw_rt (k_rt.hip): [16-row tile nt][k step ks][lane][16 bytes]; lane (r, g) holds
// K-bytes 64 ks + 16 g .. + 15 of row 16 nt + r.  `group` pixels form one row of the product: row gi * N + n multiplies
// only the K-bytes gj * K .. of its own pixel (block diagonal).  With `ones`, KS more KiB follow: a tile whose every row
// is 1 on the real K-bytes (the row sum a weight zero point needs).
std::vector<int8_t> build_pw_rt_weights(const int8_t *w /*[N][K]*/, int K, int N, int group, bool ones) {
    const int Kg = K * group, Ng = N * group, KS = (Kg + 63) / 64, NT = (Ng + 15) / 16;
    std::vector<int8_t> out(((size_t)NT * KS + (ones ? KS : 0)) * 1024, 0);
    for (int nt = 0; nt < NT; ++nt)
        for (int ks = 0; ks < KS; ++ks)
            for (int lane = 0; lane < 64; ++lane) {
                const int row = 16 * nt + (lane & 15), g = lane >> 4;
                if (row >= Ng) continue;
                const int gi = row / N, n = row % N;
                int8_t *dst = &out[(((size_t)nt * KS + ks) * 64 + lane) * 16];
                for (int i = 0; i < 16; ++i) {
                    const int kk = ks * 64 + g * 16 + i;
                    if (kk < Kg && kk / K == gi) dst[i] = w[(size_t)n * K + kk % K];
                }
            }
    if (ones) fill_ones_tile(&out[(size_t)NT * KS * 1024], Kg, KS);
    return out;
}

// The same product for pw_rt with the weights in registers: [block][tile t][k step][lane][16 bytes], TB tiles per block, and
// row 4 gr + i of tile t = channel 16 TB blk + 4 TB gr + 4 t + i (so that a lane ends with 4 TB consecutive output bytes).
std::vector<int8_t> build_pw_rt_reg_weights(const int8_t *w /*[N][K]*/, int K, int N, int group, int TB, int NBLK) {
    const int Kg = K * group, Ng = N * group, KS = (Kg + 63) / 64;
    std::vector<int8_t> out((size_t)NBLK * TB * KS * 1024, 0);
    for (int blk = 0; blk < NBLK; ++blk)
        for (int t = 0; t < TB; ++t)
            for (int ks = 0; ks < KS; ++ks)
                for (int lane = 0; lane < 64; ++lane) {
                    const int r = lane & 15, g = lane >> 4;
                    const int row = 16 * TB * blk + 4 * TB * (r >> 2) + 4 * t + (r & 3);
                    if (row >= Ng) continue;
                    const int gi = row / N, n = row % N;
                    int8_t *dst = &out[((((size_t)blk * TB + t) * KS + ks) * 64 + lane) * 16];
                    for (int i = 0; i < 16; ++i) {
                        const int kk = ks * 64 + g * 16 + i;
                        if (kk < Kg && kk / K == gi) dst[i] = w[(size_t)n * K + kk % K];
                    }
                }
    return out;
}

// Pointwise weights [N][K] as operands A of v_mfma_i32_16x16x64_i8 for the stage kernel: [tile][k-step][lane][16 B],
// row r = lane & 15 of tile tt is output channel 16 tt + r, K-bytes 64 ks + 16 (lane >> 4) .. + 15
std::vector<int8_t> build_pw_plain_weights(const int8_t *w, int K, int N) {
    const int KS = K / 64, NT = N / 16;
    std::vector<int8_t> out((size_t)NT * KS * 64 * 16);
    for (int tt = 0; tt < NT; ++tt)
        for (int ks = 0; ks < KS; ++ks)
            for (int lane = 0; lane < 64; ++lane) {
                const int r = lane & 15, g = lane >> 4;
                std::memcpy(&out[(((size_t)tt * KS + ks) * 64 + lane) * 16], w + (size_t)(16 * tt + r) * K + 64 * ks + 16 * g, 16);
            }
    return out;
}

// A tile of ones over the real K-bytes, [k step][lane][16 bytes] like the tiles above: the row sum a weight zero point
// needs comes out of the same product (pw_rt's and conv_mm_rt's <wzp> instances, k_rt.hip).
void fill_ones_tile(int8_t *dst, int K, int KS) {
    for (int ks = 0; ks < KS; ++ks)
        for (int lane = 0; lane < 64; ++lane)
            for (int i = 0; i < 16; ++i)
                if (ks * 64 + (lane >> 4) * 16 + i < K) dst[((size_t)ks * 64 + lane) * 16 + i] = 1;
}

// pair_wz_rt (k_pair_wz.hip) multiplies a filter zero point with a sum of stored bytes, and takes both sums from the matrix pipe:
// the window sum per channel is the depthwise product against the image of an all-ones filter (row c meets the nine bytes of
// channel c; lane group 3 meets zeros, as in every tap image), and a pixel's sum over its C intermediate bytes is the 1x1 product
// against a tile of ones that ends at C (a padded k step adds nothing).
std::vector<int8_t> build_dw_ones_image() {
    const std::vector<int8_t> ones((size_t)9 * 16, 1);
    return build_dw_mm_weights(ones.data(), 16);
}
std::vector<int8_t> build_pw_ones_tile(int C) {
    const int KS = (C + 63) / 64;
    std::vector<int8_t> out((size_t)KS * 1024, 0);
    fill_ones_tile(out.data(), C, KS);
    return out;
}

// The one-channel 3x3 stem dw3x3_stem (k_depthwise.hip), weights [3][3][N] with 8 output channels:
// wrow[ky][c] = bytes (w[ky][0][c], w[ky][1][c], w[ky][2][c], 0)
void build_stem_rows(const int8_t *w, int N, uint32_t wrow[3][8]) {
    for (int ky = 0; ky < 3; ++ky)
        for (int c = 0; c < 8; ++c) {
            uint32_t d = 0;
            for (int kx = 0; kx < 3; ++kx)
                d |= (uint32_t)(uint8_t)w[((size_t)ky * 3 + kx) * N + c] << (8 * kx);
            wrow[ky][c] = d;
        }
}

// ... and its matrix-pipe form, also operand A of dw3x3_stem_rt (k_rt.hip; N = 4 or 8): accumulator row r = (p, c) = pixel p of
// a 16-byte output group (N = 8: pixel 2j + p of a pixel pair), channel c; lane group g = filter row; the lane's K-bytes are
// input columns XS j - 4 .. of that row (N = 8: 4j-4 .. 4j+3), of which pixel p uses bytes 3 + 2 p .. 5 + 2 p.  8 K-bytes per
// lane for N = 8, else 16; `pitch` dwords per lane in wmm (2: dw3x3_stem, N = 8 only; 4: dw3x3_stem_rt, zero beyond the K-bytes).
void build_stem_mm(const int8_t *w, int N, uint32_t *wmm, int pitch) {
    const int KB = N == 8 ? 8 : 16;
    for (int lane = 0; lane < 64; ++lane) {
        const int r = lane & 15, g = lane >> 4, pp = r / N, c = r % N;
        uint8_t b[16] = {0};
        if (g < 3)
            for (int kx = 0; kx < 3; ++kx) b[3 + 2 * pp + kx] = (uint8_t)w[((size_t)g * 3 + kx) * N + c];
        for (int d = 0; d < pitch; ++d)
            wmm[lane * pitch + d] = d * 4 < KB ? ((uint32_t)b[4 * d] | (uint32_t)b[4 * d + 1] << 8 | (uint32_t)b[4 * d + 2] << 16 | (uint32_t)b[4 * d + 3] << 24) : 0u;
    }
}

// conv_rows_lds (k_rt.hip): a filter row as dwords, [ky][dword of the row][NP output channels], zero beyond the row and beyond N.
// (dw_c1_lds, k_depthwise.hip, reads the depthwise form with NP = 8: build_dw_c1_pack.)
// conv filters [N][KH][KW][C]: byte b of row ky = (kx, c) in memory order; depthwise [KH][KW][N], C == 1
std::vector<uint32_t> build_conv_rows_pack(const int8_t *w, bool depthwise, int KH, int KW, int C, int N, int KG, int NP) {
    std::vector<uint32_t> wp((size_t)KH * KG * NP, 0);
    const int RWB = KW * C;
    for (int n = 0; n < N; ++n)
        for (int ky = 0; ky < KH; ++ky)
            for (int b = 0; b < RWB; ++b) {
                const int8_t wv = depthwise ? w[((size_t)ky * KW + b) * N + n] : w[((size_t)n * KH + ky) * RWB + b];
                wp[((size_t)ky * KG + b / 4) * NP + n] |= (uint32_t)(uint8_t)wv << (8 * (b & 3));
            }
    return wp;
}
// ... and which bytes of each dword are taps (the window sum a weight zero point needs counts only those)
std::vector<uint32_t> build_conv_rows_mask(int RWB, int KG) {
    std::vector<uint32_t> mk((size_t)KG, 0);
    for (int b = 0; b < RWB; ++b) mk[(size_t)(b / 4)] |= 1u << (8 * (b & 3));
    return mk;
}

} // namespace wimage
} // namespace mf
