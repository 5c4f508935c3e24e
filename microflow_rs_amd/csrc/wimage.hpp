// wimage.hpp -- weight images: every operand layout the host builds for the kernels (operand A maps of the matrix
// instructions, packed window rows), as plain functions on bytes and ints.  Host only -- no HIP, no device -- so each
// layout can be checked on any machine (tests/test_wimage_host.py).  The maps themselves are described at the
// definitions (wimage.cpp).  Layouts that need a kernel's own plan struct stay with that kernel (k_conv_gemm.hip
// conv_gemm_weight_image, k_fc_rt.hip fc_rt_weight_image, k_fc_sparse.hip fc_sparse24_image).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mf {
namespace wimage {

std::vector<int8_t> build_pw_weights(const int8_t *w /*[N][K]*/, int K, int N);
std::vector<int8_t> build_dw_mm_weights(const int8_t *w /*[3][3][C]*/, int C);
std::vector<int8_t> build_dw_sp_weights(const std::vector<int8_t> &dense /* build_dw_mm_weights */, int NQ);
std::vector<int8_t> build_dw_blk_weights(const int8_t *w /*[3][3][C]*/, int C);
std::vector<int8_t> build_pw_iso_weights(const int8_t *w /*[N][8]*/, int N);
std::vector<int8_t> build_dw_mm_rt_weights(const int8_t *w, int KH, int KW, int C, int KS /* >= (KH KW + 3) / 4: padded with zero steps */,
                                           int P = 1);
std::vector<int8_t> build_dw_mm_weights_sp(const int8_t *w /*[3][3][C]*/, int C, int S);
std::vector<int8_t> build_pw_rr_weights(const int8_t *w /*[N][K]*/, int K, int N);
std::vector<int8_t> build_pw_rt_weights(const int8_t *w /*[N][K]*/, int K, int N, int group, bool ones);
std::vector<int8_t> build_pw_rt_reg_weights(const int8_t *w /*[N][K]*/, int K, int N, int group, int TB, int NBLK);
std::vector<int8_t> build_pw_plain_weights(const int8_t *w, int K, int N);

void fill_ones_tile(int8_t *dst /* KS KiB, zeroed */, int K, int KS);
// pair_wz_rt's two ones images (k_pair_wz.hip): the sums a filter zero point is multiplied with come out of the matrix pipe
std::vector<int8_t> build_dw_ones_image();     // build_dw_mm_weights of an all-ones 3x3x16 filter: [filter row][lane][16 bytes], three equal rows
std::vector<int8_t> build_pw_ones_tile(int C); // fill_ones_tile over the (C + 63) / 64 k steps of a 1x1 product: [k step][lane][16 bytes], zero beyond C
void build_stem_rows(const int8_t *w /*[3][3][N]*/, int N, uint32_t wrow[3][8]);
void build_stem_mm(const int8_t *w /*[3][3][N]*/, int N, uint32_t *wmm /*[64][pitch]*/, int pitch);
std::vector<uint32_t> build_conv_rows_pack(const int8_t *w, bool depthwise, int KH, int KW, int C, int N, int KG, int NP);
inline std::vector<uint32_t> build_dw_c1_pack(const int8_t *w /*[KH][KW][N], N <= 8*/, int KH, int KW, int N, int KG) { return build_conv_rows_pack(w, true, KH, KW, 1, N, KG, 8); }
std::vector<uint32_t> build_conv_rows_mask(int RWB /* KW C */, int KG);

// TRANSPOSE_CONV split by output phase (k_tconv.hip): the phases of a filter at strides (sh, sw) in the order py sw + px, and the
// host-built operands of tconv_phase_rt (wimage.cpp)
struct TconvPhase {
    int py, px, Ty, Tx; // taps ky = py + sh t (t < Ty), kx = px + sw u (u < Tx); Ty = Tx = 0: the phase has no tap
    int KWCP, KS;       // Tx C rounded up to 16; 64-deep k steps over K' = Ty KWCP
};
std::vector<TconvPhase> tconv_phases(int KH, int KW, int C, int sh, int sw);
// the staged tile's geometry, one definition for tconv_plan (k_tconv.hip) and the host checks: base rows / pixels per image, most taps
// of a phase per column / row, the image's byte offset in a tile row, bytes per tile row; rows of a tile of bh base rows = bh + TYM - 1
struct TconvTile {
    int NBY, NBX, TYM, TXM, LP;
    long long ROW;
};
TconvTile tconv_tile(int W, int C, int KH, int KW, int sh, int sw, int OH, int OW, int padt, int padl);
std::vector<int8_t> build_tconv_phase_matrix(const int8_t *w /*[N][KH][KW][C]*/, int N, int KH, int KW, int C, int sh, int sw, const TconvPhase &p);
std::vector<int8_t> build_tconv_image(const int8_t *w /*[N][KH][KW][C]*/, int N, int KH, int KW, int C, int sh, int sw, int NTS);
std::vector<int32_t> build_tconv_kc(const int8_t *w /*[N][KH][KW][C]*/, int N, int KH, int KW, int C, int sh, int sw, int izp, int NT16);
std::vector<int> build_tconv_table(int KH, int KW, int C, int sh, int sw, int ROW);

// A Conv2D with dilation factors (k_conv_dil.hip): the geometry of a tile row staged in dw column-phase planes, one definition for
// conv_dil_plan and the host checks; and the tap / mask tables of conv_gemm_rt's K layout with the filter rows dh tile rows apart
struct ConvDilTile {
    int KWCP;          // KW C rounded up to 16
    int PL, LP;        // positions per plane; bytes in front of plane 0
    long long PP, ROW; // plane pitch, bytes per tile row
};
ConvDilTile conv_dil_tile(int W, int C, int KW, int sw, int dw, int OW, int padl);
long long conv_dil_column(const ConvDilTile &t, int C, int dw, int xe /* x + padl */);
void conv_dil_tables(int KH, int KW, int C, int dh, int ROW, std::vector<int> &tap, std::vector<uint32_t> &mask);

// A resize by (sy, .) + Conv2D on a tile of source rows (k_upconv.hip): the source row, relative to an output row's own, that tile row 0
// stands for, and the sy y-phase tap tables [py][KS][4]
int upconv_dmin(int padt, int sy);
std::vector<int> upconv_tables(int KH, int KW, int C, int sy, int padt, int ROW);

} // namespace wimage
} // namespace mf
