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

} // namespace wimage
} // namespace mf
