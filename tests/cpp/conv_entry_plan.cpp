// The plans of the two kernels that take a Conv2D-stem model's f32 input (k_rt.hip: k::conv_rows_plan; k_conv_gemm.hip:
// k::conv_gemm_plan) without a GPU, linked against the built library.
//   conv_entry_plan H W C N KH KW S same   ->   "rows G TILE lds"  or  "gemm NSL NBANDS G ROWB lds"  or  "none"
// (the order of ops.hip's routes: conv_rows_lds where its plan takes the shape, else conv_gemm_rt)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels.hpp"

int main(int argc, char **argv) {
    if (argc != 9) return 2;
    const int H = atoi(argv[1]), W = atoi(argv[2]), C = atoi(argv[3]), N = atoi(argv[4]), KH = atoi(argv[5]), KW = atoi(argv[6]), S = atoi(argv[7]);
    const bool same = atoi(argv[8]) != 0;
    if (S < 1 || H < KH || W < KW) return 2;
    const int OH = same ? (H + S - 1) / S : (H - KH) / S + 1, OW = same ? (W + S - 1) / S : (W - KW) / S + 1;
    mf::k::ConvRowsArgs r{};
    if (mf::k::conv_rows_plan(r, H, W, C, N, KH, KW, S, S, OH, OW, same)) {
        printf("rows %d %d %d\n", r.G, r.TILE, mf::k::conv_rows_lds_bytes(r));
        return 0;
    }
    mf::k::ConvGemmArgs g{};
    std::vector<int> tap;
    std::vector<uint32_t> mask;
    if (mf::k::conv_gemm_plan(g, tap, mask, H, W, C, N, KH, KW, S, S, OH, OW, same, false)) {
        printf("gemm %d %d %d %d %d\n", g.NSL, g.NBANDS, g.G, W * C, g.lds);
        return 0;
    }
    printf("none\n");
    return 0;
}
