// k::conv_grp_plan (k_conv_grp.hip) without a GPU, linked against the built library.
//   conv_grp_plan H W C N G K S same wz   ->   "GPT TPG SPAN KS PW NT NSL"  or  "none"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels.hpp"

int main(int argc, char **argv) {
    if (argc != 10) return 2;
    int v[9];
    for (int i = 0; i < 9; ++i) v[i] = atoi(argv[i + 1]);
    const int H = v[0], W = v[1], K = v[5], S = v[6], pad = v[7] ? (K - 1) / 2 : 0;
    const int OH = v[7] ? (H + S - 1) / S : (H - K) / S + 1, OW = v[7] ? (W + S - 1) / S : (W - K) / S + 1;
    mf::k::ConvGrpArgs a{};
    std::vector<int> tap, colch;
    if (!mf::k::conv_grp_plan(a, tap, colch, H, W, v[2], v[3], v[4], K, K, S, S, OH, OW, pad, pad, v[8] != 0)) return printf("none\n"), 0;
    return printf("%d %d %d %d %d %d %d\n", a.GPT, a.TPG, a.SPAN, a.g.KS, a.PW, a.g.NT, a.g.NSL), 0;
}
