// The plan of conv_pool_rt (k_conv_pool.hip: k::conv_pool_plan) without a GPU, linked against the built library.
//   conv_pool_plan H W C N KH KW S same wz PFH PFW PS pool_same
//     ->  "ok key=value ... band=py0:py1:c0:c1 ..."  or  "none"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels.hpp"

int main(int argc, char **argv) {
    if (argc != 14) return 2;
    int v[13];
    for (int i = 0; i < 13; ++i) v[i] = atoi(argv[i + 1]);
    const int H = v[0], W = v[1], C = v[2], N = v[3], KH = v[4], KW = v[5], S = v[6], same = v[7], wz = v[8], PFH = v[9], PFW = v[10], PS = v[11], psame = v[12];
    auto out_size = [](int in, int k, int s, int sm) { return sm ? (in + s - 1) / s : (in - k) / s + 1; };
    const int OH = out_size(H, KH, S, same), OW = out_size(W, KW, S, same);
    const int POH = out_size(OH, PFH, PS, psame), POW = out_size(OW, PFW, PS, psame);
    mf::k::ConvPoolArgs a{};
    std::vector<int> tap;
    std::vector<uint32_t> mask;
    if (!mf::k::conv_pool_plan(a, tap, mask, H, W, C, N, KH, KW, S, S, OH, OW, same != 0, wz != 0, PFH, PFW, PS, PS, POH, POW, psame != 0)) {
        printf("none\n");
        return 0;
    }
    printf("ok OH=%d OW=%d POH=%d POW=%d KS=%d NT=%d TB=%d LP=%d ROW=%d RB=%d TILE=%d NP=%d CB=%d YIMG=%d G=%d PB=%d NB=%d xoff=%d yoff=%d toff=%d moff=%d coff=%d lds=%d pshy=%d ntap=%zu nmask=%zu",
           a.OH, a.OW, a.POH, a.POW, a.KS, a.NT, a.TB, a.LP, a.ROW, a.RB, a.TILE, a.NP, a.CB, a.YIMG, a.G, a.PB, a.NB, a.xoff, a.yoff, a.toff, a.moff, a.coff, a.lds, a.pshy,
           tap.size(), mask.size());
    for (int b = 0; b < a.NB; ++b) {
        int py0, py1, c0, c1;
        mf::k::conv_pool_band(a.OH, a.POH, a.PB, a.psh, a.pshy, a.PFH, b, py0, py1, c0, c1);
        printf(" band=%d:%d:%d:%d", py0, py1, c0, c1);
    }
    printf("\n");
    return 0;
}
