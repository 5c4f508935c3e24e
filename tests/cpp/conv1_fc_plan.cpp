// The plan of conv1_fc_rt (k_conv1_fc.hip: k::conv1_fc_plan) without a GPU, linked against the built library.
//   conv1_fc_plan H W N KH KW sh sw same NFC [wz [finite]]
//     ->   "ok BH NB KS NT lds wres PP NRT KSC XO PITCH TROWS TILE BP toff tbytes boff qoff aoff poff"   or   "none"
#include <cstdio>
#include <cstdlib>

#include "kernels.hpp"

int main(int argc, char **argv) {
    if (argc < 10) return 2;
    mf::k::Conv1FcArgs a{};
    a.H = atoi(argv[1]), a.W = atoi(argv[2]), a.N = atoi(argv[3]), a.KH = atoi(argv[4]), a.KW = atoi(argv[5]);
    a.sh = atoi(argv[6]), a.sw = atoi(argv[7]), a.pad_same = atoi(argv[8]);
    if (a.sh < 1 || a.sw < 1) return 2;
    a.OH = a.pad_same ? (a.H + a.sh - 1) / a.sh : (a.H - a.KH) / a.sh + 1;
    a.OW = a.pad_same ? (a.W + a.sw - 1) / a.sw : (a.W - a.KW) / a.sw + 1;
    a.fc.N = atoi(argv[9]), a.fc.K = a.OH * a.OW * a.N;
    a.wz = argc > 10 ? atoi(argv[10]) : 0;
    a.finite = argc > 11 ? atoi(argv[11]) : 1;
    if (!mf::k::conv1_fc_plan(a)) {
        printf("none\n");
        return 0;
    }
    printf("ok %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", a.BH, a.NB, a.fc.KS, a.fc.NT, a.lds, a.wres, a.PP, a.NRT, a.KSC, a.XO,
           a.PITCH, a.TROWS, a.TILE, a.BP, a.toff, a.tbytes, a.boff, a.qoff, a.aoff, a.poff);
    return 0;
}
