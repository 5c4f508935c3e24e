// The LDS plan of pool_fc_chain (k_pool_fc.hip: k::pool_fc_plan) without a GPU, linked against the built library.
//   pool_fc_plan H W C softmax N1 [N2 ...]   ->   "ok R lds xoff xbytes aoff abytes poff CGW NS NPASS NIT woff1 [woff2 ...]"  or  "none"
#include <cstdio>
#include <cstdlib>

#include "kernels.hpp"

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    mf::k::PoolFcArgs a{};
    const int H = atoi(argv[1]), W = atoi(argv[2]), C = atoi(argv[3]);
    a.P = H * W, a.C = C;
    a.c.softmax = atoi(argv[4]);
    a.c.L = argc - 5;
    if (a.c.L > mf::k::FC_CHAIN_MAX) return 2;
    int K = C;
    for (int l = 0; l < a.c.L; ++l) {
        a.c.l[l].K = K, a.c.l[l].N = atoi(argv[5 + l]);
        K = a.c.l[l].N;
    }
    if (!mf::k::pool_fc_plan(a)) {
        printf("none\n");
        return 0;
    }
    printf("ok %d %d %d %d %d %d %d %d %d %d %d", a.c.R, a.c.lds, a.c.xoff, a.c.xbytes, a.c.aoff, a.c.abytes, a.c.poff, a.CGW, a.NS, a.NPASS, a.NIT);
    for (int l = 0; l < a.c.L; ++l) printf(" %d", a.c.l[l].woff);
    printf("\n");
    return 0;
}
