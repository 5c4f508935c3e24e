// The explicit-pad entries of the run-time-geometry planners (k::conv_rows_plan_pads, conv_mm_plan_pads, conv_gemm_plan_pads,
// dw_gemm_plan_pads) without a GPU, linked against the built library.
//   pad_conv_plan same dw H W C N KH KW S wz
//     every planner through its pad_same entry (SAME) and through its explicit entry with (padt, padl) = ((KH - 1) / 2, (KW - 1) / 2) and
//     SAME's OH, OW, on argument blocks that were zeroed first:  "<planner>=same|differ|none ..."  (none: both entries refuse)
//   pad_conv_plan pads dw H W C N KH KW S wz padt padl OH OW
//     the explicit entries alone:  "<planner> key=value ..."  or  "<planner> none", one line per planner
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kernels.hpp"

using namespace mf::k;

template <typename A> static A zeroed() {
    A a;
    std::memset((void *)&a, 0, sizeof(A));
    return a;
}
template <typename A> static const char *verdict(bool ok1, bool ok2, const A &a, const A &b, bool tables_equal) {
    if (!ok1 && !ok2) return "none";
    return ok1 == ok2 && std::memcmp((const void *)&a, (const void *)&b, sizeof(A)) == 0 && tables_equal ? "same" : "differ";
}

int main(int argc, char **argv) {
    if (argc < 11) return 2;
    const std::string mode = argv[1];
    int v[13] = {0};
    for (int i = 2; i < argc && i < 15; ++i) v[i - 2] = atoi(argv[i]);
    const bool dw = v[0] != 0, wz = v[8] != 0;
    const int H = v[1], W = v[2], C = v[3], N = v[4], KH = v[5], KW = v[6], S = v[7];
    if (mode == "same") {
        if (argc != 11) return 2;
        const int OH = (H + S - 1) / S, OW = (W + S - 1) / S, pt = (KH - 1) / 2, pl = (KW - 1) / 2;
        {
            ConvRowsArgs a = zeroed<ConvRowsArgs>(), b = zeroed<ConvRowsArgs>();
            const bool o1 = conv_rows_plan(a, H, W, C, N, KH, KW, S, S, OH, OW, true), o2 = conv_rows_plan_pads(b, H, W, C, N, KH, KW, S, S, OH, OW, pt, pl);
            printf("conv_rows=%s ", verdict(o1, o2, a, b, true));
        }
        {
            ConvMmArgs a = zeroed<ConvMmArgs>(), b = zeroed<ConvMmArgs>();
            std::vector<int> t1, t2;
            const bool o1 = conv_mm_plan(a, t1, H, W, C, N, KH, KW, S, S, OH, OW, true, wz, dw), o2 = conv_mm_plan_pads(b, t2, H, W, C, N, KH, KW, S, S, OH, OW, pt, pl, wz, dw);
            printf("conv_mm=%s ", verdict(o1, o2, a, b, t1 == t2));
        }
        {
            ConvGemmArgs a = zeroed<ConvGemmArgs>(), b = zeroed<ConvGemmArgs>();
            std::vector<int> t1, t2;
            std::vector<uint32_t> m1, m2;
            const bool o1 = conv_gemm_plan(a, t1, m1, H, W, C, N, KH, KW, S, S, OH, OW, true, wz), o2 = conv_gemm_plan_pads(b, t2, m2, H, W, C, N, KH, KW, S, S, OH, OW, pt, pl, wz);
            printf("conv_gemm=%s ", verdict(o1, o2, a, b, t1 == t2 && m1 == m2));
        }
        {
            DwGemmArgs a = zeroed<DwGemmArgs>(), b = zeroed<DwGemmArgs>();
            const bool o1 = dw_gemm_plan(a, H, W, C, KH, KW, S, S, OH, OW, true), o2 = dw_gemm_plan_pads(b, H, W, C, KH, KW, S, S, OH, OW, pt, pl);
            printf("dw_gemm=%s\n", verdict(o1, o2, a, b, true));
        }
        return 0;
    }
    if (mode != "pads" || argc != 15) return 2;
    const int pt = v[9], pl = v[10], OH = v[11], OW = v[12];
    {
        ConvRowsArgs a = zeroed<ConvRowsArgs>();
        if ((!dw || C == 1) && conv_rows_plan_pads(a, H, W, C, N, KH, KW, S, S, OH, OW, pt, pl, true)) // (as the PAD + convolution group asks)
            printf("conv_rows shy=%d XO=%d X0=%d TWP=%d TILE=%d KG=%d G=%d\n", a.shy, a.XO, a.X0, a.TWP, a.TILE, a.KG, a.G);
        else printf("conv_rows none\n");
    }
    {
        ConvMmArgs a = zeroed<ConvMmArgs>();
        std::vector<int> t;
        if (conv_mm_plan_pads(a, t, H, W, C, N, KH, KW, S, S, OH, OW, pt, pl, wz, dw))
            printf("conv_mm padt=%d padl=%d LP=%d ROW=%d RB=%d TILE=%d G=%d BH=%d NBANDS=%d NTHR=%d\n", a.padt, a.padl, a.LP, a.ROW, a.RB, a.TILE, a.G, a.BH, a.NBANDS, a.NTHR);
        else printf("conv_mm none\n");
    }
    {
        ConvGemmArgs a = zeroed<ConvGemmArgs>();
        std::vector<int> t;
        std::vector<uint32_t> m;
        if (!dw && conv_gemm_plan_pads(a, t, m, H, W, C, N, KH, KW, S, S, OH, OW, pt, pl, wz))
            printf("conv_gemm padt=%d padl=%d LP=%d ROW=%d RB=%d TILE=%d G=%d BH=%d NBANDS=%d\n", a.padt, a.padl, a.LP, a.ROW, a.RB, a.TILE, a.G, a.BH, a.NBANDS);
        else printf("conv_gemm none\n");
    }
    {
        DwGemmArgs a = zeroed<DwGemmArgs>();
        if (dw && dw_gemm_plan_pads(a, H, W, C, KH, KW, S, S, OH, OW, pt, pl))
            printf("dw_gemm padt=%d padl=%d LP=%d ROW=%d RB=%d TILE=%d G=%d BH=%d NBANDS=%d\n", a.padt, a.padl, a.LP, a.ROW, a.RB, a.TILE, a.G, a.BH, a.NBANDS);
        else printf("dw_gemm none\n");
    }
    return 0;
}
