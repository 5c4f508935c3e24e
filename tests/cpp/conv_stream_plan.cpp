// The class of conv_stream_rt (k_conv_stream.hip: k::conv_stream_plan) without a GPU, linked against the built library.
//   conv_stream_plan H W C N KH KW sh sw OH OW padt padl dh dw groups depthwise wz finite   ->   "ok K min_rows tile_at_65536_rows"  or  "none"
#include <cstdio>
#include <cstdlib>

#include "kernels.hpp"

int main(int argc, char **argv) {
    if (argc != 19) return 2;
    int v[18];
    for (int i = 0; i < 18; ++i) v[i] = atoi(argv[i + 1]);
    mf::k::ConvStreamSpec s{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11]};
    s.dh = v[12], s.dw = v[13], s.groups = v[14], s.depthwise = v[15] != 0, s.wz = v[16] != 0, s.finite = v[17] != 0;
    mf::k::ConvStreamArgs a{};
    if (!mf::k::conv_stream_plan(a, s)) {
        printf("none\n");
        return 0;
    }
    printf("ok %d %d %d\n", a.K, a.min_rows, mf::k::conv_stream_tile(a, 65536));
    return 0;
}
