// The band plan of pair_band_deep_rt (k_pair_band_deep.hip: k::pair_band_deep_plan) without a GPU, linked against the built library.
//   pair_band_deep_plan H W C S N   ->   "ok RB NB TR ROW TILE dbuf tile_off mid_off mid_bytes q_off lds wgs CX CY UX UY NCH TB NBLK SLOTS NWB KSC"  or  "none"
#include <cstdio>
#include <cstdlib>

#include "kernels.hpp"

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    const int H = atoi(argv[1]), W = atoi(argv[2]), C = atoi(argv[3]), S = atoi(argv[4]), N = atoi(argv[5]);
    if (S < 1) return 2;
    mf::k::PairBandArgs a{};
    if (!mf::k::pair_band_deep_plan(mf::k::ChainGeom{H, W, C, S, (H + S - 1) / S, (W + S - 1) / S, N, 0u}, a)) {
        printf("none\n");
        return 0;
    }
    printf("ok %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", a.RB, a.NB, a.TR, a.ROW, a.TILE, a.dbuf, a.tile_off, a.mid_off, a.mid_bytes, a.q_off,
           a.lds_bytes, a.wgs, 1 << a.lgCX, 1 << a.lgCY, a.UX, a.UY, a.NCH, a.TB, a.NBLK, a.SLOTS, a.NWB, a.KSC);
    return 0;
}
