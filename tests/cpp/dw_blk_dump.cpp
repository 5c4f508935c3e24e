// Writes the block-form operands of microflow_rs_amd/csrc/wimage.cpp for weights read from a file:
//     dw_blk_dump dw C  weights.bin out.bin     build_dw_blk_weights of [3][3][C] int8 -> [C/4][64 lanes][16 bytes]
//     dw_blk_dump pw N  weights.bin out.bin     build_pw_iso_weights of [N][8] int8    -> [4][N/16][64 lanes][8 bytes]
// tests/test_dw_block_host.py builds this with the address and undefined-behaviour sanitizers and multiplies the operands in numpy.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../microflow_rs_amd/csrc/wimage.hpp"

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const bool dw = !strcmp(argv[1], "dw");
    const int n = atoi(argv[2]);
    const size_t want = dw ? (size_t)9 * n : (size_t)8 * n;
    std::vector<int8_t> w(want);
    FILE *f = fopen(argv[3], "rb");
    if (!f || fread(w.data(), 1, want, f) != want) return 3;
    fclose(f);
    const std::vector<int8_t> out = dw ? mf::wimage::build_dw_blk_weights(w.data(), n) : mf::wimage::build_pw_iso_weights(w.data(), n);
    f = fopen(argv[4], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) return 4;
    fclose(f);
    return 0;
}
