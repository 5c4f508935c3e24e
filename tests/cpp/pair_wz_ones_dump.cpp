// Prints pair_wz_rt's two ones images (microflow_rs_amd/csrc/wimage.cpp: build_dw_ones_image, build_pw_ones_tile) as hex, one line
// per image: `name shape hex`.  tests/test_pair_wz_host.py builds this with the address and undefined-behaviour sanitizers and checks
// the bytes: `dw_ones` against `dw_mm_of_ones` (build_dw_mm_weights of an all-ones 3x3x16 filter, built here) and both against the
// map of the matrix instruction's operand A.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../microflow_rs_amd/csrc/wimage.hpp"

using namespace mf::wimage;

static void line(const char *name, int shape, const std::vector<int8_t> &v) {
    printf("%s %d ", name, shape);
    for (int8_t b : v) printf("%02x", (unsigned)(uint8_t)b);
    printf("\n");
}

int main() {
    line("dw_ones", 16, build_dw_ones_image());
    line("dw_mm_of_ones", 16, build_dw_mm_weights(std::vector<int8_t>((size_t)9 * 16, 1).data(), 16));
    for (int C : {16, 48, 80, 128, 192, 256}) line("pw_ones", C, build_pw_ones_tile(C));
    return 0;
}
