// k_pair_band_body.hpp -- what the band-by-band pair kernels share: pair_band_rt (k_pair_band.hip: 1, 2 or 4 k steps) and
// pair_band_deep_rt (k_pair_band_deep.hip: 8 k steps).  The operand structs are here; the kernel body is k_pair_band_body.inc.
// The structure (step, tile, halo, the two phases, the two barriers) is described at the top of k_pair_band.hip.
#pragma once
#include "k_common.hpp"

namespace mf {
namespace k {

namespace {
struct BDwW { // depthwise operands of one 16-channel group
    v4i A[3];
    float4 a, s;
    int4 k;
};
template <int KSC> struct BPwW { // pointwise operands of one block of (at most two) output tiles
    v4i A[2][KSC];
    float4 a[2], s[2];
    int4 k[2];
};
} // namespace

} // namespace k
} // namespace mf
