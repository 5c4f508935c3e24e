// k_concat.hpp -- CONCATENATION's per-element arithmetic as device functions: one byte, one dword.  The contract is DESIGN section 2's
// (k_concat.hip states it); shared by the CONCATENATION kernels (k_concat.hip) and the side convolution + CONCATENATION launch
// (k_side_join.hip), so that there is ONE text of it.
#pragma once
#include "k_common.hpp"

namespace mf {
namespace k {

// One element of one input.  u: the stored byte with xin applied (kernels.hpp: ConcatArgs), 0 .. 255; c, kz: that input's constant and
// f32(off + z_i).  f32(u) - kz equals f32(x - z_i): both are integers below 2^24, so the f32 subtraction is exact and gives the i32
// difference's conversion bit for bit.  Then one multiplication, one addition, roundf, `as T` -- each rounded on its own.
__device__ __forceinline__ int concat_one(uint32_t u, float c, float kz, const ConcatArgs &p) {
    const float y = __fadd_rn(p.zo_f, __fmul_rn(c, __fsub_rn((float)u, kz)));
    float r = __fadd_rn(y, __builtin_copysignf(0x1.fffffep-2f, y)); // roundf, half away from zero (as add_one)
    r = (r != r) ? 0.0f : r;                                        // NaN converts to 0 like Rust's `as`, then the clamp
    return (int)__builtin_amdgcn_fmed3f(r, p.lo_f, p.hi_f);         // `as T`
}
// One dword of input a (B = false) or b (B = true).  A slice whose requantisation is the identity (copy_i) keeps its bytes: the
// formula gives y = x for every byte there, so this is a case of the text
template <bool B> __device__ __forceinline__ uint32_t concat_dword(uint32_t w, const ConcatArgs &p) {
    if (B ? p.copy_b : p.copy_a) return w;
    const float c = B ? p.cb : p.ca, kz = B ? p.kb : p.ka;
    w ^= p.xin4;
    const int q0 = concat_one(w & 0xffu, c, kz, p), q1 = concat_one((w >> 8) & 0xffu, c, kz, p);
    const int q2 = concat_one((w >> 16) & 0xffu, c, kz, p), q3 = concat_one(w >> 24, c, kz, p);
    return pack4(q0, q1, q2, q3) ^ p.xout4;
}

} // namespace k
} // namespace mf
