// k_add.hpp -- ADD's arithmetic as device functions: one element, one dword, one 16-byte group.  The contract is DESIGN section 2's
// (k_add.hip states it); shared by the ADD kernels (k_add.hip) and the shortcut convolution + ADD launch (k_side_join.hip), so that
// there is ONE text of it.
#pragma once
#include "k_common.hpp"

namespace mf {
namespace k {

// One element.  ua, ub: the stored bytes with xin applied (kernels.hpp: AddArgs), 0 .. 255.  f32(u) - ka equals f32(v - za): the
// operands are integers below 2^24, so this f32 subtraction is exact and gives the i32 difference's conversion bit for bit
// (v_cvt_f32_ubyteN + v_sub_f32 instead of a byte extract, an integer subtract and a conversion).
//
// FMA: the gated form -- two conversions, two fused multiply-adds with the zero points folded into k1 on the host, the same rounding
// and clamp.  Its roundings differ from the text's, so it runs only for an operator whose constants the host checked over ALL 65 536
// (ua, ub) pairs to give the same byte (hostmath.cpp: h_add_fma_form, which also requires finite constants: no NaN can arise).
template <bool FMA> __device__ __forceinline__ int add_one(uint32_t ua, uint32_t ub, const AddArgs &p) {
    float y;
    if constexpr (FMA) {
        y = __fmaf_rn(p.cb, (float)ub, __fmaf_rn(p.ca, (float)ua, p.k1));
    } else {
        const float ta = __fmul_rn(p.ca, __fsub_rn((float)ua, p.ka));
        const float tb = __fmul_rn(p.cb, __fsub_rn((float)ub, p.kb));
        y = __fadd_rn(__fadd_rn(p.zo_f, ta), tb);
    }
    float r = __fadd_rn(y, __builtin_copysignf(0x1.fffffep-2f, y)); // roundf, half away from zero (as requant_any)
    if constexpr (!FMA) r = (r != r) ? 0.0f : r;                    // NaN converts to 0 like Rust's `as`, then the clamp
    return (int)__builtin_amdgcn_fmed3f(r, p.lo_f, p.hi_f);         // `as T` and the activation: one clamp
}
template <bool FMA> __device__ __forceinline__ uint32_t add_dword(uint32_t wa, uint32_t wb, const AddArgs &p) {
    wa ^= p.xin4, wb ^= p.xin4;
    const int q0 = add_one<FMA>(wa & 0xffu, wb & 0xffu, p), q1 = add_one<FMA>((wa >> 8) & 0xffu, (wb >> 8) & 0xffu, p);
    const int q2 = add_one<FMA>((wa >> 16) & 0xffu, (wb >> 16) & 0xffu, p), q3 = add_one<FMA>(wa >> 24, wb >> 24, p);
    return pack4(q0, q1, q2, q3) ^ p.xout4;
}

template <bool FMA> __device__ __forceinline__ uint4 add_group(v4i va, v4i vb, const AddArgs &p) {
    uint4 r;
    r.x = add_dword<FMA>((uint32_t)va.x, (uint32_t)vb.x, p), r.y = add_dword<FMA>((uint32_t)va.y, (uint32_t)vb.y, p);
    r.z = add_dword<FMA>((uint32_t)va.z, (uint32_t)vb.z, p), r.w = add_dword<FMA>((uint32_t)va.w, (uint32_t)vb.w, p);
    return r;
}

} // namespace k
} // namespace mf
