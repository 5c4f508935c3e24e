// k_add.hip -- ADD (TFLite builtin 0) of two tensors with per-tensor quantisation.  The reference has no such operator; the contract
// is DESIGN section 2's (include/microflow_amd.h: mf_add_create):
//     ta = ca * f32(a - za),  tb = cb * f32(b - zb),  y = T::from(roundf((f32(zo) + ta) + tb)),  then the fused activation,
// every step an individually rounded f32 operation.  The constants are per-tensor, so a batch is ONE flat array of bytes and image
// boundaries do not matter.  No LDS, no barrier; the output may be exactly one of the inputs (every lane reads its bytes before it
// writes them), which is how the model runtime never needs a third buffer for a skip connection.
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

// 16 bytes per lane and operand (dword x 4 loads and stores), 64-bit offsets (524 288 x 36 864 bytes is past 2^32), a grid-stride loop
// over a grid sized from the CU count; the last partial 16-byte group goes through the byte path in the same launch.  Writes exactly
// bytes [0, n) of out.  a, b and out are not __restrict__: out may be a or b.
template <bool FMA> __global__ __launch_bounds__(256) void add_c16(const int8_t *a, const int8_t *b, int8_t *out, AddArgs p, size_t n) {
    const size_t n16 = n >> 4, tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    for (size_t i = tid; i < n16; i += stride) {
        const v4i va = *(const v4i *)(a + i * 16), vb = *(const v4i *)(b + i * 16);
        st_out_t<false>(out + i * 16, add_group<FMA>(va, vb, p));
    }
    const size_t t = n16 * 16 + tid; // at most 15 bytes, the first lanes of the grid
    if (t < n) {
        const uint32_t xi = p.xin4 & 0xffu, xo = p.xout4 & 0xffu;
        const uint32_t ua = (uint32_t)(uint8_t)a[t] ^ xi, ub = (uint32_t)(uint8_t)b[t] ^ xi;
        out[t] = (int8_t)(((uint32_t)add_one<FMA>(ua, ub, p) & 0xffu) ^ xo);
    }
}

// byte-wise, the text's form: any pointers (the set_generic route)
__global__ __launch_bounds__(256) void add_generic(const int8_t *a, const int8_t *b, int8_t *out, AddArgs p, size_t n) {
    const uint32_t xi = p.xin4 & 0xffu, xo = p.xout4 & 0xffu;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const uint32_t ua = (uint32_t)(uint8_t)a[i] ^ xi, ub = (uint32_t)(uint8_t)b[i] ^ xi;
        out[i] = (int8_t)(((uint32_t)add_one<false>(ua, ub, p) & 0xffu) ^ xo);
    }
}

void launch_add_c16(const int8_t *a, const int8_t *b, int8_t *out, const AddArgs &p, size_t n, int cus, bool fma, hipStream_t s) {
    // 8 blocks of 4 waves fill a CU's wave slots; fewer where the array is short (one block at least: the byte tail)
    const size_t want = ((n >> 4) + 255) / 256, cap = (size_t)(cus > 0 ? cus : 256) * 8;
    const size_t grid = want < 1 ? 1 : (want < cap ? want : cap);
    if (fma) MF_LAUNCH(add_c16<true>, dim3((unsigned)grid), dim3(256), 0, s, a, b, out, p, n);
    else MF_LAUNCH(add_c16<false>, dim3((unsigned)grid), dim3(256), 0, s, a, b, out, p, n);
}
void launch_add_generic(const int8_t *a, const int8_t *b, int8_t *out, const AddArgs &p, size_t n, hipStream_t s) {
    MF_LAUNCH(add_generic, dim3(grid_for(n)), dim3(256), 0, s, a, b, out, p, n);
}

} // namespace k
} // namespace mf
