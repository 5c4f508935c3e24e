// k_concat.hip -- CONCATENATION (TFLite builtin 2) of two tensors along the last axis, with per-tensor quantisation.  The reference has
// no such operator; the contract is DESIGN section 2's (include/microflow_amd.h: mf_concatenation_create): output row r is row r of a
// (Ca elements) followed by row r of b (Cb elements), each element of input i requantised as
//     y = T::from(roundf(f32(zo) + c_i * f32(x - z_i))),   c_i = s_i / so,
// every step an individually rounded f32 operation.  Where s_i is bit-equal to so and z_i == zo that is y = x, and the slice is copied
// (ConcatArgs::copy_a / copy_b, set by the host).  No LDS, no barrier, one grid pass; every output byte is written exactly once.  The
// output overlaps neither input (the row pitches differ, so nothing can be done in place).
#include "k_concat.hpp"

namespace mf {
namespace k {

template <bool B> __device__ __forceinline__ uint32_t concat_word(uint32_t w, const ConcatArgs &p) { return concat_dword<B>(w, p); }
template <bool B> __device__ __forceinline__ uint2 concat_word(uint2 w, const ConcatArgs &p) {
    return make_uint2(concat_dword<B>(w.x, p), concat_dword<B>(w.y, p));
}
template <bool B> __device__ __forceinline__ v4i concat_word(v4i w, const ConcatArgs &p) {
    return v4i{(int)concat_dword<B>((uint32_t)w.x, p), (int)concat_dword<B>((uint32_t)w.y, p), (int)concat_dword<B>((uint32_t)w.z, p),
               (int)concat_dword<B>((uint32_t)w.w, p)};
}

// The word kernel: Ca and Cb are whole words of V (16, 8 or 4 bytes) and all three pointers are aligned to V, so an output word is one
// aligned word of a or of b.  A grid-stride loop over (row, word) with 64-bit offsets (524 288 rows x 512 bytes is past 2^31); the
// grid is sized from the CU count.  Reads words [0, rows * Ca / sizeof(V)) of a and [0, rows * Cb / sizeof(V)) of b, writes exactly
// words [0, total) of out.
template <typename V> __global__ __launch_bounds__(256) void concat_c4(const int8_t *__restrict__ a, const int8_t *__restrict__ b, int8_t *__restrict__ out, ConcatArgs p, size_t total) {
    const size_t wa = (size_t)(p.Ca / (int)sizeof(V)), wb = (size_t)(p.Cb / (int)sizeof(V)), wpr = wa + wb;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t row = i / wpr, w = i - row * wpr;
        V v;
        if (w < wa) v = concat_word<false>(((const V *)a)[row * wa + w], p);
        else v = concat_word<true>(((const V *)b)[row * wb + (w - wa)], p);
        ((V *)out)[i] = v;
    }
}

// byte-wise, the text's form: any Ca, Cb and pointers (the set_generic route)
__global__ __launch_bounds__(256) void concat_generic(const int8_t *__restrict__ a, const int8_t *__restrict__ b, int8_t *__restrict__ out, ConcatArgs p, size_t total) {
    const size_t Ca = (size_t)p.Ca, Cb = (size_t)p.Cb, pitch = Ca + Cb;
    const uint32_t xi = p.xin4 & 0xffu, xo = p.xout4 & 0xffu;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t row = i / pitch, c = i - row * pitch;
        const bool from_b = c >= Ca;
        const uint32_t u = (uint32_t)(uint8_t)(from_b ? b[row * Cb + (c - Ca)] : a[row * Ca + c]);
        uint32_t y = u;
        if (!(from_b ? p.copy_b : p.copy_a)) y = ((uint32_t)concat_one(u ^ xi, from_b ? p.cb : p.ca, from_b ? p.kb : p.ka, p) & 0xffu) ^ xo;
        out[i] = (int8_t)y;
    }
}

template <typename V> static void launch_concat_words(const int8_t *a, const int8_t *b, int8_t *out, const ConcatArgs &p, size_t rows, int cus, hipStream_t s) {
    const size_t total = rows * (size_t)((p.Ca + p.Cb) / (int)sizeof(V));
    // 8 blocks of 4 waves fill a CU's wave slots; fewer where the tensor is short
    const size_t want = (total + 255) / 256, cap = (size_t)(cus > 0 ? cus : 256) * 8;
    const size_t grid = want < 1 ? 1 : (want < cap ? want : cap);
    MF_LAUNCH((concat_c4<V>), dim3((unsigned)grid), dim3(256), 0, s, a, b, out, p, total);
}
void launch_concat_c4(const int8_t *a, const int8_t *b, int8_t *out, const ConcatArgs &p, size_t rows, int unit, int cus, hipStream_t s) {
    if (unit == 16) launch_concat_words<v4i>(a, b, out, p, rows, cus, s);
    else if (unit == 8) launch_concat_words<uint2>(a, b, out, p, rows, cus, s);
    else launch_concat_words<uint32_t>(a, b, out, p, rows, cus, s);
}
void launch_concat_generic(const int8_t *a, const int8_t *b, int8_t *out, const ConcatArgs &p, size_t rows, hipStream_t s) {
    const size_t total = rows * ((size_t)p.Ca + (size_t)p.Cb);
    MF_LAUNCH(concat_generic, dim3(grid_for(total)), dim3(256), 0, s, a, b, out, p, total);
}

} // namespace k
} // namespace mf
