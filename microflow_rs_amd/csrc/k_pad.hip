// k_pad.hip -- PAD (TFLite builtin 34) of a rank-4 tensor in H and W.  The reference has no such operator; the contract is DESIGN
// section 2's (include/microflow_amd.h: mf_pad_create): the output is the input with `top` / `bottom` rows and `left` / `right`
// columns of new elements around every image, each new element the tensor's zero point as a value of T.  No arithmetic: input and
// output carry the same quantisation, so the kernels move bytes and know the zero point only as the stored fill byte (for u8 the
// internal domain's, zp ^ 0x80).  No LDS, no barrier, one grid pass; every output byte is written exactly once, the fill as a
// splatted constant that is never read from memory.
#include "k_common.hpp"

namespace mf {
namespace k {

// Any shape, any pointers: one output byte per thread and step (the set_generic route, and C % 4 != 0).
__global__ __launch_bounds__(256) void pad_generic(const int8_t *__restrict__ in, int8_t *__restrict__ out, PadArgs p, size_t total) {
    const size_t out_row = (size_t)p.out_row, in_row = (size_t)p.in_row, lp = (size_t)p.lp;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t row = i / out_row, b = i - row * out_row;
        const size_t img = row / (size_t)p.OH, oy = row - img * (size_t)p.OH;
        int8_t v = (int8_t)(p.fill4 & 0xffu);
        if (oy >= (size_t)p.top && oy < (size_t)(p.top + p.H) && b >= lp && b < lp + in_row)
            v = in[(img * (size_t)p.H + (oy - (size_t)p.top)) * in_row + (b - lp)];
        out[i] = v;
    }
}

// The word kernel: an output row is whole words of V (a dword, or 16 bytes) in each of its three segments -- left fill, image row,
// right fill -- so a word is either fill or one aligned word of the input.  One word per thread and step; I is the index type: 32 bits
// wherever the output has fewer than 2^32 words (the divisions are the cost of the address), else 64.  Reads only words
// [0, batch * H * in_row / sizeof(V)) of in, writes exactly words [0, total) of out.
template <typename V, typename I> __global__ __launch_bounds__(256) void pad_c4(const int8_t *__restrict__ in, int8_t *__restrict__ out, PadArgs p, I total) {
    const I wpr = (I)(p.out_row / (int)sizeof(V)), lpw = (I)(p.lp / (int)sizeof(V)), irw = (I)(p.in_row / (int)sizeof(V));
    const I OH = (I)p.OH, H = (I)p.H, top = (I)p.top;
    V fill;
    if constexpr (sizeof(V) == 16) fill = V{(int)p.fill4, (int)p.fill4, (int)p.fill4, (int)p.fill4};
    else fill = (V)p.fill4;
    for (I i = (I)blockIdx.x * 256 + threadIdx.x; i < total; i += (I)gridDim.x * 256) {
        const I row = i / wpr, w = i - row * wpr;
        const I img = row / OH, oy = row - img * OH;
        V v = fill;
        if (oy >= top && oy < top + H && w >= lpw && w < lpw + irw) v = ((const V *)in)[(img * H + (oy - top)) * irw + (w - lpw)];
        ((V *)out)[i] = v;
    }
}

void launch_pad_generic(const int8_t *in, int8_t *out, const PadArgs &a, size_t batch, hipStream_t s) {
    const size_t total = batch * (size_t)a.OH * (size_t)a.out_row;
    MF_LAUNCH(pad_generic, dim3(grid_for(total)), dim3(256), 0, s, in, out, a, total);
}

template <typename V> static void launch_pad_words(const int8_t *in, int8_t *out, const PadArgs &a, size_t batch, hipStream_t s) {
    const size_t total = batch * (size_t)a.OH * (size_t)(a.out_row / (int)sizeof(V));
    // (a grid-stride step adds at most 2048 x 256 to an index below `total`: the 32-bit form stops short of where that could wrap)
    if (total < 0xfff00000ull) MF_LAUNCH((pad_c4<V, uint32_t>), dim3(grid_for(total)), dim3(256), 0, s, in, out, a, (uint32_t)total);
    else MF_LAUNCH((pad_c4<V, size_t>), dim3(grid_for(total)), dim3(256), 0, s, in, out, a, total);
}
void launch_pad_c4(const int8_t *in, int8_t *out, const PadArgs &a, size_t batch, int unit, hipStream_t s) {
    if (unit == 16) launch_pad_words<v4i>(in, out, a, batch, s);
    else launch_pad_words<uint32_t>(in, out, a, batch, s);
}

} // namespace k
} // namespace mf
