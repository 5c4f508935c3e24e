// k_add.hip -- ADD (TFLite builtin 0) of two tensors with per-tensor quantisation.  The reference has no such operator; the contract
// is DESIGN section 2's (include/microflow_amd.h: mf_add_create):
//     ta = ca * f32(a - za),  tb = cb * f32(b - zb),  y = T::from(roundf((f32(zo) + ta) + tb)),  then the fused activation,
// every step an individually rounded f32 operation.  The constants are per-tensor, so a batch is ONE flat array of bytes and image
// boundaries do not matter.  No LDS, no barrier; the output may be exactly one of the inputs (every lane reads its bytes before it
// writes them), which is how the model runtime never needs a third buffer for a skip connection.
#include "k_add.hpp"

namespace mf {
namespace k {

// (one element, one dword, one 16-byte group: add_one, add_dword, add_group -- k_add.hpp)
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
