// k_resize.hip -- RESIZE_NEAREST_NEIGHBOR (TFLite builtin 97; Keras' UpSampling2D) of a rank-4 tensor by integer factors (sy, sx).  The
// reference has no such operator; the contract is include/microflow_amd.h's (mf_resize_nearest_create): out[oy][ox][c] =
// in[oy / sy][ox / sx][c].  No arithmetic: input and output carry the same quantisation, so the kernels move bytes (the u8 internal
// domain flips both sides alike).  No LDS, no barrier, one grid pass; every output byte is written exactly once.
#include "k_common.hpp"

namespace mf {
namespace k {

// Any shape, any pointers: one output byte per thread and step (the set_generic route, and C % 4 != 0).
__global__ __launch_bounds__(256) void resize_nn_generic(const int8_t *__restrict__ in, int8_t *__restrict__ out, ResizeArgs p, size_t total) {
    const size_t C = (size_t)p.C, OW = (size_t)p.W * p.sx, OH = (size_t)p.H * p.sy;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t c = i % C, px = i / C;
        const size_t ox = px % OW, row = px / OW;
        const size_t oy = row % OH, img = row / OH;
        out[i] = in[((img * (size_t)p.H + oy / (size_t)p.sy) * (size_t)p.W + ox / (size_t)p.sx) * C + c];
    }
}

// The word kernel: a pixel is whole words of V (a dword, or 16 bytes).  One SOURCE word per thread and step: loaded once, stored sx times
// along the row and that sy times down the rows, all from the same register -- so the sy output rows of a source row come from the
// same workgroup.  Reads exactly words [0, total) of in; writes words of out below total * sy * sx, each once.
template <typename V> __global__ __launch_bounds__(256) void resize_nn_c4(const int8_t *__restrict__ in, int8_t *__restrict__ out, ResizeArgs p, size_t total) {
    const size_t wpp = (size_t)p.C / sizeof(V), wpr = wpp * (size_t)p.W, owpr = wpr * (size_t)p.sx; // words per pixel, source row, output row
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const V v = ((const V *)in)[i];
        const size_t row = i / wpr, w = i - row * wpr; // (row counts source rows over the whole batch: image * H + y)
        const size_t x = w / wpp, cw = w - x * wpp;
        V *dst = (V *)out + row * (size_t)p.sy * owpr + x * (size_t)p.sx * wpp + cw;
        for (int ry = 0; ry < p.sy; ++ry)
            for (int rx = 0; rx < p.sx; ++rx) dst[(size_t)ry * owpr + (size_t)rx * wpp] = v;
    }
}

void launch_resize_generic(const int8_t *in, int8_t *out, const ResizeArgs &a, size_t batch, hipStream_t s) {
    const size_t total = batch * (size_t)a.H * a.sy * (size_t)a.W * a.sx * (size_t)a.C;
    MF_LAUNCH(resize_nn_generic, dim3(grid_for(total)), dim3(256), 0, s, in, out, a, total);
}

void launch_resize_c4(const int8_t *in, int8_t *out, const ResizeArgs &a, size_t batch, int unit, hipStream_t s) {
    const size_t total = batch * (size_t)a.H * (size_t)a.W * (size_t)(a.C / unit);
    if (unit == 16) MF_LAUNCH((resize_nn_c4<v4i>), dim3(grid_for(total)), dim3(256), 0, s, in, out, a, total);
    else MF_LAUNCH((resize_nn_c4<uint32_t>), dim3(grid_for(total)), dim3(256), 0, s, in, out, a, total);
}

} // namespace k
} // namespace mf
