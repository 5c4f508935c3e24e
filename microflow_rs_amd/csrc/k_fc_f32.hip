// k_fc_f32.hip -- M::predict's boundary conversions inside a model's first and last launch (microflow-macros/src/lib.rs:188-191:
// Tensor::quantize of the f32 input, predict_inner, .dequantize()), for the launches whose input rows / output patch pass through LDS:
// fc_rt and fc_chain (k_fc_rt.hip) at either end, pool_fc_chain (k_pool_fc.hip) at the exit.  The kernels are those files' bodies
// (k_fc_rt_body.hpp, k_pool_fc_body.hpp) with EDGE != 0:
//
//   entry : the step's rows [r0 K, r1 K) are FLOATS; they are loaded 16 bytes at a time (r0 is a multiple of 16, so each step starts
//           on a 16-byte boundary of a 16-byte aligned input; the last K (r1 - r0) % 4 floats singly), quantised with quantize_f32's
//           arithmetic value by value (k_fc_layer.hpp edge_quant; a u8 model gets the internal byte directly) and written to the row
//           buffer from its first byte on.  Only floats inside rows x K are read; everything behind the staging is unchanged.
//   exit  : the step's patch of int8 results leaves as floats, scale * (f32(q) - zp) (dequantize_i8's expression), 4 bytes per thread
//           and store; nothing outside rows x N floats is written.
//
// Both conversions need round-to-nearest: only epilogue modes 0 .. 2 exist here (these launches have no mode 3 anyway).
#include <algorithm>

#include "k_fc_rt_body.hpp"
#include "k_pool_fc_body.hpp"

namespace mf {
namespace k {

template <int AL, int MG, uint32_t XR4, int EDGE>
__global__ __launch_bounds__(256) void fc_rt_f32(const int8_t *__restrict__ in, int8_t *__restrict__ out, FcRtArgs p, F32Edge eg, long long rows) {
    static_assert(MG <= 2 && EDGE >= 1 && EDGE <= 3, "both conversions need round-to-nearest: no single-fma epilogue here");
    fc_rt_body<AL, MG, XR4, EDGE>(in, out, p, rows, eg);
}

template <int MG, uint32_t XR4, int EDGE>
__global__ __launch_bounds__(256) void fc_chain_f32(const int8_t *__restrict__ in, int8_t *__restrict__ out, FcChainArgs p, F32Edge eg, long long rows) {
    static_assert(MG <= 2 && EDGE >= 1 && EDGE <= 3, "both conversions need round-to-nearest: no single-fma epilogue here");
    fc_chain_body<MG, XR4, EDGE>(in, out, p, rows, eg);
}

template <int MG, uint32_t XR4>
__global__ __launch_bounds__(256) void pool_fc_chain_f32(const int8_t *__restrict__ in, int8_t *__restrict__ out, PoolFcArgs p, F32Edge eg, long long rows) {
    static_assert(MG <= 2, "the dequantisation needs round-to-nearest: no single-fma epilogue here");
    pool_fc_body<MG, XR4, true>(in, out, p, rows, eg);
}

// ---- host side (geometry as the int8 launchers') ---------------------------------------------------------------------
template <int EDGE, int AL, int MG, uint32_t XR4>
static void launch_fc_rt_f32_t(const void *in, void *out, const FcRtArgs &a, const F32Edge &e, long long rows, hipStream_t s) {
    static LaunchState st[FC_RT_LDS_MAX / 1024 + 2];
    const int per_cu = prepared(st[(a.lds + 1023) / 1024], fc_rt_f32<AL, MG, XR4, EDGE>, 256, a.lds);
    FcRtArgs b = a; // (geometry as launch_fc_rt_t)
    b.R = (int)std::min<long long>(a.R, std::max<long long>(16, rows / 1024 / 16 * 16));
    const long long ntiles = (rows + b.R - 1) / b.R;
    long long walkers = std::max(1LL, 256LL * per_cu / a.NSL);
    walkers = std::min(walkers, ntiles);
    MF_LAUNCH((fc_rt_f32<AL, MG, XR4, EDGE>), dim3((unsigned)(walkers * a.NSL)), dim3(256), a.lds, s, (const int8_t *)in, (int8_t *)out, b, e, rows);
}
template <int EDGE> static void launch_fc_rt_f32_e(const void *in, void *out, const FcRtArgs &a, const F32Edge &e, long long rows, hipStream_t s) {
    if (a.K % 4 == 0) MF_DISPATCH4(a.magic, a.xr, launch_fc_rt_f32_t, (in, out, a, e, rows, s), EDGE, 4)
    else MF_DISPATCH4(a.magic, a.xr, launch_fc_rt_f32_t, (in, out, a, e, rows, s), EDGE, 1)
}
void launch_fc_rt_f32(const void *in, void *out, const FcRtArgs &a, const F32Edge &e, int edge, long long rows, hipStream_t s) {
    if (rows <= 0) return;
    if (edge == 3) launch_fc_rt_f32_e<3>(in, out, a, e, rows, s);
    else if (edge == EDGE_OUT) launch_fc_rt_f32_e<EDGE_OUT>(in, out, a, e, rows, s);
    else launch_fc_rt_f32_e<EDGE_IN>(in, out, a, e, rows, s);
}

template <int EDGE, int MG, uint32_t XR4>
static void launch_fc_chain_f32_t(const void *in, void *out, const FcChainArgs &a, const F32Edge &e, long long rows, hipStream_t s) {
    static LaunchState st[FC_RT_LDS_MAX / 1024 + 2];
    const int per_cu = prepared(st[(a.lds + 1023) / 1024], fc_chain_f32<MG, XR4, EDGE>, 256, a.lds);
    FcChainArgs b = a;
    b.R = (int)std::min<long long>(a.R, std::max<long long>(16, rows / 1024 / 16 * 16)); // (as launch_fc_rt_t)
    const long long ntiles = (rows + b.R - 1) / b.R;
    const long long grid = std::min(ntiles, 256LL * per_cu);
    MF_LAUNCH((fc_chain_f32<MG, XR4, EDGE>), dim3((unsigned)grid), dim3(256), a.lds, s, (const int8_t *)in, (int8_t *)out, b, e, rows);
}
void launch_fc_chain_f32(const void *in, void *out, const FcChainArgs &a, const F32Edge &e, int edge, long long rows, hipStream_t s) {
    if (rows <= 0) return;
    if (edge == 3) MF_DISPATCH4(a.magic, a.xr, launch_fc_chain_f32_t, (in, out, a, e, rows, s), 3)
    else if (edge == EDGE_OUT) MF_DISPATCH4(a.magic, a.xr, launch_fc_chain_f32_t, (in, out, a, e, rows, s), EDGE_OUT)
    else MF_DISPATCH4(a.magic, a.xr, launch_fc_chain_f32_t, (in, out, a, e, rows, s), EDGE_IN)
}

template <int MG, uint32_t XR4>
static void launch_pool_fc_f32_t(const int8_t *in, float *out, const PoolFcArgs &a, const F32Edge &e, long long rows, hipStream_t s) {
    static LaunchState st[FC_RT_LDS_MAX / 1024 + 2];
    const int per_cu = prepared(st[(a.c.lds + 1023) / 1024], pool_fc_chain_f32<MG, XR4>, 256, a.c.lds);
    PoolFcArgs b = a; // (geometry as launch_pool_fc_t)
    b.c.R = (int)std::min<long long>(a.c.R, std::max<long long>(16, rows / 1024 / 16 * 16));
    pool_fc_tb(b.c, b.c.R);
    const long long ntiles = (rows + b.c.R - 1) / b.c.R;
    const long long grid = std::min(ntiles, 256LL * per_cu);
    MF_LAUNCH((pool_fc_chain_f32<MG, XR4>), dim3((unsigned)grid), dim3(256), a.c.lds, s, in, (int8_t *)out, b, e, rows);
}
void launch_pool_fc_f32(const int8_t *in, float *out, const PoolFcArgs &a, const F32Edge &e, long long batch, hipStream_t s) {
    if (batch <= 0) return;
    if (a.c.xr) {
        if (a.c.magic == 2) launch_pool_fc_f32_t<2, 0x80808080u>(in, out, a, e, batch, s);
        else if (a.c.magic) launch_pool_fc_f32_t<1, 0x80808080u>(in, out, a, e, batch, s);
        else launch_pool_fc_f32_t<0, 0x80808080u>(in, out, a, e, batch, s);
    } else {
        if (a.c.magic == 2) launch_pool_fc_f32_t<2, 0u>(in, out, a, e, batch, s);
        else if (a.c.magic) launch_pool_fc_f32_t<1, 0u>(in, out, a, e, batch, s);
        else launch_pool_fc_f32_t<0, 0u>(in, out, a, e, batch, s);
    }
}

} // namespace k
} // namespace mf
