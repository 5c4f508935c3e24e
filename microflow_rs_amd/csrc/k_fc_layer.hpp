// k_fc_layer.hpp -- the steps that the launches with FullyConnected layers resident in LDS share (k_fc_rt.hip: fc_chain;
// k_pool_fc.hip: pool_fc_chain): one layer over the step's R rows, the Softmax over one row, and the step's output patch.
// Device code only; every function is inlined into its kernel.
#pragma once
#include "k_common.hpp"

namespace mf {
namespace k {

// One FullyConnected layer of a step: products of the R source rows in LDS (`src`, row pitch K, readable for 20 bytes past the
// last row) with the layer's resident image `W`, the weight-zero-point row sums, the layer's own epilogue (requant_pack4: the
// bytes of its layer-wise launch), and its int8 [R][N] tile at `dst` (row pitch N).  The four waves share the (16-row chunk,
// group of TB tiles) units.
template <int MG, uint32_t XR4>
__device__ __forceinline__ void fc_chain_layer(const FcChainLayer &L, const uint8_t *src, uint8_t *dst, const uint8_t *W, int R, int wave,
                                               int lane) {
    const int K = L.K, N = L.N, KS = L.KS, TB = L.TB, nts = L.NT;
    const int col = lane & 15, g = lane >> 4;
    uint32_t km[4];
    {
        const int rem = K - (KS - 1) * 64 - g * 16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int nb = min(max(rem - 4 * i, 0), 4);
            km[i] = nb >= 4 ? 0xffffffffu : (1u << (8 * nb)) - 1u;
        }
    }
    const v4i ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    const int CH = R / 16, ngr = (nts + TB - 1) / TB, units = CH * ngr;
    for (int u = wave; u < units; u += 4) {
        const int c = u % CH, grp = u / CH;
        const int lt0 = grp * TB, tb = min(TB, nts - lt0);
        const int rr = c * 16 + col;
        const int base = rr * K + g * 16;
        v4i acc[4], rsa = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < tb) {
                const int4 kc = magic4<MG>(*(const int4 *)(L.Kc + (lt0 + i) * 16 + g * 4));
                acc[i] = v4i{kc.x, kc.y, kc.z, kc.w};
            }
        }
        for (int ks = 0; ks < KS; ++ks) {
            const int off = base + ks * 64;
            const uint32_t *q = (const uint32_t *)(src + (off & ~3));
            const uint32_t sh = off & 3, d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], d4 = q[4];
            v4i b = v4i{(int)__builtin_amdgcn_alignbyte(d1, d0, sh), (int)__builtin_amdgcn_alignbyte(d2, d1, sh),
                        (int)__builtin_amdgcn_alignbyte(d3, d2, sh), (int)__builtin_amdgcn_alignbyte(d4, d3, sh)};
            if (ks == KS - 1) b &= v4i{(int)km[0], (int)km[1], (int)km[2], (int)km[3]};
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < tb) acc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(*(const v4i *)(W + (((lt0 + i) * KS + ks) * 64 + lane) * 16), b, acc[i], 0, 0, 0);
            if (L.wzp) rsa = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, b, rsa, 0, 0, 0);
        }
        const int wr = L.wzp * rsa[0];
        const float4 S4 = {L.S, L.S, L.S, L.S};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < tb) {
                const int ch = (lt0 + i) * 16 + g * 4;
                v4i a = acc[i];
                a[0] -= wr, a[1] -= wr, a[2] -= wr, a[3] -= wr;
                const float4 A4 = *(const float4 *)(L.A + ch);
                const uint32_t d = requant_pack4<MG, XR4>(a[0], a[1], a[2], a[3], A4, S4, L.lo_f, L.hi_f);
                uint8_t *dp = dst + rr * N + ch;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (ch + j < N) dp[j] = (uint8_t)(d >> (8 * j));
            }
        }
    }
}

// microflow::ops::softmax over the N outputs of each of the step's nr rows (softmax_table's arithmetic, k_generic.hip): `x` is the
// last layer's [nr][N] tile, `y` the [nr][N] patch; one thread per row
__device__ __forceinline__ void fc_chain_softmax(const SoftmaxArgs &sm, const uint8_t *x_tile, uint8_t *y_tile, int nr, int N, int tid) {
    for (int r = tid; r < nr; r += 256) {
        const int8_t *x = (const int8_t *)x_tile + r * N;
        uint8_t *y = y_tile + r * N;
        float sum = 0.0f;
        for (int j = 0; j < N; ++j) sum = __fadd_rn(sum, sm.exp_table[(int)x[j] + 128]);
        for (int j = 0; j < N; ++j) {
            const float ev = sm.exp_table[(int)x[j] + 128];
            const float prob = __fdiv_rn(ev, sum);
            const float q = __fadd_rn(__fdiv_rn(prob, sm.oscale), sm.ozp_f);
            const float rq = __fadd_rn(q, __builtin_copysignf(0x1.fffffep-2f, q));
            const int qi = (rq != rq) ? 0 : (int)__builtin_amdgcn_fmed3f(rq, sm.sat_lo, sm.sat_hi);
            y[j] = (uint8_t)(qi ^ sm.xr);
        }
    }
}

// The step's output: `nbytes` contiguous bytes at `gs`, taken from the LDS patch `po` (po[i] is byte gs + i; the patch sits at the
// output's alignment): bytes up to the first 16-byte boundary, 16-byte stores, bytes after the last boundary.  Nothing else is written.
__device__ __forceinline__ void fc_chain_store_patch(int8_t *gs, const uint8_t *po, long long nbytes, int tid) {
    int8_t *ge = gs + nbytes;
    const uintptr_t ugs = (uintptr_t)gs, uge = (uintptr_t)ge;
    const uintptr_t up = (ugs + 15) & ~(uintptr_t)15, dn = uge & ~(uintptr_t)15;
    const uintptr_t hb = up < uge ? up : uge, te = dn > hb ? dn : hb;
    const int nhead = (int)(hb - ugs), nbody = (int)((te - hb) >> 4), ntail = (int)(uge - te);
    for (int i = tid; i < nbody; i += 256)
        *(v4i *)(gs + nhead + i * 16) = *(const v4i *)(po + nhead + i * 16);
    if (tid < nhead) gs[tid] = (int8_t)po[tid];
    else if (tid >= 64 && tid < 64 + ntail) gs[nhead + nbody * 16 + (tid - 64)] = (int8_t)po[nhead + nbody * 16 + (tid - 64)];
}

// ---- the model boundary inside these launches (kernels.hpp: F32Edge) ----
// quantize_f32's value-by-value arithmetic (k_generic.hip), the division in the form the host verified for the model's parameters
__device__ __forceinline__ int edge_quant(float x, const F32Edge &e) {
    const float t = __fadd_rn(quant_div(x, e.in_scale, e.in_rcp, e.in_fast != 0), e.in_zp_f);
    const float r = __fadd_rn(t, __builtin_copysignf(0x1.fffffep-2f, t));
    return (r != r) ? 0 : (int)__builtin_amdgcn_fmed3f(r, e.in_sat_lo, e.in_sat_hi);
}
// f32 entry: the step's `n` floats at `src` (16-byte aligned) become the int8 bytes buf[0 .. n) of the row buffer in LDS: 16-byte
// loads of whole quads, the last n % 4 floats one by one.  Only those n floats are read.
__device__ __forceinline__ void edge_stage_f32(const float *src, uint8_t *buf, int n, const F32Edge &e, int tid) {
    const int n4 = n >> 2;
    for (int i = tid; i < n4; i += 256) {
        const float4 v = ((const float4 *)src)[i];
        *(uint32_t *)(buf + 4 * i) = pack4(edge_quant(v.x, e), edge_quant(v.y, e), edge_quant(v.z, e), edge_quant(v.w, e)) ^ e.in_xr4;
    }
    for (int i = (n4 << 2) + tid; i < n; i += 256) buf[i] = (uint8_t)(edge_quant(src[i], e) ^ (int)(e.in_xr4 & 0xffu));
}
// f32 exit: the `n` bytes of the LDS patch `po` (internal domain) leave as the floats dst[0 .. n), dequantize_i8's expression.  Nothing
// else is written.
__device__ __forceinline__ void edge_store_f32(float *dst, const uint8_t *po, int n, const F32Edge &e, int tid) {
    for (int i = tid; i < n; i += 256) dst[i] = __fmul_rn(e.out_scale, __fsub_rn((float)(int)(int8_t)po[i], e.out_zp_f));
}

} // namespace k
} // namespace mf
