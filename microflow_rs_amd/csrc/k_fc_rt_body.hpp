// k_fc_rt_body.hpp -- the device code of fc_rt and fc_chain (k_fc_rt.hip describes both): one body each, instantiated as the int8
// kernels there and as the instances that hold a model's f32 boundary in k_fc_f32.hip.  Device code only.
#pragma once
#include "k_common.hpp"
#include "k_fc_layer.hpp"

namespace mf {
namespace k {

// EDGE (kernels.hpp: EDGE_IN | EDGE_OUT) != 0: the instances that hold a model's f32 boundary (fc_rt_f32 below).  Entry: the rows
// are staged by 16-byte loads of the floats [r0 K, r1 K), quantised and written to the row buffer from its first byte on; exit: the
// step's patch leaves as floats.  Everything between the staging and the patch is the int8 instance's.
template <int AL, int MG, uint32_t XR4, int EDGE>
__device__ __forceinline__ void fc_rt_body(const int8_t *__restrict__ in, int8_t *__restrict__ out, const FcRtArgs &p, long long rows, const F32Edge &eg) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K = p.K, N = p.N, KS = p.KS, R = p.R, TB = p.TB;
    const int slice = blockIdx.x % p.NSL, walker = blockIdx.x / p.NSL, nwalk = gridDim.x / p.NSL;
    const int nt0 = slice * p.NTS, nts = min(p.NTS, p.NT - nt0);
    const int n0 = nt0 * 16, ns = min(nts * 16, N - n0); // this slice's output columns
    uint8_t *W = lds, *PT = lds + p.poff;
    const int col = lane & 15, g = lane >> 4;

    // resident weights: the slice's tiles are one contiguous run of the image (whole 1 KiB pieces)
    const int8_t *wsrc = (const int8_t *)p.wimg + (size_t)nt0 * KS * 1024;
    for (int b = wave * 64; b < nts * KS * 64; b += 256) dma16(wsrc + (size_t)(b + lane) * 16, W + b * 16);

    // the row tile t: bytes [a0, r1 K) of the batch, a0 = r0 K rounded down to 16
    auto stage = [&](long long t, uint8_t *buf) {
        const long long r0 = t * R, r1 = min(r0 + R, rows);
        if constexpr (EDGE & EDGE_IN) { // (r0 is a multiple of 16: the step's first float is 16-byte aligned where `in` is)
            edge_stage_f32((const float *)in + r0 * K, buf, (int)((r1 - r0) * K), eg, tid);
            return;
        }
        const long long a0 = (r0 * K) & ~15ll;
        const int P = (int)((r1 * K - a0 + 15) >> 4);
        for (int b = wave * 64; b < P; b += 256)
            if (b + lane < P) dma16(in + a0 + (long long)(b + lane) * 16, buf + b * 16);
    };
    // operand bytes past K: masks of the last k step (lane group g holds k = 64 ks + 16 g .. + 15)
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
    const long long ntiles = (rows + R - 1) / R;
    const int CH = R / 16, ngr = (nts + TB - 1) / TB, units = CH * ngr;
    int cur = 0;
    if (walker < ntiles) stage(walker, lds + p.xoff);
    for (long long t = walker; t < ntiles; t += nwalk) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's DMAs of the tile (and of the weights) have landed ...
        wg_sync();                                       // ... and every other wave's
        const uint8_t *xb = lds + p.xoff + cur * p.xbytes;
        if (p.NBUF == 2 && t + nwalk < ntiles) stage(t + nwalk, lds + p.xoff + (cur ^ 1) * p.xbytes);
        const long long r0 = t * R, r1 = min(r0 + R, rows);
        const int tsh = (EDGE & EDGE_IN) ? 0 : (int)((r0 * K) & 15); // row r0's offset in the buffer
        const int osh = (EDGE & EDGE_OUT) ? 0 : (int)(((uintptr_t)out + r0 * N) & 15); // the patch sits at the output's alignment (single slice)
        for (int u = wave; u < units; u += 4) {
            const int c = u % CH, grp = u / CH;
            const int lt0 = grp * TB, tb = min(TB, nts - lt0);
            const int rr = c * 16 + col;                 // this lane's row in the tile (operand B column)
            const int base = tsh + rr * K + g * 16;
            v4i acc[4], rsa = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i < tb) {
                    const int4 kc = magic4<MG>(*(const int4 *)(p.Kc + n0 + (lt0 + i) * 16 + g * 4));
                    acc[i] = v4i{kc.x, kc.y, kc.z, kc.w};
                }
            }
            for (int ks = 0; ks < KS; ++ks) {
                const int off = base + ks * 64;
                v4i b;
                if constexpr (AL == 4) {
                    const uint32_t *q = (const uint32_t *)(xb + off);
                    b = v4i{(int)q[0], (int)q[1], (int)q[2], (int)q[3]};
                } else {
                    const uint32_t *q = (const uint32_t *)(xb + (off & ~3));
                    const uint32_t sh = off & 3, d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], d4 = q[4];
                    b = v4i{(int)__builtin_amdgcn_alignbyte(d1, d0, sh), (int)__builtin_amdgcn_alignbyte(d2, d1, sh),
                            (int)__builtin_amdgcn_alignbyte(d3, d2, sh), (int)__builtin_amdgcn_alignbyte(d4, d3, sh)};
                }
                if (ks == KS - 1) b &= v4i{(int)km[0], (int)km[1], (int)km[2], (int)km[3]};
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < tb) acc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(*(const v4i *)(W + (((lt0 + i) * KS + ks) * 64 + lane) * 16), b, acc[i], 0, 0, 0);
                if (p.wzp) rsa = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, b, rsa, 0, 0, 0); // every row: sum_k x[row][k]
            }
            const int wr = p.wzp * rsa[0];
            const float4 S4 = {p.S, p.S, p.S, p.S};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i < tb) {
                    const int lc = (lt0 + i) * 16 + g * 4, ch = n0 + lc; // slice-local / global column of the lane's 4 results
                    v4i a = acc[i];
                    a[0] -= wr, a[1] -= wr, a[2] -= wr, a[3] -= wr;
                    const float4 A4 = *(const float4 *)(p.A + ch);
                    const uint32_t d = requant_pack4<MG, XR4>(a[0], a[1], a[2], a[3], A4, S4, p.lo_f, p.hi_f);
                    if (p.NSL == 1) {
                        uint8_t *dst = PT + osh + rr * N + ch;
                        if ((N & 3) == 0) {
                            if (ch < N) *(uint32_t *)dst = d;
                        } else {
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (ch + j < N) dst[j] = (uint8_t)(d >> (8 * j));
                        }
                    } else {
                        *(uint32_t *)(PT + rr * (p.NTS * 16) + lc) = d;
                    }
                }
            }
        }
        wg_sync();                                       // the patch is complete; the row buffer is free
        if (p.NBUF == 1 && t + nwalk < ntiles) stage(t + nwalk, lds + p.xoff);
        const int nr = (int)(r1 - r0);
        if constexpr (EDGE & EDGE_OUT) {
            float *fo = (float *)out;
            if (p.NSL == 1) {
                edge_store_f32(fo + r0 * N, PT, nr * N, eg, tid);
            } else { // one slice: ns floats of each row at column n0
                const int pitch = p.NTS * 16;
                for (int e = tid; e < nr * ns; e += 256) {
                    const int r = e / ns, q = e - r * ns;
                    fo[(r0 + r) * N + n0 + q] = __fmul_rn(eg.out_scale, __fsub_rn((float)(int)(int8_t)PT[r * pitch + q], eg.out_zp_f));
                }
            }
        } else if (p.NSL == 1) {
            // R x N contiguous output bytes [gs, ge): bytes up to the first 16-byte boundary, 16-byte stores, bytes after the last
            int8_t *gs = out + r0 * N, *ge = gs + (long long)nr * N;
            const uintptr_t ugs = (uintptr_t)gs, uge = (uintptr_t)ge;
            const uintptr_t up = (ugs + 15) & ~(uintptr_t)15, dn = uge & ~(uintptr_t)15;
            const uintptr_t hb = up < uge ? up : uge, te = dn > hb ? dn : hb;
            const int nhead = (int)(hb - ugs), nbody = (int)((te - hb) >> 4), ntail = (int)(uge - te);
            const uint8_t *src = PT + osh;               // src[i] is output byte gs + i
            for (int i = tid; i < nbody; i += 256)
                *(v4i *)(gs + nhead + i * 16) = *(const v4i *)(src + nhead + i * 16);
            if (tid < nhead) gs[tid] = (int8_t)src[tid];
            else if (tid >= 64 && tid < 64 + ntail) gs[nhead + nbody * 16 + (tid - 64)] = (int8_t)src[nhead + nbody * 16 + (tid - 64)];
        } else {
            // one slice: ns bytes of each row at column n0
            const int pitch = p.NTS * 16;
            if ((N & 3) == 0) {
                const int n4 = ns >> 2;
                for (int e = tid; e < nr * n4; e += 256) {
                    const int r = e / n4, q = e - r * n4;
                    *(uint32_t *)(out + (r0 + r) * N + n0 + q * 4) = *(const uint32_t *)(PT + r * pitch + q * 4);
                }
            } else {
                for (int e = tid; e < nr * ns; e += 256) {
                    const int r = e / ns, q = e - r * ns;
                    out[(r0 + r) * N + n0 + q] = (int8_t)PT[r * pitch + q];
                }
            }
        }
        cur ^= p.NBUF - 1;
    }
}
// EDGE != 0: the f32 boundary as in fc_rt_body (fc_chain_f32 below)
template <int MG, uint32_t XR4, int EDGE>
__device__ __forceinline__ void fc_chain_body(const int8_t *__restrict__ in, int8_t *__restrict__ out, const FcChainArgs &p, long long rows, const F32Edge &eg) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int R = p.R, L = p.L, K0 = p.l[0].K, NL = p.l[L - 1].N;
    uint8_t *PT = lds + p.poff;
    for (int l = 0; l < L; ++l) {
        const int8_t *wsrc = (const int8_t *)p.l[l].wimg;
        for (int b = wave * 64; b < p.l[l].NT * p.l[l].KS * 64; b += 256) dma16(wsrc + (size_t)(b + lane) * 16, lds + p.l[l].woff + b * 16);
    }
    const uintptr_t uin = (uintptr_t)in;
    auto stage = [&](long long t, uint8_t *buf) {
        const long long r0 = t * R, r1 = min(r0 + R, rows);
        if constexpr (EDGE & EDGE_IN) {
            edge_stage_f32((const float *)in + r0 * K0, buf, (int)((r1 - r0) * K0), eg, tid);
            return;
        }
        const uintptr_t a0 = (uin + r0 * K0) & ~(uintptr_t)15, e = uin + r1 * K0;
        const int P = (int)((e - a0 + 15) >> 4);
        for (int b = wave * 64; b < P; b += 256)
            if (b + lane < P) dma16((const int8_t *)(a0 + (uintptr_t)(b + lane) * 16), buf + b * 16);
    };
    const long long ntiles = (rows + R - 1) / R;
    int cur = 0;
    if ((long long)blockIdx.x < ntiles) stage(blockIdx.x, lds + p.xoff);
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        wg_sync();
        const uint8_t *xb = lds + p.xoff + cur * p.xbytes;
        if (p.NBUF == 2 && t + gridDim.x < ntiles) stage(t + gridDim.x, lds + p.xoff + (cur ^ 1) * p.xbytes);
        const long long r0 = t * R, r1 = min(r0 + R, rows);
        const int nr = (int)(r1 - r0);
        const int tsh = (EDGE & EDGE_IN) ? 0 : (int)((uin + r0 * K0) & 15);
        const int osh = (EDGE & EDGE_OUT) ? 0 : (int)(((uintptr_t)out + r0 * NL) & 15);
        const uint8_t *src = xb + tsh;
        for (int l = 0; l < L; ++l) {
            const bool last = l == L - 1;
            uint8_t *dst = (last && !p.softmax) ? PT + osh : lds + p.aoff + (l & 1) * p.abytes;
            fc_chain_layer<MG, XR4>(p.l[l], src, dst, lds + p.l[l].woff, R, wave, lane);
            wg_sync();                                   // the layer's tile is complete: the next layer's operand
            src = dst;
        }
        if (p.softmax) {
            fc_chain_softmax(p.sm, src, PT + osh, nr, NL, tid);
            wg_sync();
        }
        if (p.NBUF == 1 && t + gridDim.x < ntiles) stage(t + gridDim.x, lds + p.xoff);
        if constexpr (EDGE & EDGE_OUT) edge_store_f32((float *)out + r0 * NL, PT, nr * NL, eg, tid);
        else fc_chain_store_patch(out + r0 * NL, PT + osh, (long long)nr * NL, tid);
        cur ^= p.NBUF - 1;
    }
}
} // namespace k
} // namespace mf
