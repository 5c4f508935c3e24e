// k_pool_fc_body.hpp -- the device code of pool_fc_chain (k_pool_fc.hip describes it), instantiated as the int8 kernels there and as
// the instances that hold a model's f32 exit in k_fc_f32.hip; and the one host helper both launchers share.
#pragma once
#include <algorithm>

#include "k_common.hpp"
#include "k_fc_layer.hpp"

namespace mf {
namespace k {

// F32OUT: the instance that holds a model's f32 exit (pool_fc_chain_f32 below): the step's patch leaves as floats
template <int MG, uint32_t XR4, bool F32OUT>
__device__ __forceinline__ void pool_fc_body(const int8_t *__restrict__ in, int8_t *__restrict__ out, const PoolFcArgs &p, long long rows, const F32Edge &eg) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FcChainArgs &c = p.c;
    const int R = c.R, L = c.L, NL = c.l[L - 1].N;
    const int P = p.P, C = p.C, CGW = p.CGW, NS = p.NS, NPASS = p.NPASS, NIT = p.NIT;
    uint8_t *PT = lds + c.poff, *TILE = lds + c.xoff;
    for (int l = 0; l < L; ++l) {
        const int8_t *wsrc = (const int8_t *)c.l[l].wimg;
        for (int b = wave * 64; b < c.l[l].NT * c.l[l].KS * 64; b += 256) dma16(wsrc + (size_t)(b + lane) * 16, lds + c.l[l].woff + b * 16);
    }
    // this lane in the pool product: column j = (channel group cgl of the pass, pixel subset sub), lane group g = one of 4 pixels
    const int j = lane & 15, g = lane >> 4;
    const int cgl = j % CGW, sub = j / CGW;
    const bool colok = sub < NS;
    const int lane_p0 = sub * 4 + g;                     // the lane's pixel in a load's 4 NS pixels
    const int lane_off = lane_p0 * C + cgl * 16;
    const int step_pix = 4 * NS;
    const int one = 1 << (8 * (j & 3));                  // operand A: row i = lane & 15 has its 1 at k = 16 g + i
    const v4i A1 = {(j >> 2) == 0 ? one : 0, (j >> 2) == 1 ? one : 0, (j >> 2) == 2 ? one : 0, (j >> 2) == 3 ? one : 0};
    const long long PC = (long long)P * C;
    const int bias_len = p.bias * P;
    const uint32_t xr4 = 0x01010101u * (uint32_t)c.xr;

    struct It { int img, pass, t; };
    auto adv = [&](It &i) {
        if (++i.t == NIT) {
            i.t = 0;
            if (++i.pass == NPASS) i.pass = 0, i.img += 4;
        }
    };
    const long long ntiles = (rows + R - 1) / R;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long long r0 = t * R, r1 = min(r0 + R, rows);
        const int nr = (int)(r1 - r0);
        const int8_t *img0 = in + r0 * PC;
        // Every load is issued, none sits behind a branch (the wait counters then know how many are in flight: a wait for the older set
        // leaves the younger one flying).  A lane with nothing to load -- an idle column, a pixel past the image, a slot past the step's
        // images -- reads the batch's first 16 bytes instead, and sum4 zeroes what it contributes.
        auto wanted = [&](const It &i) { return colok && (i.pass * 16 + cgl) * 16 < C && i.t * step_pix + lane_p0 < P; };
        auto load = [&](const It &i) {
            const int8_t *a = img0 + (long long)i.img * PC + (long long)i.t * step_pix * C + i.pass * 256 + lane_off;
            return *(const v4i *)((i.img < nr && wanted(i)) ? a : in);
        };
        // the sums of (image, pass) are complete: add the NS columns of each channel group, requantise, one dword into the tile
        auto finish = [&](const It &i, const v4i &acc) {
            int v[4] = {acc[0], acc[1], acc[2], acc[3]};
            if (NS > 1) {
                if (CGW * NS == 16) {                    // the subsets are the high bits of j: a butterfly
                    for (int m = CGW; m < 16; m <<= 1)
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] += __builtin_amdgcn_ds_bpermute((lane ^ m) << 2, v[e]);
                } else {                                 // (C / 16 = 3, 5, 6, 7: 5, 3, 2, 2 subsets) the lanes of subset 0 collect
                    int w[4] = {v[0], v[1], v[2], v[3]};
                    for (int s2 = 1; s2 < NS; ++s2)
#pragma unroll
                        for (int e = 0; e < 4; ++e) w[e] += __builtin_amdgcn_ds_bpermute(((lane + s2 * CGW) & 63) << 2, v[e]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = w[e];
                }
            }
            const int cg = i.pass * 16 + cgl;
            if (sub == 0 && cg * 16 < C) {
                int q[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float x = __fmul_rn(p.inv, (float)(v[e] + bias_len));
                    const float y = __fadd_rn(__fmul_rn(p.c0, x), p.c1);
                    const float r = __fadd_rn(y, __builtin_copysignf(0x1.fffffep-2f, y));
                    int z = (r != r) ? 0 : (int)__builtin_amdgcn_fmed3f(r, p.sat_lo, p.sat_hi);
                    z = max(z, p.lo);
                    q[e] = min(z, p.hi);
                }
                *(uint32_t *)(TILE + i.img * C + cg * 16 + 4 * g) = pack4(q[0], q[1], q[2], q[3]) ^ xr4;
            }
        };
        It li = {wave, 0, 0}, pi = li;
        v4i acc = {0, 0, 0, 0};
        auto load4 = [&](v4i (&b)[4]) {
#pragma unroll
            for (int k = 0; k < 4; ++k) b[k] = load(li), adv(li);
        };
        auto sum4 = [&](const v4i (&b)[4]) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (pi.img < nr) {
                    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A1, wanted(pi) ? b[k] : v4i{0, 0, 0, 0}, acc, 0, 0, 0);
                    if (pi.t == NIT - 1) {
                        finish(pi, acc);
                        acc = v4i{0, 0, 0, 0};
                    }
                    adv(pi);
                }
            }
        };
        // two register sets of four loads: one is being filled while the other is summed (no copies: a copy would wait for the load)
        v4i ba[4], bb[4];
        load4(ba);
        while (pi.img < nr) {
            load4(bb);
            sum4(ba);
            if (pi.img >= nr) break;
            load4(ba);
            sum4(bb);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // (first step: this wave's DMAs of the weights have landed ...)
        wg_sync();                                       // ... and every other wave's; the pooled tile is complete
        const int osh = F32OUT ? 0 : (int)(((uintptr_t)out + r0 * NL) & 15);
        const uint8_t *src = TILE;
        for (int l = 0; l < L; ++l) {
            const bool last = l == L - 1;
            uint8_t *dst = (last && !c.softmax) ? PT + osh : lds + c.aoff + (l & 1) * c.abytes;
            fc_chain_layer<MG, XR4>(c.l[l], src, dst, lds + c.l[l].woff, R, wave, lane);
            wg_sync();                                   // the layer's tile is complete: the next layer's operand
            src = dst;
        }
        if (c.softmax) {
            fc_chain_softmax(c.sm, src, PT + osh, nr, NL, tid);
            wg_sync();
        }
        if constexpr (F32OUT) edge_store_f32((float *)out + r0 * NL, PT, nr * NL, eg, tid);
        else fc_chain_store_patch(out + r0 * NL, PT + osh, (long long)nr * NL, tid);
    }
}
static inline void pool_fc_tb(FcChainArgs &c, int R) { // tiles per unit: every wave gets a (16-row chunk, tile group) unit where there are four
    for (int l = 0; l < c.L; ++l) {
        FcChainLayer &y = c.l[l];
        y.TB = std::min(4, y.NT);
        while (y.TB > 1 && (R / 16) * ((y.NT + y.TB - 1) / y.TB) < 4) y.TB /= 2;
    }
}

} // namespace k
} // namespace mf
