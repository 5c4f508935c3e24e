// k_dw_gemm.hip -- DepthwiseConv2D of ANY channel count C >= 2 (one output per channel), filters up to 7 x 7, any strides, SAME or
// VALID, with or without per-channel filter zero points, on the int8 matrix pipe (microflow::ops::depthwise_conv_2d,
// src/ops/depthwise_conv_2d.rs:28-105).
//
// The shape-specialised depthwise kernels take corners of that space (the 3x3 SAME stride-1 / 2 tables and dw3x3_rt; dw_mm_rt: C % 16
// == 0 and zero filter zero points); every other such layer with finite constants and whole-dword image rows ((W C) % 4 == 0) runs
// here instead of on the byte-wise dwconv_generic.  The contraction is dw_mm_rt's (k_rt.hip): for a 16-channel group the taps are a
// block-diagonal K = 16 KH KW product -- lane group g of k step ks supplies the group's 16 bytes of tap 4 ks + g, operand A holds the
// tap's weight of channel r in byte r of row r (wimage.cpp build_dw_mm_rt_weights) -- and a wave works through a contiguous range of
// (group, 16-pixel chunk) items with the group's operand A and constants in registers.  What differs:
//
//   operand B : a group starts at (pixel) C + 16 (group), 16-byte aligned only when C % 16 == 0; it is read at its natural alignment:
//               AL = 16 one ds_read_b128, AL = 8 two ds_read_b64, AL = 4 four aligned dwords, AL = 1 five aligned dwords and
//               v_alignbyte.  The last group's bytes >= C belong to the next pixel (or the halo) and meet zero weights; the tile
//               rows have room for that over-read.
//   staging   : conv_gemm_rt's: G whole images or one band of output rows per step inside an input-zero-point halo, rows by LDS-DMA
//               when W C % 16 == 0, else by dword loads.
//   WZ        : filter zero points: the window sum of every channel is one more MFMA per k step, on the operand B already in
//               registers, against a block-diagonal tile of ones built in registers (the padded taps of the last step masked to
//               zero); the epilogue subtracts wzp[c] x sum.  (A -wzp diagonal folded into the same accumulator would save the second
//               accumulator but cannot hold wzp = -128, the i8-domain zero point of a u8 model whose zero point is 0.)
//   output    : each lane's 4 channels of its pixel: a dword store where C % 4 == 0, else one byte per real channel.
//
// Epilogue: requant_pack4<MG, XR4> (k_common.hpp), modes 0 .. 2 as the host proved them for the operator's constants.
#include "k_common.hpp"

#include <algorithm>
#include <map>
#include <mutex>

namespace mf {
namespace k {

// KSMAX >= p.KS: the k steps (4 taps each) the instance holds in registers -- 4, 7 or 13 (filters of up to 16, 28, 52 taps); the steps
// past p.KS are skipped by a wave-uniform test
template <int AL, bool WZ, int KSMAX, int MG, uint32_t XR4>
__global__ __launch_bounds__(256) void dw_gemm_rt(const int8_t *__restrict__ in, int8_t *__restrict__ out, DwGemmArgs p, int batch) {
    constexpr int NWAVE = 4;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = p.C, KS = p.KS, NBLK = p.NBLK, ROW = p.ROW, TILE = p.TILE, G = p.G, RB = p.RB;
    const int H = p.H, OH = p.OH, OW = p.OW, ROWB = p.W * C, BH = p.BH, NBANDS = p.NBANDS, T = p.KH * p.KW;
    const uint32_t izp4 = p.izp4;
    for (int i = tid; i < (G * TILE + 256) / 16; i += 256) ((uint4 *)lds)[i] = make_uint4(izp4, izp4, izp4, izp4);
    const int col = lane & 15, g = lane >> 4;
    int toff[KSMAX]; // this lane group's tap offset from the window start in every k step (0 past the filter: zero weights)
#pragma unroll
    for (int ks = 0; ks < KSMAX; ++ks) {
        const int t = 4 * ks + g;
        toff[ks] = t < T ? (t / p.KW) * ROW + (t % p.KW) * C : 0;
    }
    // the ones tile: row r of every real tap has its 1 in byte r (the tap's channel r)
    const int one1 = 1 << (8 * (col & 3));
    const v4i ones = {(col >> 2) == 0 ? one1 : 0, (col >> 2) == 1 ? one1 : 0, (col >> 2) == 2 ? one1 : 0, (col >> 2) == 3 ? one1 : 0};
    const v4i zero4 = {0, 0, 0, 0};
    const int P = p.P, OWS = (OW + P - 1) / P, PC = P == 1 ? C : P * C; // columns per output row; real rows of a 16-row group
    const float inv_ow = 1.0f / (float)OWS, inv_bp = 1.0f / (float)(BH * OWS);
    const int nsteps = ((batch + G - 1) / G) * NBANDS;
    for (int step = blockIdx.x; step < nsteps; step += gridDim.x) {
        const int band = step % NBANDS, ist = step / NBANDS;
        const int yfirst = band * BH * p.sh - p.padt;   // input row held by tile row 0
        wg_sync();                                       // the previous step's reads of the tile are done (the first time: the fill)
        for (int gi = 0; gi < G; ++gi) {
            const long img = (long)ist * G + gi;
            if (img >= batch) break;
            for (int r = wave; r < RB; r += NWAVE) {
                const int y = yfirst + r;
                uint8_t *dst = lds + gi * TILE + r * ROW + p.LP;
                if (y >= 0 && y < H) {
                    const int8_t *src = in + (img * H + y) * (long)ROWB;
                    if ((ROWB & 15) == 0) {
                        for (int o = 0; o < ROWB; o += 1024)
                            if (o + lane * 16 < ROWB) dma16(src + o + lane * 16, dst + o);
                    } else {
                        for (int o = lane * 4; o < ROWB; o += 256) *(uint32_t *)(dst + o) = *(const uint32_t *)(src + o);
                    }
                } else if (NBANDS > 1) {                 // band mode: this tile row is padding in this step only
                    for (int o = lane * 4; o < ROWB; o += 256) *(uint32_t *)(dst + o) = izp4;
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's DMAs have landed ...
        wg_sync();                                       // ... and every other wave's
        const int gvalid = min(G, batch - ist * G);
        const int rows_here = min(BH, OH - band * BH);
        const int bp = BH * OWS, npix = gvalid * bp;      // (band mode: the rows past the image are masked below)
        // items = (16-channel group, chunk of 16 pixels), group-major; every wave takes one contiguous quarter of them, so that a group's
        // operand A and constants stay in registers across the wave's chunks of that group
        const int nchunks = (npix + 15) >> 4, nitems = NBLK * nchunks;
        const int i0 = (int)(((long)nitems * wave) / NWAVE), i1 = (int)(((long)nitems * (wave + 1)) / NWAVE);
        int blk_have = -1;
        v4i wA[KSMAX];
        int4 kc = make_int4(0, 0, 0, 0), wz = kc;
        float4 cA = make_float4(0.f, 0.f, 0.f, 0.f), cS = cA;
        for (int it = i0; it < i1; ++it) {
            const int blk = it / nchunks, chunk = it - blk * nchunks;
            const int ch = 16 * blk + 4 * g;             // the lane's 4 channels
            if (blk != blk_have) { // (wave-uniform; at most NBLK / NWAVE + 1 times per step)
                blk_have = blk;
#pragma unroll
                for (int ks = 0; ks < KSMAX; ++ks)
                    wA[ks] = ks < KS ? ((const v4i *)p.wprep)[((size_t)blk * KS + ks) * 64 + lane] : zero4;
                kc = magic4<MG>(*(const int4 *)(p.Kc + ch));
                cA = *(const float4 *)(p.A + ch), cS = *(const float4 *)(p.S + ch);
                if constexpr (WZ) wz = *(const int4 *)(p.wzp + ch);
            }
            const int pp = chunk * 16 + col;             // the lane's column: a pixel, or with P > 1 a run of P pixels of one row
            const int pc = pp < npix ? pp : npix - 1;
            const int gi = (int)(((float)pc + 0.5f) * inv_bp);
            const int rr = pc - gi * bp;
            const int oyl = (int)(((float)rr + 0.5f) * inv_ow), ox = (rr - oyl * OWS) * P;
            const bool live = pp < npix && oyl < rows_here;
            const int wbase = gi * TILE + (oyl * p.sh) * ROW + p.LP + (ox * p.sw - p.padl) * C + 16 * blk; // the group's window start
            // operand B of k step ks: the group's 16 bytes of tap 4 ks + g, from reads at their natural alignment
            auto operand = [&](int ks) -> v4i {
                const int off = wbase + toff[ks];
                if constexpr (AL == 16) {
                    return *(const v4i *)(lds + off);
                } else if constexpr (AL == 8) {
                    // (left to itself hipcc fuses the pair into ONE ds_read_b128, 8 bytes off its natural alignment: replayed at ~64
                    // cycles, 48x48x8 5x5 ran 4x slower than with two ds_read_b64; the opaque second address keeps them apart)
                    int off8 = off + 8;
                    asm("" : "+v"(off8));
                    const uint2 lo = *(const uint2 *)(lds + off), hi = *(const uint2 *)(lds + off8);
                    return v4i{(int)lo.x, (int)lo.y, (int)hi.x, (int)hi.y};
                } else if constexpr (AL == 4) {
                    const uint32_t *q = (const uint32_t *)(lds + off);
                    return v4i{(int)q[0], (int)q[1], (int)q[2], (int)q[3]};
                } else {
                    const uint32_t *q = (const uint32_t *)(lds + (off & ~3));
                    const uint32_t sh = off & 3, d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], d4 = q[4];
                    return v4i{(int)__builtin_amdgcn_alignbyte(d1, d0, sh), (int)__builtin_amdgcn_alignbyte(d2, d1, sh),
                               (int)__builtin_amdgcn_alignbyte(d3, d2, sh), (int)__builtin_amdgcn_alignbyte(d4, d3, sh)};
                }
            };
            v4i acc = {kc.x, kc.y, kc.z, kc.w}, sum = zero4;
            // (no ring of operand-B registers as in dw_mm_rt: one of three, fetching step ks + 3 behind the MFMA of step ks, took 85 ->
            // 118 VGPRs at 5x5 and measured 1.3 - 2.2x SLOWER on the C >= 16 rows of scripts/time_dw_gemm.py; occupancy hides the
            // LDS latency here)
#pragma unroll
            for (int ks = 0; ks < KSMAX; ++ks) {
                if (ks < KS) {
                    const v4i b = operand(ks);
                    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(wA[ks], b, acc, 0, 0, 0);
                    if constexpr (WZ) sum = __builtin_amdgcn_mfma_i32_16x16x64_i8(4 * ks + g < T ? ones : zero4, b, sum, 0, 0, 0);
                }
            }
            if constexpr (WZ) acc[0] -= wz.x * sum[0], acc[1] -= wz.y * sum[1], acc[2] -= wz.z * sum[2], acc[3] -= wz.w * sum[3];
            const uint32_t d = requant_pack4<MG, XR4>(acc[0], acc[1], acc[2], acc[3], cA, cS, p.lo_f, p.hi_f);
            // the lane's 4 rows are output bytes ch .. ch + 3 from its pixel's first byte (P > 1: row r = byte r of the run of P pixels,
            // pixel r / C, channel r % C); the real ones end at the group's channels or at the image row's last pixel
            const int lim = min(PC, (OW - ox) * C);
            if (live && ch < lim) {
                const size_t opix = ((size_t)(ist * G + gi) * OH + band * BH + oyl) * OW + ox;
                int8_t *dst = out + opix * C + ch;
                if ((C & 3) == 0 && ch + 4 <= lim) {
                    *(uint32_t *)dst = d;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (ch + j < lim) dst[j] = (int8_t)(d >> (8 * j));
                }
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
// The image step as conv_gemm_rt's: G whole images (<= 48 KiB of tiles) or one band of output rows.
bool dw_gemm_plan(DwGemmArgs &a, int H, int W, int C, int KH, int KW, int sh, int sw, int OH, int OW, bool pad_same) {
    return dw_gemm_plan_pads(a, H, W, C, KH, KW, sh, sw, OH, OW, pad_same ? (KH - 1) / 2 : 0, pad_same ? (KW - 1) / 2 : 0);
}
// ... with the window placement given (k_rt.hip conv_rows_plan_pads): the tile is sized from padt, padl, OH and OW
bool dw_gemm_plan_pads(DwGemmArgs &a, int H, int W, int C, int KH, int KW, int sh, int sw, int OH, int OW, int padt, int padl) {
    if (padt < 0 || padl < 0) return false;
    if (H < 1 || W < 1 || C < 2 || KH < 1 || KW < 1 || sh < 1 || sw < 1 || OH < 1 || OW < 1) return false;
    if (KH > 7 || KW > 7 || (W * C) % 4 != 0) return false;
    const int LP = (padl * C + 15) & ~15;
    // bytes read right of the image row: the last window's last tap, the last group's 16 bytes from its start (<= C - 1 past the
    // tap's first channel) and the 4 bytes of the aligned reads
    const int reach = ((OW - 1) * sw - padl + KW) * C + 16 + 4;
    const int ROW = (LP + std::max(W * C, reach) + 15) & ~15;
    auto rows_for = [&](int bh) { return (bh - 1) * sh + KH; };
    a.H = H, a.W = W, a.C = C, a.KH = KH, a.KW = KW, a.sh = sh, a.sw = sw, a.OH = OH, a.OW = OW;
    a.padl = padl, a.padt = padt, a.LP = LP, a.ROW = ROW;
    a.KS = (KH * KW + 3) / 4, a.NBLK = (C + 15) / 16;
    // C <= 8 at stride 1 along the row: P = 16 / C horizontally adjacent output pixels share one 16-row group -- the 16 bytes at
    // the first one's tap are the tap's bytes of all P (the rows past P C meet zero weights)
    a.P = C <= 8 && sw == 1 ? 16 / C : 1;
    constexpr int CAP = 48 * 1024;
    if (rows_for(OH) * ROW <= CAP) {
        a.NBANDS = 1, a.BH = OH, a.RB = rows_for(OH), a.TILE = a.RB * ROW;
        a.G = std::max(1, std::min(16, CAP / a.TILE));
    } else {
        int bh = OH;
        while (bh > 1 && rows_for(bh) * ROW > CAP) --bh;
        const int nb = (OH + bh - 1) / bh;
        bh = (OH + nb - 1) / nb;
        a.BH = bh, a.NBANDS = (OH + bh - 1) / bh, a.RB = rows_for(bh), a.TILE = a.RB * ROW, a.G = 1;
    }
    a.lds = a.G * a.TILE + 256;
    return a.lds <= DW_GEMM_LDS_MAX; // (false: one output row's window rows do not fit)
}

template <int AL, bool WZ, int KSMAX, int MG, uint32_t XR4>
static void launch_dw_gemm_t(const int8_t *in, int8_t *out, const DwGemmArgs &a, int batch, hipStream_t s) {
    int per_cu = 1;
    { // occupancy per (device, LDS bytes), asked once
        static std::mutex mu;
        static std::map<std::pair<int, int>, int> cache;
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> lock(mu);
        auto it = cache.find({dev, a.lds});
        if (it == cache.end()) {
            (void)hipFuncSetAttribute((const void *)dw_gemm_rt<AL, WZ, KSMAX, MG, XR4>, hipFuncAttributeMaxDynamicSharedMemorySize, DW_GEMM_LDS_MAX);
            int n = 1;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, dw_gemm_rt<AL, WZ, KSMAX, MG, XR4>, 256, (size_t)a.lds) != hipSuccess || n < 1) {
                (void)hipGetLastError();
                n = 1;
            }
            it = cache.emplace(std::make_pair(dev, a.lds), n).first;
        }
        per_cu = it->second;
    }
    const long long nsteps = (long long)((batch + a.G - 1) / a.G) * a.NBANDS;
    const long long grid = std::min(nsteps, 256LL * per_cu); // persistent: a workgroup fills its halo once
    MF_LAUNCH((dw_gemm_rt<AL, WZ, KSMAX, MG, XR4>), dim3((unsigned)grid), dim3(256), a.lds, s, in, out, a, batch);
}
template <int AL, bool WZ, int MG, uint32_t XR4>
static void launch_dw_gemm_k(const int8_t *in, int8_t *out, const DwGemmArgs &a, int batch, hipStream_t s) {
    if (a.KS <= 4) launch_dw_gemm_t<AL, WZ, 4, MG, XR4>(in, out, a, batch, s);
    else if (a.KS <= 7) launch_dw_gemm_t<AL, WZ, 7, MG, XR4>(in, out, a, batch, s);
    else launch_dw_gemm_t<AL, WZ, 13, MG, XR4>(in, out, a, batch, s);
}
template <int AL, int MG, uint32_t XR4>
static void launch_dw_gemm_w(const int8_t *in, int8_t *out, const DwGemmArgs &a, bool wz, int batch, hipStream_t s) {
    if (wz) launch_dw_gemm_k<AL, true, MG, XR4>(in, out, a, batch, s);
    else launch_dw_gemm_k<AL, false, MG, XR4>(in, out, a, batch, s);
}
void launch_dw_gemm(const int8_t *in, int8_t *out, const DwGemmArgs &a, bool wz, int batch, hipStream_t s) {
    if (batch <= 0) return;
    if (a.C % 16 == 0) MF_DISPATCH4(a.magic, a.xr, launch_dw_gemm_w, (in, out, a, wz, batch, s), 16)
    else if (a.C % 8 == 0) MF_DISPATCH4(a.magic, a.xr, launch_dw_gemm_w, (in, out, a, wz, batch, s), 8)
    else if (a.C % 4 == 0) MF_DISPATCH4(a.magic, a.xr, launch_dw_gemm_w, (in, out, a, wz, batch, s), 4)
    else MF_DISPATCH4(a.magic, a.xr, launch_dw_gemm_w, (in, out, a, wz, batch, s), 1)
}

} // namespace k
} // namespace mf
