// k_conv_pool.hip -- a Conv2D and the AveragePool2D behind it in one launch (microflow::ops::conv_2d, src/ops/conv_2d.rs:28-108;
// microflow::ops::average_pool_2d, src/ops/average_pool_2d.rs:29-66): the stages of LeNet-style CNNs.  The convolution's output, the
// widest tensor of such a network, is written by one launch and read back by the next only to be averaged; here it lives in LDS.
//
//   step    : G whole images, or one band of PB pooled rows of one image (kernels.hpp conv_pool_band: the convolution rows the band's
//             windows read; overlapping windows recompute the shared rows at a band edge).  Persistent workgroups walk the steps.
//   phase A : conv_gemm_rt's staging and product (k_conv_gemm.hip) with the whole weight image resident: the input tile inside its
//             input-zero-point halo, K' = [ky][pad16(KW C)], the [KS][4] tap table, the operand from aligned reads (AL = 16 / 4 / 1),
//             the ones-tile MFMA and the mask table for filter zero points, requant_pack4 with the convolution's own constants.  Each
//             lane's packed dword -- the bytes the convolution's own launch would store -- goes to Y[g][row][ox][NP] in LDS.
//   phase B : one work item is (image, pooled pixel, channel quad): one dword of Y per in-range tap, summed per byte with masked
//             v_dot4 as avgpool_c4 does, then avgpool_generic's arithmetic (k_generic.hip) value by value with the pool's own
//             constants.  The pooled bytes of a step are one contiguous range of the output: dwords where N % 4 == 0, else one byte
//             per real channel.
//
// Three barriers per step: top of the step (the previous step's reads of the tile and of Y are done), tile staged, Y complete.
#include "k_common.hpp"

#include <algorithm>
#include <map>
#include <mutex>

namespace mf {
namespace k {

template <int AL, bool WZ, int MG, uint32_t XR4>
__global__ __launch_bounds__(256) void conv_pool_rt(const int8_t *__restrict__ in, int8_t *__restrict__ out, ConvPoolArgs p, int batch) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = p.C, N = p.N, KS = p.KS, TB = p.TB, ROW = p.ROW, TILE = p.TILE, G = p.G, RB = p.RB, NT = p.NT;
    const int H = p.H, OH = p.OH, OW = p.OW, ROWB = p.W * C, NB = p.NB, NP = p.NP, YIMG = p.YIMG;
    const int POH = p.POH, POW = p.POW, NQ = (N + 3) >> 2;
    const int nblk = (NT + TB - 1) / TB;
    uint8_t *T = lds + p.xoff;
    const uint32_t izp4 = p.izp4;
    const PoolArgs &pl = p.pool;

    // resident weights: the whole image (1 KiB pieces)
    for (int b = wave * 64; b < NT * KS * 64; b += 256) dma16((const int8_t *)p.wimg + (size_t)(b + lane) * 16, lds + b * 16);
    for (int i = tid; i < (G * TILE + 256) / 16; i += 256) ((uint4 *)T)[i] = make_uint4(izp4, izp4, izp4, izp4);
    for (int i = tid; i < KS * 4; i += 256) ((int *)(lds + p.toff))[i] = p.tap[i];
    if constexpr (WZ)
        for (int i = tid; i < KS * 16; i += 256) ((uint32_t *)(lds + p.moff))[i] = p.kmask[i];
    // the convolution's per-channel constants [Kc | A | S | wzp][NT 16]: a chunk reads them at LDS latency, not through the L2
    for (int i = tid; i < NT * 16; i += 256) {
        int *c = (int *)(lds + p.coff);
        c[i] = p.Kc[i], c[NT * 16 + i] = __float_as_int(p.A[i]), c[NT * 32 + i] = __float_as_int(p.S[i]), c[NT * 48 + i] = p.wzp[i];
    }
    const int *tab = (const int *)(lds + p.toff);
    const uint8_t *cKc = lds + p.coff, *cA = cKc + NT * 64, *cS = cKc + NT * 128, *cZ = cKc + NT * 192;
    const int col = lane & 15, g = lane >> 4;
    const int nsteps = ((batch + G - 1) / G) * NB;
    const v4i ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    const bool dword_out = (N & 3) == 0 && ((uintptr_t)out & 3) == 0;
    wg_sync();
    for (int step = blockIdx.x; step < nsteps; step += gridDim.x) {
        const int band = step % NB, ist = step / NB;
        int py0, py1, c0, c1;
        conv_pool_band(OH, POH, p.PB, p.psh, p.pshy, p.PFH, band, py0, py1, c0, c1);
        const int yfirst = c0 * p.sh - p.padt;          // input row held by tile row 0
        wg_sync();                                       // the previous step's reads of the tile and of Y are done
        const int gvalid = min(G, batch - ist * G);
        const int rlo = yfirst < 0 ? -yfirst : 0, rhi = min(RB, H - yfirst); // the tile rows [rlo, rhi) lie inside the image
        if ((ROWB & 15) == 0) {
            for (int gi = 0; gi < gvalid; ++gi)
                for (int r = rlo + wave; r < rhi; r += 4) {
                    const int8_t *src = in + (((long)ist * G + gi) * H + yfirst + r) * (long)ROWB;
                    uint8_t *dst = T + gi * TILE + r * ROW + p.LP;
                    for (int o = 0; o < ROWB; o += 1024)
                        if (o + lane * 16 < ROWB) dma16(src + o + lane * 16, dst + o);
                }
        } else {
            // dword loads: the step's rows as one index space, four loads in flight per lane before the first store (a row of a small
            // image is a few dwords: a wave per row would wait out one memory latency per row)
            const int RW = ROWB >> 2, nr = rhi - rlo, per = nr * RW, total = gvalid * per;
            for (int base = tid; base < total; base += 1024) {
                uint32_t v[4];
                int at[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int idx = base + u * 256;
                    if (idx < total) {
                        const int gi = idx / per, w = idx - gi * per, r = w / RW, c = w - r * RW;
                        v[u] = *(const uint32_t *)(in + (((long)ist * G + gi) * H + yfirst + rlo + r) * (long)ROWB + c * 4);
                        at[u] = gi * TILE + (rlo + r) * ROW + p.LP + c * 4;
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (base + u * 256 < total) *(uint32_t *)(T + at[u]) = v[u];
            }
        }
        if (NB > 1)                                      // a band's rows outside the image: the input zero point again
            for (int gi = 0; gi < gvalid; ++gi)
                for (int r = wave; r < RB; r += 4)
                    if (r < rlo || r >= rhi)
                        for (int o = lane * 4; o < ROWB; o += 256) *(uint32_t *)(T + gi * TILE + r * ROW + p.LP + o) = izp4;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's DMAs (the first time: and the weights') have landed ...
        wg_sync();                                       // ... and every other wave's
        // ---- phase A: the band's convolution rows c0 .. c1 - 1 of every image of the step into Y ----
        const int bp = (c1 - c0) * OW, npix = gvalid * bp;
        for (int chunk = wave; chunk * 16 < npix; chunk += 4) {
            const int pp = chunk * 16 + col;
            const int pc = pp < npix ? pp : npix - 1;
            const int gi = pc / bp, rr = pc - gi * bp;
            const int oyl = rr / OW, ox = rr - oyl * OW;
            const bool live = pp < npix;
            const int wbase = p.xoff + gi * TILE + (oyl * p.sh) * ROW + p.LP + (ox * p.sw - p.padl) * C; // the window's LDS byte
            // operand B of k step ks: the 16 bytes at (window) + (table offset), from aligned reads
            auto operand = [&](int ks) -> v4i {
                const int off = wbase + tab[ks * 4 + g];
                if constexpr (AL == 16) {
                    return *(const v4i *)(lds + off);
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
            int rowsum = 0;
            if constexpr (WZ) {
                v4i acc = {0, 0, 0, 0};
                for (int ks = 0; ks < KS; ++ks) {
                    const v4i m = *(const v4i *)(lds + p.moff + (ks * 4 + g) * 16);
                    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, operand(ks) & m, acc, 0, 0, 0);
                }
                rowsum = acc[0];
            }
            uint8_t *ypix = lds + p.yoff + gi * YIMG + rr * NP;
            for (int blk = 0; blk < nblk; ++blk) {
                const int lt0 = blk * TB, tb = min(TB, NT - lt0);
                v4i acc[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i < tb) {
                        const int4 kc = magic4<MG>(*(const int4 *)(cKc + ((lt0 + i) * 16 + g * 4) * 4));
                        acc[i] = v4i{kc.x, kc.y, kc.z, kc.w};
                    }
                }
                for (int ks = 0; ks < KS; ++ks) {
                    const v4i b = operand(ks);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (i < tb) acc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(*(const v4i *)(lds + (((lt0 + i) * KS + ks) * 64 + lane) * 16), b, acc[i], 0, 0, 0);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int ch = (lt0 + i) * 16 + g * 4; // the lane's 4 output channels
                    if (i < tb && ch < N) {
                        v4i a = acc[i];
                        if constexpr (WZ) {
                            const int4 wz = *(const int4 *)(cZ + ch * 4);
                            a[0] -= wz.x * rowsum, a[1] -= wz.y * rowsum, a[2] -= wz.z * rowsum, a[3] -= wz.w * rowsum;
                        }
                        const uint32_t d = requant_pack4<MG, XR4>(a[0], a[1], a[2], a[3], *(const float4 *)(cA + ch * 4), *(const float4 *)(cS + ch * 4),
                                                                  p.lo_f, p.hi_f);
                        if (live) *(uint32_t *)(ypix + ch) = d; // (the quad's bytes past N, if any, are read by no one)
                    }
                }
            }
        }
        wg_sync();                                       // Y is complete
        // ---- phase B: the band's pooled rows py0 .. py1 - 1 from Y ----
        const int nprow = py1 - py0, items = gvalid * nprow * POW * NQ;
        for (int it = tid; it < items; it += 256) {
            const int q = it % NQ;
            int t = it / NQ;
            const int px = t % POW;
            t /= POW;
            const int pr = t % nprow, gi = t / nprow;
            const int py = py0 + pr;
            const uint8_t *yb = lds + p.yoff + gi * YIMG + q * 4;
            int s0 = 0, s1 = 0, s2 = 0, s3 = 0, len = 0;
            for (int ky = 0; ky < p.PFH; ++ky) {
                const int iy = py * p.psh + ky - p.pshy;
                if (iy < 0 || iy >= OH) continue;
                for (int kx = 0; kx < p.PFW; ++kx) {
                    const int ix = px * p.psw + kx - p.pshx;
                    if (ix >= 0 && ix < OW) {
                        const uint32_t v = *(const uint32_t *)(yb + ((iy - c0) * OW + ix) * NP);
                        s0 = sdot4(v, 0x00000001u, s0), s1 = sdot4(v, 0x00000100u, s1);
                        s2 = sdot4(v, 0x00010000u, s2), s3 = sdot4(v, 0x01000000u, s3);
                        ++len;
                    }
                }
            }
            const float inv = __fdiv_rn(1.0f, (float)len);
            const int sums[4] = {s0, s1, s2, s3};
            int r4[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float x = __fmul_rn(inv, (float)(sums[k] + pl.bias * len));
                const float y = __fadd_rn(__fmul_rn(pl.c0, x), pl.c1);
                const float r = __fadd_rn(y, __builtin_copysignf(0x1.fffffep-2f, y));
                int v = (r != r) ? 0 : (int)__builtin_amdgcn_fmed3f(r, pl.sat_lo, pl.sat_hi); // NaN (len == 0) -> 0
                v = max(v, pl.lo);
                r4[k] = min(v, pl.hi);
            }
            const uint32_t d = pack4(r4[0], r4[1], r4[2], r4[3]) ^ (0x01010101u * (uint32_t)pl.xr);
            int8_t *dst = out + ((((size_t)ist * G + gi) * POH + py) * POW + px) * (size_t)N + q * 4;
            if (dword_out) {
                *(uint32_t *)dst = d;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (q * 4 + j < N) dst[j] = (int8_t)(d >> (8 * j));
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
// The whole weight image, then per step G tiles and G images of Y (at most 16 images and 48 KiB of tiles, as conv_gemm_plan): inside
// 80 KiB where that holds one whole image (two workgroups per CU), else the widest that fits, else bands of PB pooled rows -- PB as
// large as fits, the bands evened out.
bool conv_pool_plan(ConvPoolArgs &a, std::vector<int> &tap, std::vector<uint32_t> &mask, int H, int W, int C, int N, int KH, int KW, int sh, int sw,
                    int OH, int OW, bool pad_same, bool wz, int PFH, int PFW, int psh, int psw, int POH, int POW, bool pool_same) {
    if (H < 1 || W < 1 || C < 1 || N < 1 || KH < 1 || KW < 1 || sh < 1 || sw < 1 || OH < 1 || OW < 1) return false;
    if (PFH < 1 || PFW < 1 || psh < 1 || psw < 1 || POH < 1 || POW < 1) return false;
    if (POH * POW < 2) return false;                     // (a global pool belongs to the tail and pool_fc_chain groups)
    if ((W * C) % 4 != 0) return false;                  // whole-dword image rows
    const int pshy = pool_same ? (PFH - 1) / 2 : 0, pshx = pool_same ? (PFW - 1) / 2 : 0;
    if (!pool_same && ((POH - 1) * psh + PFH > OH || (POW - 1) * psw + PFW > OW)) return false; // a VALID window leaves the tensor
    if ((POH - 1) * psh - pshy >= OH || (POW - 1) * psw - pshx >= OW) return false;              // a window with no tap at all
    const int KWC = KW * C, KWCP = (KWC + 15) & ~15, KS = (KH * KWCP + 63) / 64, NT = (N + 15) / 16;
    if (KS > CONV_GEMM_KS_MAX) return false;
    const int padl = pad_same ? (KW - 1) / 2 : 0, padt = pad_same ? (KH - 1) / 2 : 0;
    const int LP = (padl * C + 15) & ~15;
    // bytes read right of the image row: the last window's padded filter row (+ the 4 bytes of the aligned reads)
    const int over = std::max(0, ((OW - 1) * sw - padl) * C + KWCP + 4 - W * C);
    const int ROW = ((LP + W * C + over + 15) & ~15) + 16;
    const int tabb = KS * 16 + (wz ? KS * 64 : 0) + NT * 256; // tap table, masks, the constants [Kc | A | S | wzp][NT 16]
    const int NP4 = (N + 3) / 4, NP = 4 * (NP4 % 2 == 0 ? NP4 + 1 : NP4); // an odd number of dwords per pixel: 16 pixels, 16 banks
    const long long wbytes = (long long)NT * KS * 1024;
    a.H = H, a.W = W, a.C = C, a.N = N, a.KH = KH, a.KW = KW, a.sh = sh, a.sw = sw, a.OH = OH, a.OW = OW;
    a.padl = padl, a.padt = padt, a.KWCP = KWCP, a.KS = KS, a.NT = NT, a.TB = std::min(4, NT), a.LP = LP, a.ROW = ROW;
    a.PFH = PFH, a.PFW = PFW, a.psh = psh, a.psw = psw, a.POH = POH, a.POW = POW, a.pshy = pshy, a.pshx = pshx, a.NP = NP;
    auto rows_for = [&](int cb) { return (cb - 1) * sh + KH; };
    auto ybytes = [&](int cb) { return ((long long)cb * OW * NP + 15) & ~15LL; };
    // the most convolution rows a band of `pb` pooled rows reads
    auto conv_rows = [&](int pb) {
        int cb = 0;
        for (int b = 0; b * pb < POH; ++b) {
            int py0, py1, c0, c1;
            conv_pool_band(OH, POH, pb, psh, pshy, PFH, b, py0, py1, c0, c1);
            cb = std::max(cb, c1 - c0);
        }
        return cb;
    };
    auto finish = [&](int G, int PB, int CB) {
        a.G = G, a.PB = PB, a.NB = (POH + PB - 1) / PB, a.CB = CB, a.RB = rows_for(CB), a.TILE = a.RB * ROW, a.YIMG = (int)ybytes(CB);
        a.xoff = (int)wbytes, a.yoff = a.xoff + G * a.TILE + 256, a.toff = a.yoff + G * a.YIMG, a.moff = a.toff + KS * 16;
        a.coff = a.moff + (wz ? KS * 64 : 0), a.lds = a.toff + tabb;
        tap.assign((size_t)KS * 4, 0);
        mask.assign((size_t)KS * 16, 0);
        for (int ks = 0; ks < KS; ++ks)
            for (int gg = 0; gg < 4; ++gg) {
                const int k0 = ks * 64 + gg * 16, ky = k0 / KWCP, j = k0 % KWCP;
                if (ky >= KH) continue;                  // beyond K': zero weights, offset 0, no window bytes
                tap[(size_t)ks * 4 + gg] = ky * ROW + j;
                for (int i = 0; i < 16; ++i)
                    if (j + i < KWC) mask[(size_t)(ks * 4 + gg) * 4 + i / 4] |= 0xffu << (8 * (i & 3));
            }
        return true;
    };
    const int cb_all = conv_rows(POH);
    const long long tile_all = (long long)rows_for(cb_all) * ROW, per_img = tile_all + ybytes(cb_all);
    for (int pass = 0; pass < 2; ++pass) {
        const long long avail = (pass == 0 ? 80 * 1024 : CONV_GEMM_LDS_MAX) - wbytes - tabb - 256;
        if (tile_all > 48 * 1024 || avail < per_img) continue;
        const int G = (int)std::min<long long>(std::min<long long>(16, 48 * 1024 / tile_all), avail / per_img);
        return finish(G, POH, cb_all);
    }
    const long long avail = CONV_GEMM_LDS_MAX - wbytes - tabb - 256;
    auto fits = [&](int pb) {
        const int cb = conv_rows(pb);
        const long long tile = (long long)rows_for(cb) * ROW;
        return tile <= 48 * 1024 && tile + ybytes(cb) <= avail;
    };
    int pb = POH;
    while (pb > 1 && !fits(pb)) --pb;
    if (!fits(pb)) return false;                         // the weights do not fit whole beside a band of one pooled row
    const int nb = (POH + pb - 1) / pb;
    pb = (POH + nb - 1) / nb;                            // evened out (not larger than the one that fits)
    while (pb > 1 && !fits(pb)) --pb;                    // (an evened band may read one more convolution row at another phase of the stride)
    return finish(1, pb, conv_rows(pb));
}

template <int AL, bool WZ, int MG, uint32_t XR4>
static void launch_conv_pool_t(const int8_t *in, int8_t *out, const ConvPoolArgs &a, int batch, hipStream_t s) {
    int per_cu = 1;
    { // occupancy per (device, LDS bytes), asked once; the attribute is the whole budget, so no shape lowers it for another
        static std::mutex mu;
        static std::map<std::pair<int, int>, int> cache;
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> lock(mu);
        auto it = cache.find({dev, a.lds});
        if (it == cache.end()) {
            (void)hipFuncSetAttribute((const void *)conv_pool_rt<AL, WZ, MG, XR4>, hipFuncAttributeMaxDynamicSharedMemorySize, CONV_GEMM_LDS_MAX);
            int n = 1;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, conv_pool_rt<AL, WZ, MG, XR4>, 256, (size_t)a.lds) != hipSuccess || n < 1) {
                (void)hipGetLastError();
                n = 1;
            }
            it = cache.emplace(std::make_pair(dev, a.lds), n).first;
        }
        per_cu = it->second;
    }
    const long long nsteps = (long long)((batch + a.G - 1) / a.G) * a.NB;
    const long long walkers = std::min(std::max(1LL, 256LL * per_cu), nsteps); // persistent: the weights are staged once per workgroup
    MF_LAUNCH((conv_pool_rt<AL, WZ, MG, XR4>), dim3((unsigned)walkers), dim3(256), a.lds, s, in, out, a, batch);
}
template <int AL, int MG, uint32_t XR4>
static void launch_conv_pool_w(const int8_t *in, int8_t *out, const ConvPoolArgs &a, bool wz, int batch, hipStream_t s) {
    if (wz) launch_conv_pool_t<AL, true, MG, XR4>(in, out, a, batch, s);
    else launch_conv_pool_t<AL, false, MG, XR4>(in, out, a, batch, s);
}
void launch_conv_pool(const int8_t *in, int8_t *out, const ConvPoolArgs &a, bool wz, int batch, hipStream_t s) {
    if (batch <= 0) return;
    if (a.C % 16 == 0) MF_DISPATCH4(a.magic, a.xr, launch_conv_pool_w, (in, out, a, wz, batch, s), 16)
    else if (a.C % 4 == 0) MF_DISPATCH4(a.magic, a.xr, launch_conv_pool_w, (in, out, a, wz, batch, s), 4)
    else MF_DISPATCH4(a.magic, a.xr, launch_conv_pool_w, (in, out, a, wz, batch, s), 1)
}

} // namespace k
} // namespace mf
