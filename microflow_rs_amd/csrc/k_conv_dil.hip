// k_conv_dil.hip -- Conv2D with dilation factors (dh, dw) != (1, 1) on the int8 matrix pipe (include/microflow_amd.h:
// mf_conv_2d_dilated_create; the reference has no dilation).  Tap (ky, kx) of output (oy, ox) reads input
// (oy sh - padt + ky dh, ox sw - padl + kx dw); a tap outside the image reads the input zero point.
//
// conv_gemm_rt (k_conv_gemm.hip) rests on the KW C bytes of a filter row being ONE contiguous run of the staged image row.  With
// dw > 1 they are KW runs of C bytes, dw C apart.  This kernel restores the run by the way it stages a row:
//
//   planes  : with xe = x + padl the halo-extended column, a tile row holds dw planes; plane f holds the columns xe % dw == f in
//             order, C bytes each (wimage.cpp conv_dil_tile).  The taps of a window are xe = ox sw + kx dw: ONE plane, (ox sw) % dw,
//             at KW consecutive positions from (ox sw) / dw -- KW C contiguous bytes again, for any stride, because the phase depends
//             on ox alone.  The window's LDS byte is (row) + LP + phase PP + position C.
//   rows    : dh only moves the filter rows apart: table entries are ky dh ROW + j, a tile has (BH - 1) sh + (KH - 1) dh + 1 rows and
//             two bands share (KH - 1) dh + 1 - sh of them.
//   staging : dw > 1: the de-interleaving copy, one 16-byte (C % 16 == 0) or 4-byte unit per lane from consecutive global addresses to
//             plane (xe % dw), position (xe / dw).  dw == 1 (row-only dilation): one plane, the row copied as conv_gemm_rt does, by
//             LDS-DMA when W C % 16 == 0.  Everything outside the image is the input zero point: the whole tile once per workgroup, and
//             in band mode the rows a band holds above or below the image once per step.
//   K, weights, WZ, N slices, walkers, epilogue, stores: conv_gemm_rt's, unchanged (the argument block holds a ConvGemmArgs and the
//             weight image is conv_gemm_weight_image's).  Operand B at 16-byte (C % 16 == 0) or dword (C % 4 == 0) granularity; other
//             channel counts stay on conv2d_generic: the de-interleaving copy moves whole pixels, and a pixel that is no whole number
//             of dwords would make it a byte copy.
#include "k_common.hpp"
#include "wimage.hpp"

#include <algorithm>
#include <map>
#include <mutex>

namespace mf {
namespace k {

template <int AL, bool WZ, int MG, uint32_t XR4>
__global__ __launch_bounds__(256) void conv_dil_rt(const int8_t *__restrict__ in, int8_t *__restrict__ out, ConvDilArgs q, int batch) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const ConvGemmArgs &p = q.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = p.C, N = p.N, KS = p.KS, TB = p.TB, ROW = p.ROW, TILE = p.TILE, G = p.G, RB = p.RB;
    const int H = p.H, OH = p.OH, OW = p.OW, ROWB = p.W * C, BH = p.BH, NBANDS = p.NBANDS;
    const int DW = q.dw, PP = q.PP;
    const int slice = blockIdx.x % p.NSL, walker = blockIdx.x / p.NSL, nwalk = gridDim.x / p.NSL;
    const int nt0 = slice * p.NTS, nts = min(p.NTS, p.NT - nt0), nblk = (nts + TB - 1) / TB;
    uint8_t *T = lds + p.xoff;
    const uint32_t izp4 = p.izp4;
    const uint4 izp16 = make_uint4(izp4, izp4, izp4, izp4);

    // resident weights: the slice's tiles are one contiguous run of the image (whole 1 KiB pieces)
    const int8_t *wsrc = (const int8_t *)p.wimg + (size_t)nt0 * KS * 1024;
    for (int b = wave * 64; b < nts * KS * 64; b += 256) dma16(wsrc + (size_t)(b + lane) * 16, lds + b * 16);
    for (int i = tid; i < (G * TILE + 256) / 16; i += 256) ((uint4 *)T)[i] = izp16;
    for (int i = tid; i < KS * 4; i += 256) ((int *)(lds + p.toff))[i] = p.tap[i];
    if constexpr (WZ)
        for (int i = tid; i < KS * 16; i += 256) ((uint32_t *)(lds + p.moff))[i] = p.kmask[i];
    const int *tab = (const int *)(lds + p.toff);
    const int col = lane & 15, g = lane >> 4;
    const int nsteps = ((batch + G - 1) / G) * NBANDS;
    const v4i ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    constexpr int U = AL == 16 ? 16 : 4;                 // bytes per unit of the de-interleaving copy
    const int CU = C / U, NU = p.W * CU;                 // units per pixel, per image row
    wg_sync();
    for (int step = walker; step < nsteps; step += nwalk) {
        const int band = step % NBANDS, ist = step / NBANDS;
        const int yfirst = band * BH * p.sh - p.padt;   // input row held by tile row 0
        wg_sync();                                       // the previous step's reads of the tile are done
        for (int gi = 0; gi < G; ++gi) {
            const long img = (long)ist * G + gi;
            if (img >= batch) break;
            for (int r = wave; r < RB; r += 4) {
                const int y = yfirst + r;
                uint8_t *row = T + gi * TILE + r * ROW;
                if (y >= 0 && y < H) {
                    const int8_t *src = in + (img * H + y) * (long)ROWB;
                    if (DW == 1) {                       // one plane: the row as it is, behind the left halo
                        uint8_t *dst = row + p.LP + p.padl * C;
                        if ((ROWB & 15) == 0) {
                            for (int o = 0; o < ROWB; o += 1024)
                                if (o + lane * 16 < ROWB) dma16(src + o + lane * 16, dst + o);
                        } else {
                            for (int o = lane * 4; o < ROWB; o += 256) *(uint32_t *)(dst + o) = *(const uint32_t *)(src + o);
                        }
                    } else {                             // pixel x to plane (x + padl) % dw, position (x + padl) / dw
                        for (int i = lane; i < NU; i += 64) {
                            const int x = i / CU, cu = i - x * CU, xe = x + p.padl;
                            const int pos = xe / DW, ph = xe - pos * DW;
                            uint8_t *dst = row + ph * PP + pos * C + cu * U;
                            if constexpr (AL == 16) *(uint4 *)dst = *(const uint4 *)(src + (size_t)i * 16);
                            else *(uint32_t *)dst = *(const uint32_t *)(src + (size_t)i * 4);
                        }
                    }
                } else if (NBANDS > 1) {                 // band mode: this tile row is padding in this step only
                    for (int o = lane * 16; o < ROW; o += 1024) *(uint4 *)(row + o) = izp16;
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's DMAs (the first time: and the weights') have landed ...
        wg_sync();                                       // ... and every other wave's
        const int gvalid = min(G, batch - ist * G);
        const int rows_here = min(BH, OH - band * BH);
        const int bp = BH * OW, npix = gvalid * bp;      // (rows past the image are masked below)
        for (int chunk = wave; chunk * 16 < npix; chunk += 4) {
            const int pp = chunk * 16 + col;
            const int pc = pp < npix ? pp : npix - 1;
            const int gi = pc / bp, rr = pc - gi * bp;
            const int oyl = rr / OW, ox = rr - oyl * OW;
            const bool live = pp < npix && oyl < rows_here;
            const int xe0 = ox * p.sw, pos0 = xe0 / DW, ph0 = xe0 - pos0 * DW; // the window's first column: its plane and position
            const int wbase = p.xoff + gi * TILE + (oyl * p.sh) * ROW + p.LP + ph0 * PP + pos0 * C; // the window's LDS byte
            // operand B of k step ks: the 16 bytes at (window) + (table offset)
            auto operand = [&](int ks) -> v4i {
                const int off = wbase + tab[ks * 4 + g];
                if constexpr (AL == 16) {
                    return *(const v4i *)(lds + off);
                } else {
                    const uint32_t *w4 = (const uint32_t *)(lds + off);
                    return v4i{(int)w4[0], (int)w4[1], (int)w4[2], (int)w4[3]};
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
            const size_t opix = ((size_t)(ist * G + gi) * OH + band * BH + oyl) * OW + ox;
            for (int blk = 0; blk < nblk; ++blk) {
                const int lt0 = blk * TB, tb = min(TB, nts - lt0);
                v4i acc[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i < tb) {
                        const int4 kc = magic4<MG>(*(const int4 *)(p.Kc + (nt0 + lt0 + i) * 16 + g * 4));
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
                    const int ch = (nt0 + lt0 + i) * 16 + g * 4; // the lane's 4 output channels
                    if (i < tb && ch < N) {
                        v4i a = acc[i];
                        if constexpr (WZ) {
                            const int4 wz = *(const int4 *)(p.wzp + ch);
                            a[0] -= wz.x * rowsum, a[1] -= wz.y * rowsum, a[2] -= wz.z * rowsum, a[3] -= wz.w * rowsum;
                        }
                        const uint32_t d = requant_pack4<MG, XR4>(a[0], a[1], a[2], a[3], *(const float4 *)(p.A + ch), *(const float4 *)(p.S + ch),
                                                                  p.lo_f, p.hi_f);
                        if (live) {
                            int8_t *dst = out + opix * N + ch;
                            if ((N & 3) == 0) {
                                *(uint32_t *)dst = d;
                            } else {
#pragma unroll
                                for (int j = 0; j < 4; ++j)
                                    if (ch + j < N) dst[j] = (int8_t)(d >> (8 * j));
                            }
                        }
                    }
                }
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
// conv_gemm_plan_pads' search -- the widest N slice that leaves room for a second workgroup per CU, else the widest that fits; G whole
// images (<= 48 KiB of tiles) or bands of output rows -- over the plane tile: rows of conv_dil_tile's ROW bytes, (bh - 1) sh + (KH - 1)
// dh + 1 of them for bh output rows.  The class: C % 4 == 0 (operand B and the de-interleaving copy in whole dwords), factors and
// effective extents that keep every offset far inside an int.
bool conv_dil_plan(ConvDilArgs &d, std::vector<int> &tap, std::vector<uint32_t> &mask, int H, int W, int C, int N, int KH, int KW, int sh,
                   int sw, int dh, int dw, int OH, int OW, int padt, int padl, bool wz) {
    if (padt < 0 || padl < 0 || dh < 1 || dw < 1) return false;
    if (H < 1 || W < 1 || C < 1 || N < 1 || KH < 1 || KW < 1 || sh < 1 || sw < 1 || OH < 1 || OW < 1) return false;
    if (C % 4 != 0) return false;
    const long long KEH = (long long)(KH - 1) * dh + 1, KEW = (long long)(KW - 1) * dw + 1;
    if (KEH > 4096 || KEW > 4096 || (long long)KW * C > 8192) return false;
    const wimage::ConvDilTile t = wimage::conv_dil_tile(W, C, KW, sw, dw, OW, padl);
    const int KS = (KH * t.KWCP + 63) / 64, NT = (N + 15) / 16;
    if (KS > CONV_GEMM_KS_MAX || t.ROW > CONV_GEMM_LDS_MAX) return false;
    const int ROW = (int)t.ROW;
    const int tabb = KS * 16 + (wz ? KS * 64 : 0);
    auto rows_for = [&](int bh) { return (long long)(bh - 1) * sh + KEH; };
    ConvGemmArgs &a = d.g;
    a.H = H, a.W = W, a.C = C, a.N = N, a.KH = KH, a.KW = KW, a.sh = sh, a.sw = sw, a.OH = OH, a.OW = OW;
    a.padl = padl, a.padt = padt, a.KWCP = t.KWCP, a.KS = KS, a.NT = NT, a.LP = t.LP, a.ROW = ROW;
    d.dh = dh, d.dw = dw, d.PP = (int)t.PP;
    for (int pass = 0; pass < 2; ++pass) {
        const int lmax = pass == 0 ? 80 * 1024 : CONV_GEMM_LDS_MAX;
        for (int NTS = NT; NTS >= 1; --NTS) {
            const int NSL = (NT + NTS - 1) / NTS;
            if (NSL > 1 && (NT + NSL - 1) / NSL != NTS) continue; // balanced slices only
            const int wbytes = NTS * KS * 1024;
            const long long cap = std::min(lmax - wbytes - tabb - 256, 48 * 1024);
            // (the first pass also wants bands of at least 4 output rows: thinner bands leave waves without a 16-pixel chunk)
            if (cap < rows_for(pass == 0 ? std::min(OH, 4) : 1) * ROW) continue;
            if (rows_for(OH) * ROW <= cap) {
                a.NBANDS = 1, a.BH = OH, a.RB = (int)rows_for(OH), a.TILE = a.RB * ROW;
                a.G = (int)std::max(1LL, std::min(16LL, cap / a.TILE));
            } else {
                int bh = OH;
                while (bh > 1 && rows_for(bh) * ROW > cap) --bh;
                const int nb = (OH + bh - 1) / bh;
                bh = (OH + nb - 1) / nb;
                a.BH = bh, a.NBANDS = (OH + bh - 1) / bh, a.RB = (int)rows_for(bh), a.TILE = a.RB * ROW, a.G = 1;
            }
            a.NTS = NTS, a.NSL = NSL, a.TB = std::min(4, NTS);
            a.xoff = wbytes, a.toff = a.xoff + a.G * a.TILE + 256, a.moff = a.toff + KS * 16;
            a.lds = a.toff + tabb;
            wimage::conv_dil_tables(KH, KW, C, dh, ROW, tap, mask);
            return true;
        }
    }
    return false;
}

template <int AL, bool WZ, int MG, uint32_t XR4>
static void launch_conv_dil_t(const int8_t *in, int8_t *out, const ConvDilArgs &a, int batch, hipStream_t s) {
    int per_cu = 1;
    { // occupancy per (device, LDS bytes), asked once; the attribute is the whole budget, so no shape lowers it for another
        static std::mutex mu;
        static std::map<std::pair<int, int>, int> cache;
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> lock(mu);
        auto it = cache.find({dev, a.g.lds});
        if (it == cache.end()) {
            (void)hipFuncSetAttribute((const void *)conv_dil_rt<AL, WZ, MG, XR4>, hipFuncAttributeMaxDynamicSharedMemorySize, CONV_GEMM_LDS_MAX);
            int n = 1;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, conv_dil_rt<AL, WZ, MG, XR4>, 256, (size_t)a.g.lds) != hipSuccess || n < 1) {
                (void)hipGetLastError();
                n = 1;
            }
            it = cache.emplace(std::make_pair(dev, a.g.lds), n).first;
        }
        per_cu = it->second;
    }
    const long long nsteps = (long long)((batch + a.g.G - 1) / a.g.G) * a.g.NBANDS;
    long long walkers = std::max(1LL, 256LL * per_cu / a.g.NSL); // persistent: the resident slice is staged once per workgroup
    walkers = std::min(walkers, nsteps);
    MF_LAUNCH((conv_dil_rt<AL, WZ, MG, XR4>), dim3((unsigned)(walkers * a.g.NSL)), dim3(256), a.g.lds, s, in, out, a, batch);
}
template <int AL, int MG, uint32_t XR4>
static void launch_conv_dil_w(const int8_t *in, int8_t *out, const ConvDilArgs &a, bool wz, int batch, hipStream_t s) {
    if (wz) launch_conv_dil_t<AL, true, MG, XR4>(in, out, a, batch, s);
    else launch_conv_dil_t<AL, false, MG, XR4>(in, out, a, batch, s);
}
void launch_conv_dil(const int8_t *in, int8_t *out, const ConvDilArgs &a, bool wz, int batch, hipStream_t s) {
    if (batch <= 0) return;
    const int magic = a.g.magic, xr = a.g.xr;
    if (a.g.C % 16 == 0) MF_DISPATCH4(magic, xr, launch_conv_dil_w, (in, out, a, wz, batch, s), 16)
    else MF_DISPATCH4(magic, xr, launch_conv_dil_w, (in, out, a, wz, batch, s), 4)
}

} // namespace k
} // namespace mf
