// k_conv_gemm.hip -- Conv2D of ANY channel count C and output count N on the int8 matrix pipe (microflow::ops::conv_2d,
// src/ops/conv_2d.rs:28-108: const generics over every shape).
//
// The shape-specialised Conv2D kernels take corners of that space (conv_rows_lds: C < 16, N <= 64, a small image;
// conv_mm_rt: C % 16 == 0, N % 4 == 0, weights <= 96 KiB; pw_rt; conv1x1_rowwave); every other Conv2D with finite constants
// and whole-dword image rows ((W C) % 4 == 0) runs here instead of on the byte-wise conv2d_generic.  The staging and the pixel
// walk are conv_mm_rt's (k_rt.hip), the weight image and the N slices are fc_rt's (k_fc_rt.hip).  What differs:
//
//   K       : k' = ky * KWCP + j with KWCP = KW C rounded up to 16: in NHWC the KW C bytes of one filter row are ONE contiguous
//             run of the staged image row, so lane group g of k step ks reads 16 consecutive bytes at (the pixel's window start)
//             + (ky ROW + j) from a [KS][4] table.  The bytes j >= KW C meet zero weights.  For C % 16 == 0 this is conv_mm_rt's
//             K; for other C the window start is not 16-byte aligned and the operand is built from aligned dword reads and
//             v_alignbyte (AL = 1) or from aligned dwords (AL = 4, C % 4 == 0): no misaligned ds_read_b128.
//   weights : the fc_rt image of the padded [N][KH KWCP] matrix; a slice of NTS 16-column tiles stays resident in LDS for the
//             whole launch and the grid is (NSL slices) x (walkers over the image steps); each slice re-reads the image tile.
//   image   : G whole images or one band of BH output rows per step, in tiles with an input-zero-point halo (SAME needs no
//             per-tap test); rows staged by LDS-DMA when W C % 16 == 0, else by dword loads.
//   WZ      : filter zero points: the sum of the window's real bytes is one more MFMA per k step against a tile of ones
//             (registers), the operand masked to the real taps by a [KS][4] table of 16-byte masks.
//   output  : each lane's 4 results of a 16-column tile: a dword store where N % 4 == 0, else one byte per real column.
//
// Epilogue: requant_pack4<MG, XR4> (k_common.hpp), modes 0 .. 2 as the host proved them for the operator's constants.
#include "k_common.hpp"

#include <algorithm>
#include <map>
#include <mutex>

namespace mf {
namespace k {

template <int AL, bool WZ, int MG, uint32_t XR4>
__global__ __launch_bounds__(256) void conv_gemm_rt(const int8_t *__restrict__ in, int8_t *__restrict__ out, ConvGemmArgs p, int batch) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = p.C, N = p.N, KS = p.KS, TB = p.TB, ROW = p.ROW, TILE = p.TILE, G = p.G, RB = p.RB;
    const int H = p.H, OH = p.OH, OW = p.OW, ROWB = p.W * C, BH = p.BH, NBANDS = p.NBANDS;
    const int slice = blockIdx.x % p.NSL, walker = blockIdx.x / p.NSL, nwalk = gridDim.x / p.NSL;
    const int nt0 = slice * p.NTS, nts = min(p.NTS, p.NT - nt0), nblk = (nts + TB - 1) / TB;
    uint8_t *T = lds + p.xoff;
    const uint32_t izp4 = p.izp4;

    // resident weights: the slice's tiles are one contiguous run of the image (whole 1 KiB pieces)
    const int8_t *wsrc = (const int8_t *)p.wimg + (size_t)nt0 * KS * 1024;
    for (int b = wave * 64; b < nts * KS * 64; b += 256) dma16(wsrc + (size_t)(b + lane) * 16, lds + b * 16);
    for (int i = tid; i < (G * TILE + 256) / 16; i += 256) ((uint4 *)T)[i] = make_uint4(izp4, izp4, izp4, izp4);
    for (int i = tid; i < KS * 4; i += 256) ((int *)(lds + p.toff))[i] = p.tap[i];
    if constexpr (WZ)
        for (int i = tid; i < KS * 16; i += 256) ((uint32_t *)(lds + p.moff))[i] = p.kmask[i];
    const int *tab = (const int *)(lds + p.toff);
    const int col = lane & 15, g = lane >> 4;
    const int nsteps = ((batch + G - 1) / G) * NBANDS;
    const v4i ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
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
                uint8_t *dst = T + gi * TILE + r * ROW + p.LP;
                if (y >= 0 && y < H) {
                    const int8_t *src = in + (img * H + y) * (long)ROWB;
                    if ((ROWB & 15) == 0) {
                        for (int o = 0; o < ROWB; o += 1024)
                            if (o + lane * 16 < ROWB) dma16(src + o + lane * 16, dst + o);
                    } else {
                        for (int o = lane * 4; o < ROWB; o += 256) *(uint32_t *)(dst + o) = *(const uint32_t *)(src + o);
                    }
                } else if (NBANDS > 1) {
                    for (int o = lane * 4; o < ROWB; o += 256) *(uint32_t *)(dst + o) = izp4;
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
// Geometry: the widest N slice (most tiles resident) that leaves room for a second workgroup per CU, else the widest that fits
// at all; the image step as conv_mm_rt's: G whole images (<= 48 KiB of tiles) or one band of output rows.
bool conv_gemm_plan(ConvGemmArgs &a, std::vector<int> &tap, std::vector<uint32_t> &mask, int H, int W, int C, int N, int KH, int KW, int sh,
                    int sw, int OH, int OW, bool pad_same, bool wz) {
    return conv_gemm_plan_pads(a, tap, mask, H, W, C, N, KH, KW, sh, sw, OH, OW, pad_same ? (KH - 1) / 2 : 0, pad_same ? (KW - 1) / 2 : 0, wz);
}
// ... with the window placement given (k_rt.hip conv_rows_plan_pads): the tile is sized from padt, padl, OH and OW
bool conv_gemm_plan_pads(ConvGemmArgs &a, std::vector<int> &tap, std::vector<uint32_t> &mask, int H, int W, int C, int N, int KH, int KW,
                         int sh, int sw, int OH, int OW, int padt, int padl, bool wz) {
    if (padt < 0 || padl < 0) return false;
    if (H < 1 || W < 1 || C < 1 || N < 1 || KH < 1 || KW < 1 || sh < 1 || sw < 1 || OH < 1 || OW < 1) return false;
    if ((W * C) % 4 != 0) return false;                  // whole-dword image rows
    const int KWC = KW * C, KWCP = (KWC + 15) & ~15, KS = (KH * KWCP + 63) / 64, NT = (N + 15) / 16;
    if (KS > CONV_GEMM_KS_MAX) return false;
    const int LP = (padl * C + 15) & ~15;
    // bytes read right of the image row: the last window's padded filter row (+ the 4 bytes of the aligned reads)
    const int over = std::max(0, ((OW - 1) * sw - padl) * C + KWCP + 4 - W * C);
    const int ROW = ((LP + W * C + over + 15) & ~15) + 16;
    const int tabb = KS * 16 + (wz ? KS * 64 : 0);
    auto rows_for = [&](int bh) { return (bh - 1) * sh + KH; };
    a.H = H, a.W = W, a.C = C, a.N = N, a.KH = KH, a.KW = KW, a.sh = sh, a.sw = sw, a.OH = OH, a.OW = OW;
    a.padl = padl, a.padt = padt, a.KWCP = KWCP, a.KS = KS, a.NT = NT, a.LP = LP, a.ROW = ROW;
    for (int pass = 0; pass < 2; ++pass) {
        const int lmax = pass == 0 ? 80 * 1024 : CONV_GEMM_LDS_MAX;
        for (int NTS = NT; NTS >= 1; --NTS) {
            const int NSL = (NT + NTS - 1) / NTS;
            if (NSL > 1 && (NT + NSL - 1) / NSL != NTS) continue; // (the same slicing as a wider NTS: balanced slices only)
            const int wbytes = NTS * KS * 1024;
            const int cap = std::min(lmax - wbytes - tabb - 256, 48 * 1024);
            // (the first pass also wants bands of at least 4 output rows: thinner bands leave waves without a 16-pixel chunk)
            if (cap < rows_for(pass == 0 ? std::min(OH, 4) : 1) * ROW) continue;
            if (rows_for(OH) * ROW <= cap) {
                a.NBANDS = 1, a.BH = OH, a.RB = rows_for(OH), a.TILE = a.RB * ROW;
                a.G = std::max(1, std::min(16, cap / a.TILE));
            } else {
                int bh = OH;
                while (bh > 1 && rows_for(bh) * ROW > cap) --bh;
                const int nb = (OH + bh - 1) / bh;
                bh = (OH + nb - 1) / nb;
                a.BH = bh, a.NBANDS = (OH + bh - 1) / bh, a.RB = rows_for(bh), a.TILE = a.RB * ROW, a.G = 1;
            }
            a.NTS = NTS, a.NSL = NSL, a.TB = std::min(4, NTS);
            a.xoff = wbytes, a.toff = a.xoff + a.G * a.TILE + 256, a.moff = a.toff + KS * 16;
            a.lds = a.toff + tabb;
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
        }
    }
    return false;
}

// the fc_rt image of [N][KH KWCP]: filter row ky's KW C bytes at k' = ky KWCP, zeros behind them
std::vector<int8_t> conv_gemm_weight_image(const int8_t *w /*[N][KH][KW][C]*/, const ConvGemmArgs &a) {
    const int KWC = a.KW * a.C, K = a.KH * a.KWCP;
    std::vector<int8_t> wp((size_t)a.N * K, 0);
    for (int n = 0; n < a.N; ++n)
        for (int ky = 0; ky < a.KH; ++ky)
            std::copy(w + ((size_t)n * a.KH + ky) * KWC, w + ((size_t)n * a.KH + ky + 1) * KWC, wp.begin() + (size_t)n * K + (size_t)ky * a.KWCP);
    return fc_rt_weight_image(wp.data(), K, a.N);
}

template <int AL, bool WZ, int MG, uint32_t XR4>
static void launch_conv_gemm_t(const int8_t *in, int8_t *out, const ConvGemmArgs &a, int batch, hipStream_t s) {
    int per_cu = 1;
    { // occupancy per (device, LDS bytes), asked once; the attribute is the whole budget, so no shape lowers it for another
        static std::mutex mu;
        static std::map<std::pair<int, int>, int> cache;
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> lock(mu);
        auto it = cache.find({dev, a.lds});
        if (it == cache.end()) {
            (void)hipFuncSetAttribute((const void *)conv_gemm_rt<AL, WZ, MG, XR4>, hipFuncAttributeMaxDynamicSharedMemorySize, CONV_GEMM_LDS_MAX);
            int n = 1;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, conv_gemm_rt<AL, WZ, MG, XR4>, 256, (size_t)a.lds) != hipSuccess || n < 1) {
                (void)hipGetLastError();
                n = 1;
            }
            it = cache.emplace(std::make_pair(dev, a.lds), n).first;
        }
        per_cu = it->second;
    }
    const long long nsteps = (long long)((batch + a.G - 1) / a.G) * a.NBANDS;
    long long walkers = std::max(1LL, 256LL * per_cu / a.NSL); // persistent: the resident slice is staged once per workgroup
    walkers = std::min(walkers, nsteps);
    MF_LAUNCH((conv_gemm_rt<AL, WZ, MG, XR4>), dim3((unsigned)(walkers * a.NSL)), dim3(256), a.lds, s, in, out, a, batch);
}
template <int AL, int MG, uint32_t XR4>
static void launch_conv_gemm_w(const int8_t *in, int8_t *out, const ConvGemmArgs &a, bool wz, int batch, hipStream_t s) {
    if (wz) launch_conv_gemm_t<AL, true, MG, XR4>(in, out, a, batch, s);
    else launch_conv_gemm_t<AL, false, MG, XR4>(in, out, a, batch, s);
}
void launch_conv_gemm(const int8_t *in, int8_t *out, const ConvGemmArgs &a, bool wz, int batch, hipStream_t s) {
    if (batch <= 0) return;
    if (a.C % 16 == 0) MF_DISPATCH4(a.magic, a.xr, launch_conv_gemm_w, (in, out, a, wz, batch, s), 16)
    else if (a.C % 4 == 0) MF_DISPATCH4(a.magic, a.xr, launch_conv_gemm_w, (in, out, a, wz, batch, s), 4)
    else MF_DISPATCH4(a.magic, a.xr, launch_conv_gemm_w, (in, out, a, wz, batch, s), 1)
}

} // namespace k
} // namespace mf
