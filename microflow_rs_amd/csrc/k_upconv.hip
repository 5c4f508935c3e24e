// k_upconv.hip -- RESIZE_NEAREST_NEIGHBOR by integer factors (sy, sx) + the stride-1 Conv2D on its result, as ONE product on the int8
// matrix pipe (include/microflow_amd.h: mf_conv_2d_upsampled_create; Keras' UpSampling2D + Conv2D).  The upsampled tensor is never
// written: not to HBM, and in y not to LDS either.
//
// The product is conv_gemm_rt's (k_conv_gemm.hip): K' = [ky][KW C rounded up to 16], the fc_rt weight image with a slice of 16-column
// tiles resident in LDS for the launch, grid = slices x walkers, chunks of 16 consecutive output pixels of the step per wave, the weight
// tile of a (tile, k step) read once per chunk.  What is its own is how the image reaches operand B:
//
//   tile    : a step stages the SOURCE rows its output rows reach -- floor((oy - padt + ky) / sy) over the band -- each written with
//             every pixel repeated sx times behind an input-zero-point halo of padl pixels, conv_gemm_rt's right halo behind it.  A staged
//             row therefore IS a row of the upsampled image and the KW C bytes of a filter row are one contiguous run of it; the tile has
//             about 1 / sy of the rows the upsampled tile would, and HBM is read once per source byte: global loads into registers (16
//             bytes where C % 16 == 0, dwords otherwise), sx LDS writes per loaded unit.  Source rows outside [0, H) are zero-point rows.
//   operand : output row oy = sy q + py reads, for filter row ky, source row q + d with d = floor((py + ky - padt) / sy).  The host
//             builds sy tables [py][KS][4] of (d - dmin) ROW + j (tile row 0 of a band holds source row q0 + dmin); lane group g of k
//             step ks reads 16 bytes at (tile row of q, column ox) + entry.  A chunk that spans output rows carries its phase PER LANE: each
//             lane indexes the table row of its own py (the tables sit in LDS; the read costs what conv_gemm_rt's does).
//   bands   : start on multiples of sy output rows, so a band's source rows are whole.
//
// Filter zero points all zero (the host routes the others to upconv_generic below).  Epilogue: requant_pack4<MG, XR4>, modes 0 .. 2.
#include "k_common.hpp"
#include "wimage.hpp"

#include <algorithm>
#include <map>
#include <mutex>

namespace mf {
namespace k {

template <int AL, int MG, uint32_t XR4>
__global__ __launch_bounds__(256) void upconv_rt(const int8_t *__restrict__ in, int8_t *__restrict__ out, UpconvArgs u, int batch) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const ConvGemmArgs &p = u.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = p.C, N = p.N, KS = p.KS, TB = p.TB, ROW = p.ROW, TILE = p.TILE, G = p.G, RB = p.RB;
    const int H = p.H, OH = p.OH, OW = p.OW, ROWB = p.W * C, BH = p.BH, NBANDS = p.NBANDS, sy = u.sy, sx = u.sx;
    const int slice = blockIdx.x % p.NSL, walker = blockIdx.x / p.NSL, nwalk = gridDim.x / p.NSL;
    const int nt0 = slice * p.NTS, nts = min(p.NTS, p.NT - nt0), nblk = (nts + TB - 1) / TB;
    uint8_t *T = lds + p.xoff;
    const uint32_t izp4 = p.izp4;
    constexpr int U = AL == 16 ? 16 : 4; // bytes per staged unit

    // resident weights: the slice's tiles are one contiguous run of the image (whole 1 KiB pieces)
    const int8_t *wsrc = (const int8_t *)p.wimg + (size_t)nt0 * KS * 1024;
    for (int b = wave * 64; b < nts * KS * 64; b += 256) dma16(wsrc + (size_t)(b + lane) * 16, lds + b * 16);
    for (int i = tid; i < (G * TILE + 256) / 16; i += 256) ((uint4 *)T)[i] = make_uint4(izp4, izp4, izp4, izp4);
    for (int i = tid; i < sy * KS * 4; i += 256) ((int *)(lds + p.toff))[i] = p.tap[i];
    const int *tab = (const int *)(lds + p.toff);
    const int col = lane & 15, g = lane >> 4;
    const int nsteps = ((batch + G - 1) / G) * NBANDS;
    wg_sync();
    for (int step = walker; step < nsteps; step += nwalk) {
        const int band = step % NBANDS, ist = step / NBANDS;
        const int yfirst = (band * BH) / sy + u.dmin;   // source row held by tile row 0 (BH % sy == 0 where there are bands)
        const int gvalid = min(G, batch - ist * G);
        wg_sync();                                       // the previous step's reads of the tile are done
        for (int item = wave; item < gvalid * RB; item += 4) {
            const int gi = item / RB, r = item - gi * RB, y = yfirst + r;
            uint8_t *dst = T + gi * TILE + r * ROW + p.LP;
            if (y >= 0 && y < H) {
                const int8_t *src = in + (((long)ist * G + gi) * H + y) * (long)ROWB;
                for (int o = lane * U; o < ROWB; o += 64 * U) {
                    const int x = o / C, c = o - x * C;
                    uint8_t *d = dst + x * sx * C + c;
                    if constexpr (AL == 16) {
                        const uint4 v = *(const uint4 *)(src + o);
                        for (int rx = 0; rx < sx; ++rx) *(uint4 *)(d + rx * C) = v;
                    } else {
                        const uint32_t v = *(const uint32_t *)(src + o);
                        for (int rx = 0; rx < sx; ++rx) *(uint32_t *)(d + rx * C) = v;
                    }
                }
            } else if (NBANDS > 1) { // (with whole images per step the rows outside the image keep the first fill)
                for (int o = lane * 4; o < ROWB * sx; o += 256) *(uint32_t *)(dst + o) = izp4;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // (the first time: the weights' DMAs have landed)
        wg_sync();
        const int rows_here = min(BH, OH - band * BH);
        const int bp = BH * OW, npix = gvalid * bp;      // (rows past the image are masked below)
        for (int chunk = wave; chunk * 16 < npix; chunk += 4) {
            const int pp = chunk * 16 + col;
            const int pc = pp < npix ? pp : npix - 1;
            const int gi = pc / bp, rr = pc - gi * bp;
            const int oyl = rr / OW, ox = rr - oyl * OW;
            const int ql = oyl / sy, py = oyl - ql * sy;
            const bool live = pp < npix && oyl < rows_here;
            const int wbase = p.xoff + gi * TILE + ql * ROW + p.LP + (ox - p.padl) * C; // the window's column in source row q's tile row
            const int *tp = tab + py * KS * 4 + g;                                      // this lane's phase table
            auto operand = [&](int ks) -> v4i {
                const int off = wbase + tp[ks * 4];
                if constexpr (AL == 16) {
                    return *(const v4i *)(lds + off);
                } else {
                    const uint32_t *q = (const uint32_t *)(lds + off);
                    return v4i{(int)q[0], (int)q[1], (int)q[2], (int)q[3]};
                }
            };
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
                        const v4i a = acc[i];
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

// The contract in plain C++: conv2d_generic (k_generic.hip) on the image in[iy / sy][ix / sx], one thread per output byte, any shape
// and strides, filter zero points included.  p.H, p.W: the source image's.
__global__ __launch_bounds__(256) void upconv_generic(const int8_t *__restrict__ in, int8_t *__restrict__ out, ConvArgs p, int sy, int sx, size_t total) {
    const int UH = p.H * sy, UW = p.W * sx;
    const int shy = p.pad_same ? (p.KH - 1) / 2 : 0, shx = p.pad_same ? (p.KW - 1) / 2 : 0;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int n = (int)(idx % p.N);
        size_t t = idx / p.N;
        const int ox = (int)(t % p.OW);
        t /= p.OW;
        const int oy = (int)(t % p.OH);
        const size_t img = t / p.OH;
        const int8_t *ip = in + img * (size_t)p.H * p.W * p.C;
        const int8_t *wp = p.w + (size_t)n * p.KH * p.KW * p.C;
        int dot = 0, vs = 0;
        for (int ky = 0; ky < p.KH; ++ky) {
            const int iy = oy * p.sh + ky - shy;
            for (int kx = 0; kx < p.KW; ++kx) {
                const int ix = ox * p.sw + kx - shx;
                const bool ok = iy >= 0 && iy < UH && ix >= 0 && ix < UW;
                const int8_t *vp = ok ? ip + ((size_t)(iy / sy) * p.W + ix / sx) * p.C : ip;
                const int8_t *fp = wp + ((size_t)ky * p.KW + kx) * p.C;
                for (int c = 0; c < p.C; ++c) {
                    const int v = ok ? (int)vp[c] : p.izp;
                    dot += v * (int)fp[c];
                    vs += v;
                }
            }
        }
        const int acc = dot - p.wzp[n] * vs + p.Kc[n];
        out[idx] = (int8_t)(requant_any(acc, p.A[n], p.S[n], p.lo_f, p.hi_f) ^ p.xr);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
// conv_gemm_plan's budgets: the widest N slice that leaves room for a second workgroup per CU (<= 80 KiB), else the widest that fits at
// all; G whole images (<= 48 KiB of tiles) or one band of output rows, a multiple of sy, per step.
bool upconv_plan(UpconvArgs &u, std::vector<int> &tap, int H, int W, int C, int N, int KH, int KW, int sy, int sx, int OH, int OW, int padt,
                 int padl) {
    if (H < 1 || W < 1 || C < 1 || N < 1 || KH < 1 || KW < 1 || OH < 1 || OW < 1 || padt < 0 || padl < 0) return false;
    if (C % 4 != 0 || sy < 1 || sx < 1 || sy > 4 || sx > 4 || (sy == 1 && sx == 1) || KH > 7 || KW > 7 || padt >= KH || padl >= KW) return false;
    const int UH = H * sy, UW = W * sx;
    if (OH - 1 - padt + KH - 1 >= UH + KH || OW - 1 - padl + KW - 1 >= UW + KW) return false; // (windows far outside the image: not a convolution's geometry)
    ConvGemmArgs &a = u.g;
    const int KWC = KW * C, KWCP = (KWC + 15) & ~15, KS = (KH * KWCP + 63) / 64, NT = (N + 15) / 16;
    if (KS > CONV_GEMM_KS_MAX) return false;
    const int LP = (padl * C + 15) & ~15;
    const int over = std::max(0, (OW - 1 - padl) * C + KWCP + 4 - UW * C);
    const int ROW = ((LP + UW * C + over + 15) & ~15) + 16;
    const int tabb = sy * KS * 16;
    const int dmin = wimage::upconv_dmin(padt, sy);
    auto rows_for = [&](int bh) { return (bh - 1 + KH - 1 - padt) / sy - dmin + 1; }; // source rows a band of bh output rows reaches
    auto up = [&](int v) { return (v + sy - 1) / sy * sy; };
    a.H = H, a.W = W, a.C = C, a.N = N, a.KH = KH, a.KW = KW, a.sh = 1, a.sw = 1, a.OH = OH, a.OW = OW;
    a.padl = padl, a.padt = padt, a.KWCP = KWCP, a.KS = KS, a.NT = NT, a.LP = LP, a.ROW = ROW;
    u.sy = sy, u.sx = sx, u.dmin = dmin;
    for (int pass = 0; pass < 2; ++pass) {
        const int lmax = pass == 0 ? 80 * 1024 : CONV_GEMM_LDS_MAX;
        for (int NTS = NT; NTS >= 1; --NTS) {
            const int NSL = (NT + NTS - 1) / NTS;
            if (NSL > 1 && (NT + NSL - 1) / NSL != NTS) continue; // (balanced slices only)
            const int wbytes = NTS * KS * 1024;
            const int cap = std::min(lmax - wbytes - tabb - 256, 48 * 1024);
            if (cap < rows_for(std::min(OH, pass == 0 ? up(4) : sy)) * ROW) continue;
            if (rows_for(OH) * ROW <= cap) {
                a.NBANDS = 1, a.BH = OH, a.RB = rows_for(OH), a.TILE = a.RB * ROW;
                a.G = std::max(1, std::min(16, cap / a.TILE));
            } else {
                int bh = sy;
                while (bh + sy < OH && rows_for(bh + sy) * ROW <= cap) bh += sy;
                const int nb = (OH + bh - 1) / bh;
                bh = up((OH + nb - 1) / nb);
                a.BH = bh, a.NBANDS = (OH + bh - 1) / bh, a.RB = rows_for(bh), a.TILE = a.RB * ROW, a.G = 1;
            }
            a.NTS = NTS, a.NSL = NSL, a.TB = std::min(4, NTS);
            a.xoff = wbytes, a.toff = a.xoff + a.G * a.TILE + 256, a.moff = a.toff + tabb;
            a.lds = a.toff + tabb;
            tap = wimage::upconv_tables(KH, KW, C, sy, padt, ROW);
            return true;
        }
    }
    return false;
}

template <int AL, int MG, uint32_t XR4> static void launch_upconv_t(const int8_t *in, int8_t *out, const UpconvArgs &a, int batch, hipStream_t s) {
    int per_cu = 1;
    { // occupancy per (device, LDS bytes), asked once
        static std::mutex mu;
        static std::map<std::pair<int, int>, int> cache;
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> lock(mu);
        auto it = cache.find({dev, a.g.lds});
        if (it == cache.end()) {
            (void)hipFuncSetAttribute((const void *)upconv_rt<AL, MG, XR4>, hipFuncAttributeMaxDynamicSharedMemorySize, CONV_GEMM_LDS_MAX);
            int n = 1;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, upconv_rt<AL, MG, XR4>, 256, (size_t)a.g.lds) != hipSuccess || n < 1) {
                (void)hipGetLastError();
                n = 1;
            }
            it = cache.emplace(std::make_pair(dev, a.g.lds), n).first;
        }
        per_cu = it->second;
    }
    // persistent: the resident slice is staged once per workgroup.  The plan's G is the most images a step's tiles hold; where the batch
    // leaves the grid fewer than two steps per workgroup the device keeps resident, fewer images per step (the same LDS plan, fewer
    // tiles used) make more, shorter steps, so that a moderate batch still fills the device
    UpconvArgs b = a;
    const long long resident = std::max(1LL, 256LL * per_cu / a.g.NSL);
    while (b.g.G > 1 && (long long)((batch + b.g.G - 1) / b.g.G) * b.g.NBANDS < 2 * resident) b.g.G = (b.g.G + 1) / 2;
    const long long nsteps = (long long)((batch + b.g.G - 1) / b.g.G) * b.g.NBANDS;
    const long long walkers = std::min(resident, nsteps);
    MF_LAUNCH((upconv_rt<AL, MG, XR4>), dim3((unsigned)(walkers * b.g.NSL)), dim3(256), b.g.lds, s, in, out, b, batch);
}
void launch_upconv(const int8_t *in, int8_t *out, const UpconvArgs &a, int batch, hipStream_t s) {
    if (batch <= 0) return;
    if (a.g.C % 16 == 0) MF_DISPATCH4(a.g.magic, a.g.xr, launch_upconv_t, (in, out, a, batch, s), 16)
    else MF_DISPATCH4(a.g.magic, a.g.xr, launch_upconv_t, (in, out, a, batch, s), 4)
}

void launch_upconv_generic(const int8_t *in, int8_t *out, const ConvArgs &a, int sy, int sx, size_t batch, hipStream_t s) {
    const size_t total = batch * (size_t)a.OH * a.OW * a.N;
    MF_LAUNCH(upconv_generic, dim3(grid_for(total)), dim3(256), 0, s, in, out, a, sy, sx, total);
}

} // namespace k
} // namespace mf
