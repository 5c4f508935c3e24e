// k_tconv.hip -- TRANSPOSE_CONV (TFLite builtin 67; the reference has none: include/microflow_amd.h states the contract) on the int8
// matrix pipe, split by output phase.
//
// Output (oy, ox) of a stride-(sh, sw) transposed convolution has the phase (py, px) = ((oy + padt) % sh, (ox + padl) % sw) and the
// base pixel (q, qx) = ((oy + padt) / sh, (ox + padl) / sw).  Its taps are ky = py + sh t, kx = px + sw u, and tap (t, u) reads input
// pixel (q - t, qx - u): per phase the operator is an ordinary stride-1 convolution with a sub-filter, and the sh sw phases together
// do exactly the operator's real multiply-adds (a zero-stuffed input through conv_2d does sh sw times as many).  tconv_phase_rt:
//
//   K       : per phase k' = t KWCP + j, KWCP = Tx C rounded up to 16: the Tx pixels qx - Tx + 1 .. qx a filter row reads are ONE
//             contiguous run of the staged NHWC row, so lane group g of k step ks reads 16 bytes at (the base pixel) + an entry of
//             the phase's [KS][4] table (conv_gemm_rt's K layout, k_conv_gemm.hip); the sub-filter is packed x-reversed, rows in
//             the order of t (wimage.cpp).  Phases differ in K': 3x3 at stride 2 has 4, 2, 2 and 1 taps.  A phase with no tap
//             (K < s) runs no matrix instruction and stores the requantised zero accumulator.
//   weights : one fc_rt image per phase, all phases of a slice of NTS 16-column tiles resident in LDS for the whole launch; the grid
//             is (NSL slices) x (walkers over the image steps), slice-major within a walker.
//   image   : G whole images or one band of BH base rows per step, inside an input-zero-point halo: TYM - 1 rows above, TXM - 1
//             pixels left, and the rows / pixels bases beyond H - 1 / W - 1 reach (padding smaller than the filter's overhang), so no
//             tap is tested per pixel.  Rows by LDS-DMA when W C % 16 == 0, else by dword loads.
//   work    : a wave takes chunks of 16 consecutive base pixels of the step (row-major, so a chunk may span base rows where NBX < 16)
//             and walks the phases of those bases, px fastest: the sw pieces of an output line are stored back to back.
//   output  : each lane's 4 consecutive n of one output pixel: a dword store where N % 4 == 0, else one byte per real column;
//             pixels outside OH x OW (bases the padding cuts, the last base row / column of VALID and odd sizes) are masked.
//
// Epilogue: requant_pack4<MG, XR4> (k_common.hpp), the mode proved on the host from the whole-filter accumulator bound.
// tconv_generic is the contract in plain C++, one thread per output byte, for everything outside the fast kernel's class.
#include "k_common.hpp"
#include "wimage.hpp"

#include <algorithm>
#include <map>
#include <mutex>

namespace mf {
namespace k {

template <int AL, int MG, uint32_t XR4>
__global__ __launch_bounds__(256) void tconv_phase_rt(const int8_t *__restrict__ in, int8_t *__restrict__ out, TconvArgs p, int batch) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = p.C, N = p.N, TB = p.TB, ROW = p.ROW, TILE = p.TILE, G = p.G, RB = p.RB;
    const int H = p.H, OH = p.OH, OW = p.OW, ROWB = p.W * C, BH = p.BH, NBANDS = p.NBANDS, NBX = p.NBX, NT16 = p.NT * 16;
    const int slice = blockIdx.x % p.NSL, walker = blockIdx.x / p.NSL, nwalk = gridDim.x / p.NSL;
    const int nt0 = slice * p.NTS, nts = min(p.NTS, p.NT - nt0), nblk = (nts + TB - 1) / TB;
    uint8_t *T = lds + p.xoff;
    const uint32_t izp4 = p.izp4;

    // resident weights: the slice's tiles of every phase are one contiguous run of the image (whole 1 KiB pieces)
    const int8_t *wsrc = (const int8_t *)p.wimg + (size_t)nt0 * p.KSUM * 1024;
    for (int b = wave * 64; b < nts * p.KSUM * 64; b += 256) dma16(wsrc + (size_t)(b + lane) * 16, lds + b * 16);
    for (int i = tid; i < (G * TILE + 256) / 16; i += 256) ((uint4 *)T)[i] = make_uint4(izp4, izp4, izp4, izp4);
    for (int i = tid; i < 32 + p.KSUM * 4; i += 256) ((int *)(lds + p.toff))[i] = p.tab[i];
    const int *rec = (const int *)(lds + p.toff), *tab0 = rec + 32;
    const int col = lane & 15, g = lane >> 4;
    const int nsteps = ((batch + G - 1) / G) * NBANDS;
    wg_sync();
    for (int step = walker; step < nsteps; step += nwalk) {
        const int band = step % NBANDS, ist = step / NBANDS;
        const int yfirst = band * BH - (p.TYM - 1);      // input row held by tile row 0
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
        const int bp = BH * NBX, npix = gvalid * bp;     // (base rows past the image are masked below)
        for (int chunk = wave; chunk * 16 < npix; chunk += 4) {
            const int pp = chunk * 16 + col;
            const int pc = pp < npix ? pp : npix - 1;
            const int gi = pc / bp, rr = pc - gi * bp;
            const int bl = rr / NBX, bx = rr - bl * NBX, by = band * BH + bl;
            const bool live = pp < npix && by < p.NBY;
            const int wbase = p.xoff + gi * TILE + (bl + p.TYM - 1) * ROW + p.LP + bx * C; // the base pixel's LDS byte
            for (int ph = 0; ph < p.NPH; ++ph) {
                const int py = ph / p.sw, px = ph - py * p.sw;
                const int oy = by * p.sh + py - p.padt, ox = bx * p.sw + px - p.padl;
                const bool ok = live && oy >= 0 && oy < OH && ox >= 0 && ox < OW;
                if (__builtin_amdgcn_ballot_w64(ok) == 0) continue; // (none of the 16 bases has this phase inside the output)
                const int KS = __builtin_amdgcn_readfirstlane(rec[2 * ph]), kpre = __builtin_amdgcn_readfirstlane(rec[2 * ph + 1]);
                const int *tab = tab0 + kpre * 4;
                const uint8_t *wph = lds + (size_t)nts * kpre * 1024; // the phase's tiles of this slice
                // operand B of k step ks: the 16 bytes at (base pixel) + (table offset)
                auto operand = [&](int ks) -> v4i {
                    const int off = wbase + tab[ks * 4 + g];
                    if constexpr (AL == 16) {
                        return *(const v4i *)(lds + off);
                    } else {
                        const uint32_t *q = (const uint32_t *)(lds + off);
                        return v4i{(int)q[0], (int)q[1], (int)q[2], (int)q[3]};
                    }
                };
                const size_t opix = ok ? ((size_t)(ist * G + gi) * OH + oy) * OW + ox : 0;
                for (int blk = 0; blk < nblk; ++blk) {
                    const int lt0 = blk * TB, tb = min(TB, nts - lt0);
                    v4i acc[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (i < tb) {
                            const int4 kc = magic4<MG>(*(const int4 *)(p.Kc + ph * NT16 + (nt0 + lt0 + i) * 16 + g * 4));
                            acc[i] = v4i{kc.x, kc.y, kc.z, kc.w};
                        }
                    }
                    for (int ks = 0; ks < KS; ++ks) {
                        const v4i b = operand(ks);
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (i < tb) acc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(*(const v4i *)(wph + (((lt0 + i) * KS + ks) * 64 + lane) * 16), b, acc[i], 0, 0, 0);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int ch = (nt0 + lt0 + i) * 16 + g * 4; // the lane's 4 output channels
                        if (i < tb && ch < N) {
                            const v4i a = acc[i];
                            const uint32_t d = requant_pack4<MG, XR4>(a[0], a[1], a[2], a[3], *(const float4 *)(p.A + ch), *(const float4 *)(p.S + ch),
                                                                      p.lo_f, p.hi_f);
                            if (ok) {
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
}

// The contract, value by value: every (ky, kx) whose input pixel exists and lies inside the image
__global__ __launch_bounds__(256) void tconv_generic(const int8_t *__restrict__ in, int8_t *__restrict__ out, ConvArgs p, int padt, int padl,
                                                     size_t total) {
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int n = (int)(idx % p.N);
        size_t t = idx / p.N;
        const int ox = (int)(t % p.OW);
        t /= p.OW;
        const int oy = (int)(t % p.OH);
        const size_t img = t / p.OH;
        const int8_t *ip = in + img * (size_t)p.H * p.W * p.C;
        const int8_t *wp = p.w + (size_t)n * p.KH * p.KW * p.C;
        const int wz = p.wzp[n];
        int acc = 0;
        for (int ky = 0; ky < p.KH; ++ky) {
            const int ty = oy + padt - ky;
            if (ty < 0 || ty % p.sh != 0 || ty / p.sh >= p.H) continue;
            for (int kx = 0; kx < p.KW; ++kx) {
                const int tx = ox + padl - kx;
                if (tx < 0 || tx % p.sw != 0 || tx / p.sw >= p.W) continue;
                const int8_t *vp = ip + ((size_t)(ty / p.sh) * p.W + tx / p.sw) * p.C;
                const int8_t *fp = wp + ((size_t)ky * p.KW + kx) * p.C;
                for (int c = 0; c < p.C; ++c) acc += ((int)vp[c] - p.izp) * ((int)fp[c] - wz);
            }
        }
        out[idx] = (int8_t)(requant_any(acc, p.A[n], p.S[n], p.lo_f, p.hi_f) ^ p.xr);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
// Geometry as conv_gemm_plan's: the widest N slice that leaves room for a second workgroup per CU, else the widest that fits at all;
// the image step G whole images (<= 48 KiB of tiles) or one band of base rows.
bool tconv_plan(TconvArgs &a, int H, int W, int C, int N, int KH, int KW, int sh, int sw, int OH, int OW, int padt, int padl) {
    if (H < 1 || W < 1 || C < 1 || N < 1 || KH < 1 || KW < 1 || OH < 1 || OW < 1 || padt < 0 || padl < 0) return false;
    if (sh < 1 || sh > 4 || sw < 1 || sw > 4 || KH > 8 || KW > 8 || C % 4 != 0 || ((long long)W * C) % 4 != 0) return false;
    if ((long long)W * C > (1 << 20) || (long long)OW * sw > (1 << 20) || (long long)OH * sh > (1 << 20)) return false;
    int KSUM = 0;
    for (const wimage::TconvPhase &p : wimage::tconv_phases(KH, KW, C, sh, sw)) {
        if (p.KS > CONV_GEMM_KS_MAX) return false;
        KSUM += p.KS;
    }
    const wimage::TconvTile t = wimage::tconv_tile(W, C, KH, KW, sh, sw, OH, OW, padt, padl);
    if (t.ROW > 48 * 1024) return false;
    const int NT = (N + 15) / 16, TYM = t.TYM, TXM = t.TXM, NBY = t.NBY, NBX = t.NBX, LP = t.LP, ROW = (int)t.ROW, tabb = (32 + KSUM * 4) * 4;
    auto rows_for = [&](int bh) { return bh + TYM - 1; };
    a.H = H, a.W = W, a.C = C, a.N = N, a.KH = KH, a.KW = KW, a.sh = sh, a.sw = sw, a.OH = OH, a.OW = OW, a.padt = padt, a.padl = padl;
    a.NBY = NBY, a.NBX = NBX, a.TYM = TYM, a.TXM = TXM, a.NPH = sh * sw, a.KSUM = KSUM, a.NT = NT, a.LP = LP, a.ROW = ROW;
    for (int pass = 0; pass < 2; ++pass) {
        const int lmax = pass == 0 ? 80 * 1024 : CONV_GEMM_LDS_MAX;
        for (int NTS = NT; NTS >= 1; --NTS) {
            const int NSL = (NT + NTS - 1) / NTS;
            if (NSL > 1 && (NT + NSL - 1) / NSL != NTS) continue; // (the same slicing as a wider NTS: balanced slices only)
            const long long wbytes = (long long)NTS * KSUM * 1024;
            const long long cap = std::min<long long>(lmax - wbytes - tabb - 256, 48 * 1024);
            // (the first pass also wants bands of at least 4 base rows: thinner bands leave waves without a 16-pixel chunk)
            if (cap < (long long)rows_for(pass == 0 ? std::min(NBY, 4) : 1) * ROW) continue;
            if ((long long)rows_for(NBY) * ROW <= cap) {
                a.NBANDS = 1, a.BH = NBY, a.RB = rows_for(NBY), a.TILE = a.RB * ROW;
                a.G = (int)std::max<long long>(1, std::min<long long>(16, cap / a.TILE));
            } else {
                int bh = NBY;
                while (bh > 1 && (long long)rows_for(bh) * ROW > cap) --bh;
                const int nb = (NBY + bh - 1) / bh;
                bh = (NBY + nb - 1) / nb;
                a.BH = bh, a.NBANDS = (NBY + bh - 1) / bh, a.RB = rows_for(bh), a.TILE = a.RB * ROW, a.G = 1;
            }
            a.NTS = NTS, a.NSL = NSL, a.TB = std::min(4, NTS);
            a.xoff = (int)wbytes, a.toff = a.xoff + a.G * a.TILE + 256, a.lds = a.toff + tabb;
            return true;
        }
    }
    return false;
}

template <int AL, int MG, uint32_t XR4>
static void launch_tconv_phase_t(const int8_t *in, int8_t *out, const TconvArgs &a, int batch, hipStream_t s) {
    int per_cu = 1;
    { // occupancy per (device, LDS bytes), asked once; the attribute is the whole budget, so no shape lowers it for another
        static std::mutex mu;
        static std::map<std::pair<int, int>, int> cache;
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> lock(mu);
        auto it = cache.find({dev, a.lds});
        if (it == cache.end()) {
            (void)hipFuncSetAttribute((const void *)tconv_phase_rt<AL, MG, XR4>, hipFuncAttributeMaxDynamicSharedMemorySize, CONV_GEMM_LDS_MAX);
            int n = 1;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, tconv_phase_rt<AL, MG, XR4>, 256, (size_t)a.lds) != hipSuccess || n < 1) {
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
    MF_LAUNCH((tconv_phase_rt<AL, MG, XR4>), dim3((unsigned)(walkers * a.NSL)), dim3(256), a.lds, s, in, out, a, batch);
}
void launch_tconv_phase(const int8_t *in, int8_t *out, const TconvArgs &a, int batch, hipStream_t s) {
    if (batch <= 0) return;
    if (a.C % 16 == 0) MF_DISPATCH4(a.magic, a.xr, launch_tconv_phase_t, (in, out, a, batch, s), 16)
    else MF_DISPATCH4(a.magic, a.xr, launch_tconv_phase_t, (in, out, a, batch, s), 4)
}
void launch_tconv_generic(const int8_t *in, int8_t *out, const ConvArgs &a, int padt, int padl, size_t batch, hipStream_t s) {
    const size_t total = batch * a.OH * a.OW * a.N;
    MF_LAUNCH(tconv_generic, dim3(grid_for(total)), dim3(256), 0, s, in, out, a, padt, padl, total);
}

} // namespace k
} // namespace mf
