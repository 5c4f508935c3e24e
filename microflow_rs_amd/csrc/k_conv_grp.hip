// k_conv_grp.hip -- GROUPED Conv2D on the int8 matrix pipe (include/microflow_amd.h: mf_conv_2d_grouped_create; the reference never has
// filter.C != input.C).  Filters [N][KH][KW][Cg] with Cg = C / groups, Ng = N / groups; output channel n belongs to group n / Ng and
// reads input channels [g Cg, (g + 1) Cg) only.
//
// conv_gemm_rt (k_conv_gemm.hip) cannot serve this: its K axis is the contiguous KW C run of a staged image row, and it amortises one
// image operand over TB weight tiles of the same pixels.  Here the tiles of different groups share no operand, and the bytes one output
// column needs are Cg bytes at kx C + g Cg of each tap, not contiguous across taps.  Only the staging is conv_gemm_rt's (G whole images
// or one row band per step, the input-zero-point halo, LDS-DMA rows when W C % 16 == 0, wg_sync for every barrier).  The product:
//
//   tiles   : a 16-column tile never mixes operands.  Ng >= 16: a tile is part of ONE group (TPG = ceil(Ng / 16) tiles per group, the
//             columns past Ng dead and not stored).  Ng < 16: a tile packs GPT = min(groups, 16 / Ng) whole groups; its weights are
//             block-diagonal inside the tile's span of SPAN = GPT Cg channels and zero elsewhere.  colch[] maps tile columns to output
//             channels (-1: dead); the constants (A, S, Kc, wzp) are laid out per tile column.
//   K       : per tile, k = (ky KW + kx) SPAN + c over the tile's channel span -- not the image row.  A [KS][4][4] table holds, for every
//             k dword, its byte offset from (the pixel's window start + the tile's channel base).  SPAN % 16 == 0 and C % 16 == 0
//             (AL = 16): the four dwords of a lane group are 16 consecutive channels of one tap, one ds_read_b128 at the first offset.
//             Otherwise (AL = 4; Cg % 4 == 0, C % 4 == 0): four dword reads, each four channels of one tap, so Cg = 4 and Cg = 8 waste
//             nothing but the padding of K to 64.  k dwords past KH KW SPAN read offset 0 against zero weights.
//   reuse   : the WEIGHT operand is amortised, not the image operand: a wave takes one tile and PB = 4 chunks of 16 pixels, reads each
//             weight k step once and uses it for the four chunks (conv_gemm_rt: one image operand for four tiles; the same LDS reads per
//             MFMA).  Tiles of one group do not share image reads here.
//   weights : PW 1 KiB pieces per tile, resident in LDS for the whole launch in N slices of NTS tiles (grid = slices x walkers).
//   WZ      : filter zero points: the window sum is per GROUP, not per pixel -- columns of a packed tile need different sums.  Behind a
//             tile's KS weight pieces the image holds KS pieces of ones over the real k bytes of each column's own group; one more MFMA
//             per k step and chunk against them yields each column's sum in the accumulator's own layout (no operand masking).
//   output  : a dword store where a lane's four columns are four consecutive real channels at a dword boundary, else bytes.
//
// Epilogue: requant_pack4<MG, XR4> (k_common.hpp), modes 0 .. 2 as the host proved them for the operator's constants.
#include "k_common.hpp"

#include <algorithm>
#include <map>
#include <mutex>

namespace mf {
namespace k {

template <int AL, bool WZ, int MG, uint32_t XR4>
__global__ __launch_bounds__(256) void conv_grp_rt(const int8_t *__restrict__ in, int8_t *__restrict__ out, ConvGrpArgs q, int batch) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    constexpr int PB = 4;                                // 16-pixel chunks per weight read
    const ConvGemmArgs &p = q.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = p.C, N = p.N, KS = p.KS, ROW = p.ROW, TILE = p.TILE, G = p.G, RB = p.RB, PW = q.PW;
    const int H = p.H, OH = p.OH, OW = p.OW, ROWB = p.W * C, BH = p.BH, NBANDS = p.NBANDS;
    const int slice = blockIdx.x % p.NSL, walker = blockIdx.x / p.NSL, nwalk = gridDim.x / p.NSL;
    const int nt0 = slice * p.NTS, nts = min(p.NTS, p.NT - nt0);
    uint8_t *T = lds + p.xoff;
    const uint32_t izp4 = p.izp4;

    // resident weights: the slice's tiles are one contiguous run of the image (whole 1 KiB pieces)
    const int8_t *wsrc = (const int8_t *)p.wimg + (size_t)nt0 * PW * 1024;
    for (int b = wave * 64; b < nts * PW * 64; b += 256) dma16(wsrc + (size_t)(b + lane) * 16, lds + b * 16);
    for (int i = tid; i < (G * TILE + 256) / 16; i += 256) ((uint4 *)T)[i] = make_uint4(izp4, izp4, izp4, izp4);
    for (int i = tid; i < KS * 16; i += 256) ((int *)(lds + p.toff))[i] = p.tap[i];
    const int *tab = (const int *)(lds + p.toff);
    const int col = lane & 15, g = lane >> 4;
    const int nsteps = ((batch + G - 1) / G) * NBANDS;
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
        const int nch = (npix + 15) / 16, ncg = (nch + PB - 1) / PB;
        for (int item = wave; item < nts * ncg; item += 4) {
            const int lt = item % nts, cg = item / nts;  // one tile, PB pixel chunks
            const int t = nt0 + lt;
            const int tbase = q.GPT ? t * q.SPAN : (t / q.TPG) * q.Cg; // the tile's first input channel
            const int nb = min(PB, nch - cg * PB);
            int wb[PB];
            bool live[PB];
            size_t opix[PB];
#pragma unroll
            for (int i = 0; i < PB; ++i) {
                const int pp = (cg * PB + i) * 16 + col;
                const int pc = pp < npix ? pp : npix - 1;
                const int gi = pc / bp, rr = pc - gi * bp;
                const int oyl = rr / OW, ox = rr - oyl * OW;
                live[i] = pp < npix && oyl < rows_here;
                wb[i] = p.xoff + gi * TILE + (oyl * p.sh) * ROW + p.LP + (ox * p.sw - p.padl) * C + tbase; // the window's LDS byte, at the tile's span
                opix[i] = ((size_t)(ist * G + gi) * OH + band * BH + oyl) * OW + ox;
            }
            // operand B of k step ks for a window: the 16 bytes lane group g supplies, by the table
            auto operand = [&](int w0, int ks) -> v4i {
                if constexpr (AL == 16) {
                    return *(const v4i *)(lds + w0 + tab[(ks * 4 + g) * 4]);
                } else {
                    const int4 o = *(const int4 *)(tab + (ks * 4 + g) * 4);
                    return v4i{(int)*(const uint32_t *)(lds + w0 + o.x), (int)*(const uint32_t *)(lds + w0 + o.y),
                               (int)*(const uint32_t *)(lds + w0 + o.z), (int)*(const uint32_t *)(lds + w0 + o.w)};
                }
            };
            const int c4 = t * 16 + g * 4;               // the lane's 4 tile columns
            v4i acc[PB], rs[PB];
            {
                const int4 kc = magic4<MG>(*(const int4 *)(p.Kc + c4));
#pragma unroll
                for (int i = 0; i < PB; ++i) acc[i] = v4i{kc.x, kc.y, kc.z, kc.w}, rs[i] = v4i{0, 0, 0, 0};
            }
            const uint8_t *wt = lds + (size_t)lt * PW * 1024 + lane * 16;
            for (int ks = 0; ks < KS; ++ks) {
                const v4i a = *(const v4i *)(wt + ks * 1024);
                v4i o1 = {0, 0, 0, 0};
                if constexpr (WZ) o1 = *(const v4i *)(wt + (KS + ks) * 1024);
#pragma unroll
                for (int i = 0; i < PB; ++i)
                    if (i < nb) {
                        const v4i b = operand(wb[i], ks);
                        acc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[i], 0, 0, 0);
                        if constexpr (WZ) rs[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(o1, b, rs[i], 0, 0, 0);
                    }
            }
            const int4 ch = *(const int4 *)(q.colch + c4); // output channels of the lane's columns; the dead ones (-1) are a suffix
            if (ch.x < 0) continue;
            const float4 cA = *(const float4 *)(p.A + c4), cS = *(const float4 *)(p.S + c4);
            const bool dword = ch.w == ch.x + 3 && ((N | ch.x) & 3) == 0;
#pragma unroll
            for (int i = 0; i < PB; ++i) {
                if (i < nb) {
                    v4i a = acc[i];
                    if constexpr (WZ) {
                        const int4 wz = *(const int4 *)(p.wzp + c4);
                        a[0] -= wz.x * rs[i][0], a[1] -= wz.y * rs[i][1], a[2] -= wz.z * rs[i][2], a[3] -= wz.w * rs[i][3];
                    }
                    const uint32_t d = requant_pack4<MG, XR4>(a[0], a[1], a[2], a[3], cA, cS, p.lo_f, p.hi_f);
                    if (live[i]) {
                        int8_t *dst = out + opix[i] * N + ch.x;
                        if (dword) {
                            *(uint32_t *)dst = d;
                        } else {
                            dst[0] = (int8_t)d;
                            if (ch.y >= 0) dst[1] = (int8_t)(d >> 8);
                            if (ch.z >= 0) dst[2] = (int8_t)(d >> 16);
                            if (ch.w >= 0) dst[3] = (int8_t)(d >> 24);
                        }
                    }
                }
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
// The tile layout, then conv_gemm_plan_pads' search over it -- the widest N slice that leaves room for a second workgroup per CU, else
// the widest that fits; G whole images (<= 32 KiB of tiles) or bands of output rows (wide rows: of two output rows).  The class: Cg % 4 == 0 and C % 4 == 0 (every k
// dword is four channels of one tap at a dword boundary), whole-dword image rows.
bool conv_grp_plan(ConvGrpArgs &q, std::vector<int> &tap, std::vector<int> &colch, int H, int W, int C, int N, int groups, int KH, int KW,
                   int sh, int sw, int OH, int OW, int padt, int padl, bool wz) {
    if (padt < 0 || padl < 0 || groups < 1) return false;
    if (H < 1 || W < 1 || C < 1 || N < 1 || KH < 1 || KW < 1 || sh < 1 || sw < 1 || OH < 1 || OW < 1) return false;
    if (C % groups != 0 || N % groups != 0) return false;
    const int Cg = C / groups, Ng = N / groups;
    if (Cg % 4 != 0 || C % 4 != 0 || (W * C) % 4 != 0) return false;
    const int GPT = Ng < 16 ? std::min(groups, 16 / Ng) : 0, TPG = Ng < 16 ? 0 : (Ng + 15) / 16;
    const int SPAN = GPT ? GPT * Cg : Cg, NT = GPT ? (groups + GPT - 1) / GPT : groups * TPG;
    const long long K = (long long)KH * KW * SPAN;
    if (K > 64LL * CONV_GEMM_KS_MAX || (long long)KW * C > 8192) return false;
    const int KS = (int)((K + 63) / 64), PW = wz ? 2 * KS : KS;
    const int LP = (padl * C + 15) & ~15;
    // bytes read right of the image row: the last window's last tap, a span that a ragged packed tile lets start at most at channel C,
    // and the 16 bytes of a read
    const int over = std::max(0, ((OW - 1) * sw - padl + KW - 1) * C + C + SPAN + 16 - W * C);
    const int ROW = ((LP + W * C + over + 15) & ~15) + 16;
    const int tabb = KS * 64;
    auto rows_for = [&](int bh) { return (bh - 1) * sh + KH; };
    ConvGemmArgs &a = q.g;
    a.H = H, a.W = W, a.C = C, a.N = N, a.KH = KH, a.KW = KW, a.sh = sh, a.sw = sw, a.OH = OH, a.OW = OW;
    a.padl = padl, a.padt = padt, a.KWCP = 0, a.KS = KS, a.NT = NT, a.LP = LP, a.ROW = ROW;
    q.groups = groups, q.Cg = Cg, q.Ng = Ng, q.SPAN = SPAN, q.GPT = GPT, q.TPG = TPG, q.PW = PW;
    for (int pass = 0; pass < 2; ++pass) {
        const int lmax = pass == 0 ? 80 * 1024 : CONV_GEMM_LDS_MAX;
        for (int NTS = NT; NTS >= 1; --NTS) {
            const int NSL = (NT + NTS - 1) / NTS;
            if (NSL > 1 && (NT + NSL - 1) / NSL != NTS) continue; // balanced slices only
            const long long wbytes = (long long)NTS * PW * 1024;
            // (32 KiB of tiles, conv_gemm_rt: 48: at 56x56x128 G = 32 bands in 32 KiB ran x1.67 faster than bands in 96 KiB, which leave one
            // workgroup per CU.  Wide image rows -- 56x56x256: three rows are 44 KiB -- get, in the second pass, what a band
            // of two output rows needs, so that they run here and not as the twin)
            const long long want = pass == 0 ? 32 * 1024 : std::max<long long>(32 * 1024, (long long)rows_for(std::min(OH, 2)) * ROW);
            const long long cap = std::min<long long>(lmax - wbytes - tabb - 256, want);
            // (the first pass also wants bands of at least 4 output rows: thinner bands leave waves without a 16-pixel chunk)
            if (cap < (long long)rows_for(pass == 0 ? std::min(OH, 4) : 1) * ROW) continue;
            if ((long long)rows_for(OH) * ROW <= cap) {
                a.NBANDS = 1, a.BH = OH, a.RB = rows_for(OH), a.TILE = a.RB * ROW;
                a.G = (int)std::max(1LL, std::min(16LL, cap / a.TILE));
            } else {
                int bh = OH;
                while (bh > 1 && (long long)rows_for(bh) * ROW > cap) --bh;
                const int nb = (OH + bh - 1) / bh;
                bh = (OH + nb - 1) / nb;
                a.BH = bh, a.NBANDS = (OH + bh - 1) / bh, a.RB = rows_for(bh), a.TILE = a.RB * ROW, a.G = 1;
            }
            a.NTS = NTS, a.NSL = NSL, a.TB = 1;
            a.xoff = (int)wbytes, a.toff = a.xoff + a.G * a.TILE + 256, a.moff = a.toff + tabb;
            a.lds = a.toff + tabb;
            tap.assign((size_t)KS * 16, 0);
            for (int d = 0; d * 4 < K; ++d) {
                const int k = d * 4, t = k / SPAN, c = k % SPAN;
                tap[(size_t)d] = (t / KW) * ROW + (t % KW) * C + c;
            }
            colch.assign((size_t)NT * 16, -1);
            for (int t = 0; t < NT; ++t)
                for (int j = 0; j < 16; ++j) {
                    if (GPT) {
                        if (j < std::min(GPT, groups - t * GPT) * Ng) colch[(size_t)t * 16 + j] = t * GPT * Ng + j;
                    } else if ((t % TPG) * 16 + j < Ng) {
                        colch[(size_t)t * 16 + j] = (t / TPG) * Ng + (t % TPG) * 16 + j;
                    }
                }
            return true;
        }
    }
    return false;
}

// Per tile the fc_rt image of its [16][KS 64] matrix: column j's filter at k = tap SPAN + (its group's offset in the span) + c, zero
// elsewhere; with filter zero points, behind it the same pieces with ones at exactly those k
std::vector<int8_t> conv_grp_weight_image(const int8_t *w /*[N][KH][KW][Cg]*/, const ConvGrpArgs &q, const std::vector<int> &colch, bool wz) {
    const ConvGemmArgs &a = q.g;
    const int KP = a.KS * 64, T = a.KH * a.KW, rows = a.NT * 16;
    std::vector<int8_t> m((size_t)rows * KP, 0), o1(wz ? (size_t)rows * KP : 0, 0);
    for (int r = 0; r < rows; ++r) {
        const int ch = colch[(size_t)r];
        if (ch < 0) continue;
        const int t = r / 16, tbase = q.GPT ? t * q.SPAN : (t / q.TPG) * q.Cg;
        const int cb = (ch / q.Ng) * q.Cg - tbase;       // the column's group inside the tile's span
        for (int tp = 0; tp < T; ++tp)
            for (int c = 0; c < q.Cg; ++c) {
                const size_t k = (size_t)r * KP + (size_t)tp * q.SPAN + cb + c;
                m[k] = w[((size_t)ch * T + tp) * q.Cg + c];
                if (wz) o1[k] = 1;
            }
    }
    const std::vector<int8_t> im = fc_rt_weight_image(m.data(), KP, rows);
    if (!wz) return im;
    const std::vector<int8_t> io = fc_rt_weight_image(o1.data(), KP, rows);
    const size_t tb = (size_t)a.KS * 1024;
    std::vector<int8_t> img(2 * im.size());
    for (int t = 0; t < a.NT; ++t) {
        std::copy(im.begin() + t * tb, im.begin() + (t + 1) * tb, img.begin() + 2 * t * tb);
        std::copy(io.begin() + t * tb, io.begin() + (t + 1) * tb, img.begin() + (2 * t + 1) * tb);
    }
    return img;
}

template <int AL, bool WZ, int MG, uint32_t XR4>
static void launch_conv_grp_t(const int8_t *in, int8_t *out, const ConvGrpArgs &a, int batch, hipStream_t s) {
    int per_cu = 1;
    { // occupancy per (device, LDS bytes), asked once; the attribute is the whole budget, so no shape lowers it for another
        static std::mutex mu;
        static std::map<std::pair<int, int>, int> cache;
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> lock(mu);
        auto it = cache.find({dev, a.g.lds});
        if (it == cache.end()) {
            (void)hipFuncSetAttribute((const void *)conv_grp_rt<AL, WZ, MG, XR4>, hipFuncAttributeMaxDynamicSharedMemorySize, CONV_GEMM_LDS_MAX);
            int n = 1;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, conv_grp_rt<AL, WZ, MG, XR4>, 256, (size_t)a.g.lds) != hipSuccess || n < 1) {
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
    MF_LAUNCH((conv_grp_rt<AL, WZ, MG, XR4>), dim3((unsigned)(walkers * a.g.NSL)), dim3(256), a.g.lds, s, in, out, a, batch);
}
template <int AL, int MG, uint32_t XR4>
static void launch_conv_grp_w(const int8_t *in, int8_t *out, const ConvGrpArgs &a, bool wz, int batch, hipStream_t s) {
    if (wz) launch_conv_grp_t<AL, true, MG, XR4>(in, out, a, batch, s);
    else launch_conv_grp_t<AL, false, MG, XR4>(in, out, a, batch, s);
}
void launch_conv_grp(const int8_t *in, int8_t *out, const ConvGrpArgs &a, bool wz, int batch, hipStream_t s) {
    if (batch <= 0) return;
    const int magic = a.g.magic, xr = a.g.xr;
    if (a.SPAN % 16 == 0 && a.g.C % 16 == 0) MF_DISPATCH4(magic, xr, launch_conv_grp_w, (in, out, a, wz, batch, s), 16)
    else MF_DISPATCH4(magic, xr, launch_conv_grp_w, (in, out, a, wz, batch, s), 4)
}

} // namespace k
} // namespace mf
