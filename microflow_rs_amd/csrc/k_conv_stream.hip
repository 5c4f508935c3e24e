// k_conv_stream.hip -- deep Conv2D (microflow::ops::conv_2d, src/ops/conv_2d.rs:28-108) as a weight-streaming implicit GEMM over
// the whole batch: conv_stream_rt.
//
// conv_gemm_rt (k_conv_gemm.hip) keeps a slice of the filter resident in LDS and walks images past it; with C and N in the hundreds the
// filter is the LARGE operand (3x3x512 -> 512: 2.25 MiB) and the image the small one, so that kernel runs in dozens of slices of one or
// two tiles, each re-staging the image.  Here nothing is resident: the output pixels of ALL images of a launch are the rows of one
// NT GEMM
//
//   Y[m][n] = requant( sum_k A[m][k] W[n][k] + Kc[n] ),   m = (image, oy, ox),  k = (ky, kx, c),  M = batch OH OW,  K' = KH KW C
//
// whose W is the filter exactly as stored (OHWI: [N][K'], k contiguous) and whose Y is the NHWC output tensor row by row.  Both
// operands stream through LDS as in fc_mfma (k_gemm.hip), with the same tile shapes, LDS image, swizzle, fragment maps, XCD-aware
// tile order and packed 16-byte store; what is new is operand A, which exists nowhere in memory and is GATHERED by the DMAs:
//
//   k steps  : BK = 128 bytes.  C % 128 == 0, so a k step (ky, kx, c0) lies inside ONE tap, and row m's 128 bytes of it are the
//              contiguous run in[img][oy sh + ky - padt][ox sw + kx - padl][c0 .. c0 + 127] of the NHWC input.
//   rows     : a lane issues the DMA pieces of the same XP (row, 16-byte slot) positions for every k step of a tile, so it decomposes
//              those rows ONCE per tile into (byte offset of the window's first pixel, iy0, ix0) and keeps them in registers
//              (4 rows: 16 registers).  An image may start anywhere in a tile: every row is decomposed on its own.
//   taps     : the tap of a k step is workgroup-uniform (three scalar counters, no division in the loop).  Per piece the lane adds the
//              tap's byte offset and tests 0 <= iy0 + ky < H, 0 <= ix0 + kx < W; a tap outside the image only REDIRECTS the DMA's
//              source to a 128-byte line of the input zero point in device memory (the operator's).  The accumulator is therefore
//              sum x w with zero-point bytes at the padded taps -- the sum the per-channel Kc = -izp sum w was folded for
//              (conv2d_generic, and the zero-point halo of the tile kernels) -- with no branch in the MFMA section and no halo tile.
//   1x1 s1   : every tap test passes and the offsets are m C + c0: a plain GEMM on X.
//   ragged M : fc_mfma's rule: rows past M alias row M - 1 (computed and dropped), nothing is stored for them.
//   schedule : the lockstep loop (fc_mfma<128, 128>'s, fc_sparse24's): the DMAs of step t + 1 fly during the MFMAs of step t, one
//              vmcnt(0) + wg_sync() per step, for both tile sizes.  Every barrier is wg_sync().
//   epilogue : the convolution's own per-channel A / S / Kc (a lane loads the 16 it needs per column block), requant_pack4<MG, XR4> in
//              the mode the host proved for the operator (0 .. 2), one 16-byte store per lane and 32 x 32 tile.
//
// Filter zero points stay on conv_gemm_rt<wzp>.  The kernel is chosen per LAUNCH by the row count (ops.hip: conv_stream_selected): a
// 128 - 256 row tile cannot fill the chip with a few hundred rows, where the resident-filter kernels stay.
#include "k_common.hpp"

namespace mf {
namespace k {

typedef int v16i __attribute__((ext_vector_type(16)));

template <int BM, int BN, int WM, int WN, int MG, uint32_t XR4>
__global__ __launch_bounds__(64 * WM * WN) void conv_stream_rt(const int8_t *__restrict__ in, int8_t *__restrict__ out, ConvStreamArgs p) {
    constexpr int BK = 128;
    constexpr int NW = WM * WN;                              // waves per workgroup
    constexpr int MT = BM / WM / 32, NT = BN / WN / 32;      // 32x32 MFMA tiles per wave
    constexpr int XT = BM * BK, WT = BN * BK, BUF = XT + WT; // one staging buffer (two allocated)
    constexpr int XP = XT / 1024 / NW, WP = WT / 1024 / NW;  // 1 KiB DMA pieces per wave
    static_assert(XT % (1024 * NW) == 0 && WT % (1024 * NW) == 0, "DMA pieces must divide over the waves");
    auto key = [](int row) { return (row >> 1) & 7; };       // fc_mfma's swizzle key (k_gemm.hip: the bank argument)
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;

    // XCD-aware 2-D tile order (k_gemm.hip): the PM x PN tiles co-resident on one XCD share PM A panels and PN W panels in its L2
    constexpr int PM = (BM == 128) ? 8 : 4, PN = 8;
    const int M = p.M, K = p.K;
    const int tiles_m = (M + BM - 1) / BM, tiles_n = p.N / BN;
    int tm, tn;
    {
        const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        const int patches_n = tiles_n / PN, npatch = (tiles_m / PM) * patches_n;
        if (tiles_m % PM == 0 && tiles_n % PN == 0 && (npatch & 7) == 0) {
            const int patch = xcd * (npatch >> 3) + j / (PM * PN), t = j % (PM * PN);
            tm = (patch / patches_n) * PM + t / PN;
            tn = (patch % patches_n) * PN + t % PN;
        } else {
            tm = blockIdx.x / tiles_n, tn = blockIdx.x % tiles_n;
        }
    }
    const int8_t *Wt = p.w + (size_t)tn * BN * K;

    // this lane's XP gathered rows: DMA piece i (1 KiB) of the A tile = rows 8i .. 8i + 7, lane -> (row, swizzled 16-byte slot)
    const int r8 = lane >> 3, s8 = lane & 7;
    const int OHW = p.OH * p.OW;
    long long abase[XP]; // byte offset of (window's first pixel, channel 0) + the lane's slot; negative where the window starts in the padding
    int aiy[XP], aix[XP], aswz[XP];
#pragma unroll
    for (int j = 0; j < XP; ++j) {
        const int row = 8 * (wave * XP + j) + r8;
        const int gr = tm * BM + row, g = gr < M ? gr : M - 1; // rows past the matrix alias the last row
        const int img = g / OHW, rem = g - img * OHW, oy = rem / p.OW, ox = rem - oy * p.OW;
        aiy[j] = oy * p.sh - p.padt, aix[j] = ox * p.sw - p.padl;
        aswz[j] = (s8 ^ key(row)) << 4;
        abase[j] = (((long long)img * p.H + aiy[j]) * p.W + aix[j]) * p.C + aswz[j];
    }
    // k step kt = tap (ky, kx), channels c0 .. c0 + 127 (workgroup-uniform)
    auto stage = [&](int kt, int ky, int kx, int c0, int buf) {
        const long long tapoff = ((long long)ky * p.W + kx) * p.C + c0;
#pragma unroll
        for (int j = 0; j < XP; ++j) {
            const bool inside = (unsigned)(aiy[j] + ky) < (unsigned)p.H && (unsigned)(aix[j] + kx) < (unsigned)p.W;
            const int8_t *src = inside ? in + (abase[j] + tapoff) : p.zline + aswz[j];
            dma16(src, lds + buf * BUF + (wave * XP + j) * 1024);
        }
#pragma unroll
        for (int j = 0; j < WP; ++j) {
            const int i = wave * WP + j, row = 8 * i + r8;
            dma16(Wt + (size_t)row * K + (size_t)kt * BK + ((s8 ^ key(row)) << 4), lds + buf * BUF + XT + i * 1024);
        }
    };

    v16i acc[NT][MT];
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < MT; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0;

    // fragment rows of this lane: MFMA "A" = W rows (n, permuted so that a lane ends with 16 CONSECUTIVE n), "B" = gathered rows (m)
    const int rho = lane & 31, half = lane >> 5;
    const int nloc = 16 * ((rho >> 2) & 1) + 4 * (rho >> 3) + (rho & 3);
    int xoff[MT], woff[NT], xkey[MT], wkey[NT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int row = wm * (BM / WM) + t * 32 + rho;
        xoff[t] = row * BK, xkey[t] = key(row);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int row = wn * (BN / WN) + t * 32 + nloc;
        woff[t] = XT + row * BK, wkey[t] = key(row);
    }

    const int nk = K / BK;
    int ky = 0, kx = 0, c0 = 0, cur = 0;
    stage(0, 0, 0, 0, 0);
    for (int kt = 0; kt < nk; ++kt, cur ^= 1) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's pieces of tile kt have landed ...
        wg_sync();                                       // ... and every other wave's; all reads of the other buffer are done
        if (kt + 1 < nk) {
            c0 += BK;
            if (c0 == p.C) {
                c0 = 0;
                if (++kx == p.KW) kx = 0, ++ky;
            }
            stage(kt + 1, ky, kx, c0, cur ^ 1);
        }
        const uint8_t *lb = lds + cur * BUF;
#pragma unroll
        for (int ks = 0; ks < BK / 32; ++ks) {
            v4i a[NT], b[MT];
#pragma unroll
            for (int t = 0; t < MT; ++t) b[t] = *(const v4i *)(lb + xoff[t] + (((ks * 2 + half) ^ xkey[t]) << 4));
#pragma unroll
            for (int t = 0; t < NT; ++t) a[t] = *(const v4i *)(lb + woff[t] + (((ks * 2 + half) ^ wkey[t]) << 4));
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[nt], b[mt], acc[nt][mt], 0, 0, 0);
        }
    }

    // epilogue: lane (m column = lane & 31, half) holds n = block + 16 half + r, r = 0 .. 15, of output row m
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n0 = tn * BN + wn * (BN / WN) + nt * 32 + 16 * half;
        float4 cA[4], cS[4];
        int4 cK[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            cA[q] = *(const float4 *)(p.A + n0 + 4 * q), cS[q] = *(const float4 *)(p.S + n0 + 4 * q);
            cK[q] = magic4<MG>(*(const int4 *)(p.Kc + n0 + 4 * q));
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int m = tm * BM + wm * (BM / WM) + mt * 32 + rho;
            if (m >= M) continue; // ragged last row tile
            uint32_t d[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                d[q] = requant_pack4<MG, XR4>(acc[nt][mt][4 * q] + cK[q].x, acc[nt][mt][4 * q + 1] + cK[q].y, acc[nt][mt][4 * q + 2] + cK[q].z,
                                              acc[nt][mt][4 * q + 3] + cK[q].w, cA[q], cS[q], p.lo_f, p.hi_f);
            *(uint4 *)(out + (size_t)m * p.N + n0) = make_uint4(d[0], d[1], d[2], d[3]);
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
// The class the kernel serves, and from which row count a launch selects it.  The thresholds are measured (profiles/r27/
// time_conv_stream.txt): the smallest row count of the sweep from which conv_stream_rt beats the kernel it replaces by more than the
// larger of the two spreads.  MF_CONV_STREAM_MIN_ROWS (measurements) replaces them.
bool conv_stream_plan(ConvStreamArgs &a, const ConvStreamSpec &s) {
    if (s.depthwise || s.groups != 1 || s.dh != 1 || s.dw != 1) return false;
    if (s.wz || !s.finite) return false;                 // filter zero points: conv_gemm_rt<wzp>; NaN constants: conv2d_generic
    if (s.H < 1 || s.W < 1 || s.C < 1 || s.N < 1 || s.KH < 1 || s.KW < 1 || s.sh < 1 || s.sw < 1 || s.OH < 1 || s.OW < 1) return false;
    if (s.padt < 0 || s.padl < 0) return false;
    if (s.C % 128 != 0 || s.N % 128 != 0) return false;   // a k step inside one tap; whole column tiles
    if ((long long)s.KH * s.KW * s.C > 0x7fffffffLL / 512 || (long long)s.OH * s.OW > (1 << 24)) return false; // (int arithmetic of the kernel)
    a.H = s.H, a.W = s.W, a.C = s.C, a.N = s.N, a.KH = s.KH, a.KW = s.KW, a.sh = s.sh, a.sw = s.sw, a.OH = s.OH, a.OW = s.OW;
    a.padt = s.padt, a.padl = s.padl, a.K = s.KH * s.KW * s.C, a.M = 0;
    const int forced = switches().conv_stream_min_rows;
    const bool small = (long long)a.K * s.N <= 96 * 1024;
    const bool unit = s.KH * s.KW == 1 && s.sh == 1 && s.sw == 1;
    a.min_rows = forced > 0 ? forced : small ? (unit ? CONV_STREAM_MIN_ROWS_SMALL_S1 : CONV_STREAM_MIN_ROWS) : s.C == 128 ? CONV_STREAM_MIN_ROWS_C128 :
                 (s.KH * s.KW > 1 && a.K < 4096) ? CONV_STREAM_MIN_ROWS_KXK_SHORT : CONV_STREAM_MIN_ROWS;
    return true;
}
bool conv_stream_rows_ok(const ConvStreamArgs &a, size_t rows) {
    return rows >= (size_t)a.min_rows && rows <= (size_t)(1 << 30) && (rows + 127) / 128 * (size_t)(a.N / 128) < (1u << 30);
}

template <int BT, int MG, uint32_t XR4> static void launch_conv_stream_t(const int8_t *in, int8_t *out, const ConvStreamArgs &a, hipStream_t s) {
    constexpr int WN = BT / 64, lds = 2 * (BT + BT) * 128; // 256: 2 x 4 waves, 128 KiB; 128: 2 x 2 waves, 64 KiB
    static LaunchState st;
    (void)prepared(st, conv_stream_rt<BT, BT, 2, WN, MG, XR4>, 128 * WN, lds);
    const int grid = ((a.M + BT - 1) / BT) * (a.N / BT);
    MF_LAUNCH((conv_stream_rt<BT, BT, 2, WN, MG, XR4>), dim3(grid), dim3(128 * WN), lds, s, in, out, a);
}
// launch_fc_mfma's choice: 256 x 256 tiles halve the L2 -> LDS traffic per MAC; they need enough tiles to fill the chip
int conv_stream_tile(const ConvStreamArgs &a, size_t rows) { return a.N % 256 == 0 && (rows + 255) / 256 * (size_t)(a.N / 256) >= 192 ? 256 : 128; }
void launch_conv_stream(const int8_t *in, int8_t *out, const ConvStreamArgs &a, hipStream_t s) {
    if (a.M <= 0) return;
    if (conv_stream_tile(a, (size_t)a.M) == 256) MF_DISPATCH4(a.magic, a.xr, launch_conv_stream_t, (in, out, a, s), 256)
    else MF_DISPATCH4(a.magic, a.xr, launch_conv_stream_t, (in, out, a, s), 128)
}

} // namespace k
} // namespace mf
