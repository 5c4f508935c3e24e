// k_conv_stream_sparse.hip -- deep Conv2D (microflow::ops::conv_2d, src/ops/conv_2d.rs:28-108) whose filter is 2:4-structured-sparse
// along K' = (ky, kx, c), on gfx950's sparse int8 matrix instruction v_smfmac_i32_16x16x128_i8: conv_stream_sp24.
//
//   Y[m][n] = requant( sum_k A[m][k] W[n][k] + Kc[n] ),   m = (image, oy, ox),  k = (ky, kx, c),  M = batch OH OW,  K' = KH KW C
//
// is conv_stream_rt's product (k_conv_stream.hip) with half the matrix instructions per output.  The kernel is the GATHER of that one
// under the OPERAND MAP of fc_sparse24 (k_fc_sparse.hip), with the convolution's epilogue:
//
//   weights  : MFMA "A", sparse.  The filter as stored (OHWI) is the [N][K'] matrix k::fc_sparse24_image compresses: per k tile of 128
//              and 16-row n tile 1 KiB of kept bytes in lane order, then 256 B of index words; the slab row order leaves a lane 16
//              CONSECUTIVE n.  C % 128 == 0, so k tile kt of the image is the step (ky, kx, c0) of the scalar tap counters below.  Read
//              linearly by LDS-DMA and by the fragment reads (fc_sparse24's, unchanged).
//   pixels   : MFMA "B", dense: 16 columns (rows m) x 128 k, 32 bytes per lane.  Gathered as in conv_stream_rt: a lane decomposes the XP
//              rows whose DMA pieces it issues ONCE per tile into (byte offset of the window's first pixel, iy0, ix0); per k step it
//              adds the workgroup-uniform tap offset and tests the tap against the image; a tap outside only redirects the DMA's source
//              to the operator's 128-byte line of the input zero point.  The LDS image is fc_sparse24's X layout, [BM][128 B] with the
//              16-byte slot XOR ((row >> 1) & 5) -- the key the SOURCE slot of a piece and the offset into the zero-point line use --
//              and a lane's fragment is two ds_read_b128 (k = 32 lb .. 32 lb + 31).
//   sums     : the instruction drops only products whose weight byte is zero, so the accumulator is sum x w with zero-point bytes at
//              the padded taps: the sum the operator's Kc = -izp sum w was folded for.  Nothing else changes in the constants.
//   tile     : BM x BM per workgroup, 2 x BM / 64 waves, each wave (BM / 2) x 64: BM / 32 pixel tiles x 4 weight tiles of 16 x 16.
//              256 with 8 waves where there are enough such tiles to fill the chip (conv_stream_tile), else 128 with 4 waves.
//   staging  : BK = 128, double buffered, all by LDS-DMA.  Per buffer: pixels BM x 128 B, values BM / 16 KiB, index words BM / 16 x 256 B:
//              52 KiB for 256, 26 KiB for 128 (conv_stream_rt: 64 and 32 KiB).
//   schedule : the lockstep loop: the DMAs of step t + 1 are issued in front of the products of step t, one vmcnt(0) + wg_sync() per
//              step.  Every barrier is wg_sync().  XCD-aware tile order as in fc_mfma.
//   ragged M : rows past M alias row M - 1 (computed and dropped); nothing is stored for them.
//   hazard   : a dense MFMA and a sparse one back to back on one accumulator give wrong results (profiles/r06/smfmac_hazard.txt): the
//              accumulators are zeroed by plain moves and touched by the sparse instruction only.
//   epilogue : per-channel A / S / Kc, the 16 a lane needs per column block; requant_pack4<MG, XR4> in the operator's proven mode
//              (0 .. 2); one 16-byte store per lane and pixel row.
//
// Selected per launch (ops.hip conv_stream_sparse_selected) where conv_stream_rt is, the filter is 2:4 and the class is kept by the
// measurement (conv_stream_sp24_min_rows below).
#include "k_common.hpp"

namespace mf {
namespace k {

typedef int v8i __attribute__((ext_vector_type(8)));

template <int BM, int MG, uint32_t XR4>
__global__ __launch_bounds__(BM * 2) void conv_stream_sp24(const int8_t *__restrict__ in, int8_t *__restrict__ out, ConvStreamArgs p) {
    constexpr int BK = 128, BN = BM, WM = 2, WN = BN / 64;
    constexpr int NW = WM * WN;              // waves per workgroup
    constexpr int MT = BM / WM / 16, NT = 4; // 16 x 16 tiles per wave: a wave covers one 64-row slab of the weight image
    constexpr int XT = BM * BK, VT = BN / 16 * 1024, IT = BN / 16 * 256, BUF = XT + VT + IT;
    constexpr int XP = XT / 1024 / NW, VP = VT / 1024 / NW, IP = IT / 1024; // 1 KiB DMA pieces (pixels, values per wave; index words)
    static_assert(XT % (1024 * NW) == 0 && VT % (1024 * NW) == 0 && IT % 1024 == 0 && IP <= NW, "DMA pieces must divide over the waves");
    auto key = [](int row) { return (row >> 1) & 5; }; // fc_sparse24's slot key (k_fc_sparse.hip: the bank argument)
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;

    // XCD-aware 2-D tile order (k_gemm.hip)
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
    const int nk = K / BK, ntn = p.N / 16;
    const int8_t *Wv = p.w, *Wi = p.w + (size_t)nk * ntn * 1024; // the image: values, then index words

    // this lane's XP gathered rows: DMA piece i (1 KiB) of the pixel tile = rows 8i .. 8i + 7, lane -> (row, swizzled 16-byte slot)
    const int r8 = lane >> 3, s8 = lane & 7;
    const int OHW = p.OH * p.OW;
    long long abase[XP]; // byte offset of (window's first pixel, channel 0) + the lane's source slot; negative where the window starts in the padding
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
    // k step kt = tap (ky, kx), channels c0 .. c0 + 127 (workgroup-uniform) = k tile kt of the weight image
    auto stage = [&](int kt, int ky, int kx, int c0, int buf) {
        uint8_t *lb = lds + buf * BUF;
        const long long tapoff = ((long long)ky * p.W + kx) * p.C + c0;
#pragma unroll
        for (int j = 0; j < XP; ++j) {
            const bool inside = (unsigned)(aiy[j] + ky) < (unsigned)p.H && (unsigned)(aix[j] + kx) < (unsigned)p.W;
            const int8_t *src = inside ? in + (abase[j] + tapoff) : p.zline + aswz[j];
            dma16(src, lb + (wave * XP + j) * 1024);
        }
        const size_t t0 = (size_t)kt * ntn + (size_t)tn * (BN / 16); // first n tile of this workgroup in k tile kt
#pragma unroll
        for (int j = 0; j < VP; ++j) {
            const int i = wave * VP + j;
            dma16(Wv + (t0 + i) * 1024 + lane * 16, lb + XT + i * 1024);
        }
        if (wave < IP) dma16(Wi + t0 * 256 + wave * 1024 + lane * 16, lb + XT + VT + wave * 1024);
    };

    v4i acc[NT][MT];
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < MT; ++b) acc[a][b] = v4i{0, 0, 0, 0};

    // "B" fragment of this lane: pixel row c of tile t, k = 32 lb4 .. 32 lb4 + 31
    const int c = lane & 15, lb4 = lane >> 4;
    int xoff[MT], xkey[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int row = wm * (BM / WM) + t * 16 + c;
        xoff[t] = row * BK, xkey[t] = key(row);
    }
    const int wt0 = wn * 4; // first n tile of this wave within the workgroup's BN / 16

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
        v4i a[NT];
        int ix[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            a[t] = *(const v4i *)(lb + XT + (wt0 + t) * 1024 + lane * 16);
            ix[t] = *(const int *)(lb + XT + VT + (wt0 + t) * 256 + lane * 4);
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const v4i b0 = *(const v4i *)(lb + xoff[mt] + (((2 * lb4) ^ xkey[mt]) << 4));
            const v4i b1 = *(const v4i *)(lb + xoff[mt] + (((2 * lb4 + 1) ^ xkey[mt]) << 4));
            const v8i b = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt][mt] = __builtin_amdgcn_smfmac_i32_16x16x128_i8(a[nt], b, acc[nt][mt], ix[nt], 0, 0);
        }
    }

    // epilogue: lane (pixel row c of tile mt, lb4) holds n = slab + 16 lb4 + 4 nt + i, i = 0 .. 3: 16 consecutive channels of output row m
    const int n0 = tn * BN + wn * 64 + 16 * lb4;
    float4 cA[NT], cS[NT];
    int4 cK[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) {
        cA[q] = *(const float4 *)(p.A + n0 + 4 * q), cS[q] = *(const float4 *)(p.S + n0 + 4 * q);
        cK[q] = magic4<MG>(*(const int4 *)(p.Kc + n0 + 4 * q));
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int m = tm * BM + wm * (BM / WM) + mt * 16 + c;
        if (m >= M) continue; // ragged last row tile
        uint32_t d[NT];
#pragma unroll
        for (int q = 0; q < NT; ++q)
            d[q] = requant_pack4<MG, XR4>(acc[q][mt][0] + cK[q].x, acc[q][mt][1] + cK[q].y, acc[q][mt][2] + cK[q].z, acc[q][mt][3] + cK[q].w, cA[q],
                                          cS[q], p.lo_f, p.hi_f);
        *(uint4 *)(out + (size_t)m * p.N + n0) = make_uint4(d[0], d[1], d[2], d[3]);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
// From which row count a launch of a 2:4 filter's class takes conv_stream_sp24 instead of conv_stream_rt; 0: the class stays on
// conv_stream_rt.  The rule is the project's: the smallest swept row count from which the sparse kernel beats
// conv_stream_rt -- the parent build on the same pruned filter -- by more than the larger of the two spreads, and keeps winning above it
// (profiles/r28/time_conv_sparse.txt).  MF_CONV_SPARSE_ALL (measurements: the sweeps below the thresholds): from
// conv_stream_rt's own threshold on, whatever the class's count.
int conv_stream_sp24_min_rows(const ConvStreamArgs &a) {
    if (switches().conv_sparse_all) return a.min_rows;
    const int rows = a.KH * a.KW == 1 ? CONV_SPARSE_MIN_ROWS_1X1 : CONV_SPARSE_MIN_ROWS_KXK;
    return rows ? (rows > a.min_rows ? rows : a.min_rows) : 0;
}

template <int BM, int MG, uint32_t XR4> static void launch_conv_stream_sp24_t(const int8_t *in, int8_t *out, const ConvStreamArgs &a, hipStream_t s) {
    constexpr int lds = 2 * (BM * 128 + BM / 16 * (1024 + 256)); // 256: 104 KiB; 128: 52 KiB
    static LaunchState st;
    (void)prepared(st, conv_stream_sp24<BM, MG, XR4>, 2 * BM, lds);
    const int grid = ((a.M + BM - 1) / BM) * (a.N / BM);
    MF_LAUNCH((conv_stream_sp24<BM, MG, XR4>), dim3(grid), dim3(2 * BM), lds, s, in, out, a);
}
// a.w: the operator's fc_sparse24_image of the filter; a.M set.  The tile choice is conv_stream_rt's (conv_stream_tile).
void launch_conv_stream_sp24(const int8_t *in, int8_t *out, const ConvStreamArgs &a, hipStream_t s) {
    if (a.M <= 0) return;
    if (conv_stream_tile(a, (size_t)a.M) == 256) MF_DISPATCH4(a.magic, a.xr, launch_conv_stream_sp24_t, (in, out, a, s), 256)
    else MF_DISPATCH4(a.magic, a.xr, launch_conv_stream_sp24_t, (in, out, a, s), 128)
}

} // namespace k
} // namespace mf
