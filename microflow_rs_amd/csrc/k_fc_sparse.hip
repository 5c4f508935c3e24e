// k_fc_sparse.hip -- FullyConnected with 2:4-structured-sparse weights (src/ops/fully_connected.rs:24-82) on gfx950's sparse int8
// matrix instruction, v_smfmac_i32_16x16x128_i8: half the matrix instructions of fc_mfma (k_gemm.hip) per output.
//
// Arithmetic contract, shared device helpers and launch plumbing: k_common.hpp.
#include "k_common.hpp"

namespace mf {
namespace k {

// ------------------------------------------------------------------------
//   Y[m][n] = requant( sum_k X[m][k] * W[n][k]  - wzp * rowsum(X[m])  + (c3 - c2[n]) )
//
// Taken when every aligned group of four weights along K holds at most two non-zero bytes (ops.hip).  The operand map of the
// instruction (scripts/ubench/smfmac_check.hip, 0 of 64 random trials differ from it):
//   A (sparse, 16 rows x 128 k): lane (row r = lane & 15, group ga = lane >> 4) holds 16 stored bytes; byte s is one of the two
//       kept bytes of the 4-group k = 64 (ga & 1) + 32 (s >> 3) + 16 (ga >> 1) + 4 ((s & 7) >> 1) + {0..3}, the position in the
//       group being bits 2s..2s+1 of the lane's index word.
//   B (dense, 16 columns x 128 k): lane (column c = lane & 15, lb = lane >> 4) holds k = 32 lb .. 32 lb + 31, 32 bytes.
//   D: lane (column c, lg = lane >> 4) holds rows 4 lg .. 4 lg + 3.
// A = W rows (n), B = X rows (m), so that D[n][m] leaves every lane with results of ONE output row m.
//
//   weight image (fc_sparse24_image): per k tile of 128 and per 16-row n tile, the 64 lanes' A registers in lane order (1 KiB),
//       then in a second array the 64 lanes' index words (256 B).  Row r of n tile t of a 64-row slab is W row
//       16 (r >> 2) + 4 t + (r & 3) of the slab, so that the four tiles of a wave give each lane 16 CONSECUTIVE n: one 16-byte
//       store per lane and X row.  Both arrays are read linearly by LDS-DMA and by the fragment reads (conflict-free as they stand).
//   tile     : BM x BN per workgroup, WM x WN waves, each wave (BM / WM) x 64: BM / WM / 16 X tiles x 4 W tiles of 16 x 16.
//              256 x 256 with 8 waves, or 128 x 128 with 4 waves when the problem has too few 256^2 tiles to fill the chip.
//   staging  : BK = 128 bytes of k per step, double buffered, all by LDS-DMA (global_load_lds_dwordx4).  Per buffer: X [BM][128 B]
//              (16-byte slot XOR ((row >> 1) & 5): every ds_read_b128 service group of the B fragment reads -- rows
//              {0-3, 12-15} at one slot and rows {4-11} at the slot two on, or the other way round -- 16 distinct bank slots),
//              W values [BN / 16][1 KiB], W index words [BN / 16][256 B]: 52 KiB for 256^2, 5 / 8 of fc_mfma's W bytes.
//   schedule : fc_mfma's lockstep loop -- the DMAs of step t+1 fly during the products of step t; one vmcnt(0) + barrier per step.
//   hazard   : a dense MFMA and a sparse one back to back on one accumulator give wrong results (profiles/r06/smfmac_hazard.txt); this
//              kernel issues sparse ones only.
// The weight zero point term comes from the fc_rowsum pre-pass (p.rowsum).  The f32 epilogue is fc_mfma's, byte for byte.
// ------------------------------------------------------------------------
typedef int v8i __attribute__((ext_vector_type(8)));

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN) void fc_sparse24(const int8_t *__restrict__ X, int8_t *__restrict__ Y, FcGemmArgs p) {
    constexpr int BK = 128;
    constexpr int NW = WM * WN;
    constexpr int MT = BM / WM / 16, NT = 4; // 16 x 16 tiles per wave
    static_assert(BN / WN == 64, "a wave covers one 64-row slab of the weight image");
    constexpr int XT = BM * BK, VT = BN / 16 * 1024, IT = BN / 16 * 256, BUF = XT + VT + IT;
    constexpr int XP = XT / 1024 / NW, VP = VT / 1024 / NW, IP = IT / 1024; // 1 KiB DMA pieces (X, values per wave; index words)
    static_assert(XT % (1024 * NW) == 0 && VT % (1024 * NW) == 0 && IP <= NW, "DMA pieces must divide over the waves");
    auto key = [](int row) { return (row >> 1) & 5; };
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;

    // fc_mfma's XCD-aware 2-D tile order
    constexpr int PM = (BM == 128) ? 8 : 4, PN = 8;
    const int tiles_m = (p.M + BM - 1) / BM, tiles_n = p.N / BN;
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
    const int K = p.K, nk = K / BK, ntn = p.N / 16;
    const int8_t *Wv = p.w, *Wi = p.w + (size_t)nk * ntn * 1024;
    // rows past the matrix (ragged M) alias the last row -- their products are computed and dropped
    auto xrow = [&](int row) {
        const int g = tm * BM + row;
        return X + (size_t)(g < p.M ? g : p.M - 1) * K;
    };
    auto stage = [&](int kt, int buf) {
        const int r8 = lane >> 3, s8 = lane & 7;
        uint8_t *lb = lds + buf * BUF;
#pragma unroll
        for (int j = 0; j < XP; ++j) {
            const int i = wave * XP + j, row = 8 * i + r8;
            dma16(xrow(row) + (size_t)kt * BK + ((s8 ^ key(row)) << 4), lb + i * 1024);
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

    const int c = lane & 15, lb4 = lane >> 4;
    int xoff[MT], xkey[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int row = wm * (BM / WM) + t * 16 + c;
        xoff[t] = row * BK, xkey[t] = key(row);
    }
    const int wt0 = wn * 4; // first n tile of this wave within the workgroup's BN / 16

    int cur = 0;
    stage(0, 0);
    for (int kt = 0; kt < nk; ++kt, cur ^= 1) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        wg_sync();
        if (kt + 1 < nk) stage(kt + 1, cur ^ 1);
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

    // epilogue: lane (X row c of tile mt, lg) holds n = slab + 16 lg + 4 nt + i
    const int n0 = tn * BN + wn * 64 + 16 * lb4;
    float cA[16];
    int cK[16];
#pragma unroll
    for (int r = 0; r < 16; r += 4) {
        const float4 fa = *(const float4 *)(p.A + n0 + r);
        const int4 ik = *(const int4 *)(p.Kc + n0 + r);
        cA[r] = fa.x, cA[r + 1] = fa.y, cA[r + 2] = fa.z, cA[r + 3] = fa.w;
        cK[r] = ik.x, cK[r + 1] = ik.y, cK[r + 2] = ik.z, cK[r + 3] = ik.w;
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int m = tm * BM + wm * (BM / WM) + mt * 16 + c;
        if (m >= p.M) continue; // ragged last row tile
        const int corr = p.rowsum ? p.wzp * p.rowsum[m] : 0; // x1 = wzp * row-sum of the input
        uint32_t d[4];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int r = 4 * nt;
            const int q0 = requant(acc[nt][mt][0] + cK[r] - corr, cA[r], p.S, p.lo_f, p.hi_f);
            const int q1 = requant(acc[nt][mt][1] + cK[r + 1] - corr, cA[r + 1], p.S, p.lo_f, p.hi_f);
            const int q2 = requant(acc[nt][mt][2] + cK[r + 2] - corr, cA[r + 2], p.S, p.lo_f, p.hi_f);
            const int q3 = requant(acc[nt][mt][3] + cK[r + 3] - corr, cA[r + 3], p.S, p.lo_f, p.hi_f);
            d[nt] = pack4(q0, q1, q2, q3) ^ p.xr4;
        }
        *(uint4 *)(Y + (size_t)m * p.N + n0) = make_uint4(d[0], d[1], d[2], d[3]);
    }
}

// ---- host: weight image and launcher ----
bool fc_sparse24_eligible(const int8_t *w, int N, int K) {
    if (N % 128 || K % 128) return false;
    for (size_t g = 0; g < (size_t)N * K; g += 4) {
        const int nz = (w[g] != 0) + (w[g + 1] != 0) + (w[g + 2] != 0) + (w[g + 3] != 0);
        if (nz > 2) return false;
    }
    return true;
}
std::vector<int8_t> fc_sparse24_image(const int8_t *w, int N, int K) {
    const int nk = K / 128, ntn = N / 16;
    std::vector<int8_t> img((size_t)nk * ntn * (1024 + 256), 0);
    int8_t *vals = img.data();
    uint32_t *idx = (uint32_t *)(img.data() + (size_t)nk * ntn * 1024);
    for (int kt = 0; kt < nk; ++kt)
        for (int t = 0; t < ntn; ++t)
            for (int lane = 0; lane < 64; ++lane) {
                const int r = lane & 15, ga = lane >> 4, lt = t & 3;
                const int n = (t >> 2) * 64 + 16 * (r >> 2) + 4 * lt + (r & 3);
                const int8_t *wr = w + (size_t)n * K + (size_t)kt * 128;
                int8_t *v = vals + (((size_t)kt * ntn + t) * 64 + lane) * 16;
                uint32_t word = 0;
                for (int s = 0; s < 16; s += 2) {
                    const int k0 = 64 * (ga & 1) + 32 * (s >> 3) + 16 * (ga >> 1) + 4 * ((s & 7) >> 1);
                    // the two kept positions, distinct and ascending; a group with fewer than two non-zero bytes keeps zeros
                    int pos[2], np = 0;
                    for (int q = 0; q < 4 && np < 2; ++q)
                        if (wr[k0 + q] != 0) pos[np++] = q;
                    if (np == 0) pos[0] = 0, pos[1] = 1;
                    else if (np == 1) pos[1] = pos[0] == 3 ? 3 : pos[0] + 1, pos[0] = pos[0] == 3 ? 2 : pos[0];
                    v[s] = wr[k0 + pos[0]], v[s + 1] = wr[k0 + pos[1]];
                    word |= (uint32_t)pos[0] << (2 * s) | (uint32_t)pos[1] << (2 * s + 2);
                }
                idx[((size_t)kt * ntn + t) * 64 + lane] = word;
            }
    return img;
}
template <int BM, int BN, int WM, int WN>
static void launch_fc_sparse24_t(const int8_t *in, int8_t *out, const FcGemmArgs &a, hipStream_t s) {
    constexpr int lds = 2 * (BM * 128 + BN / 16 * (1024 + 256));
    static LaunchState st;
    (void)prepared(st, fc_sparse24<BM, BN, WM, WN>, 64 * WM * WN, lds);
    const int grid = ((a.M + BM - 1) / BM) * (a.N / BN);
    MF_LAUNCH((fc_sparse24<BM, BN, WM, WN>), dim3(grid), dim3(64 * WM * WN), lds, s, in, out, a);
}
void launch_fc_sparse24(const int8_t *in, int8_t *out, const FcGemmArgs &a, hipStream_t s) {
    // fc_mfma's tile choice: 256 x 256 tiles where there are enough of them to fill the chip
    const bool big = a.N % 256 == 0 && (size_t)((a.M + 255) / 256) * (a.N / 256) >= 192;
    if (big) launch_fc_sparse24_t<256, 256, 2, 4>(in, out, a, s);
    else launch_fc_sparse24_t<128, 128, 2, 2>(in, out, a, s);
}

} // namespace k
} // namespace mf
