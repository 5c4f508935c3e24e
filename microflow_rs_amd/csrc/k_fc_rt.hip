// k_fc_rt.hip -- FullyConnected of ANY K and N on the int8 matrix pipe (microflow::ops::fully_connected,
// src/ops/fully_connected.rs:24-82: const generics INPUT_ROWS x INPUT_COLS x WEIGHTS_COLS, any of them).
//
// The shape-specialised kernels take two corners of that space (fc_rowwave: N in {1, 2, 4, 8}, K % 16 == 0, K >= 256;
// fc_mfma: N % 128 == 0, K % 128 == 0); every other shape with finite constants runs here instead of on the byte-wise
// fc_generic.  The product is pw_rt_lds's (k_rt.hip): v_mfma_i32_16x16x64_i8 with the weights as operand A (16 output
// columns x 64 k per tile and k step) and 16 rows of the batch as operand B.  What differs:
//
//   rows    : a step is R consecutive rows (a multiple of 16).  Their input is ONE contiguous byte range
//             [r0 K, (r0 + R) K) of the batch, staged by LDS-DMA (dma16) from the 16-byte-aligned address below it; a lane
//             builds its operand bytes from LDS at the row's byte offset (dword reads; + v_alignbyte when K % 4 != 0).
//             Only the staged range is read from HBM: an odd K costs no extra bytes.  The last DMA piece of the batch
//             reads at most 15 bytes past its end, inside the same 16-byte block (so inside the same page).
//   k tail  : the k positions past K are zeroed in the OPERAND (per-lane byte masks on the last k step), never in
//             memory, so neither the dot product nor the row sum sees them.
//   N       : the host image pads N to 16-column tiles with zero weights; padded columns are computed and never stored.
//   weights : a slice of NTS tiles (all of them when the padded image fits the LDS budget) stays resident for the
//             whole launch; the grid is NSL slices x row-tile walkers, and each slice re-reads the rows (L2 / MALL).
//   wzp     : the per-tensor weight zero point needs sum_k x[row][k]: one more MFMA per k step against a constant tile
//             of ones (registers), formed inside the launch from the staged tile: no scratch, no pre-pass, no counters.
//   output  : results go to an LDS patch; a single-slice step's R x N output bytes are one contiguous range and leave
//             in 16-byte stores, with bytes at the two unaligned edges; nothing past row `rows` is ever written.
//   work    : the 4 waves of a workgroup share the step's (16-row chunk, group of TB tiles) units.
//   buffers : NBUF = 2 row buffers where they fit (the next step's DMA flies during this step's products), else 1.
//
// Epilogue: requant_pack4<MG, XR4> (k_common.hpp), modes 0 .. 2 as the host proved them for the operator's constants;
// mode 0 converts the accumulator with v_cvt (round to nearest), which is fc_generic's (float)acc for every |acc|.
#include "k_common.hpp"
#include "k_fc_layer.hpp"
#include "k_fc_rt_body.hpp"

#include <algorithm>

namespace mf {
namespace k {

template <int AL, int MG, uint32_t XR4>
__global__ __launch_bounds__(256) void fc_rt(const int8_t *__restrict__ in, int8_t *__restrict__ out, FcRtArgs p, long long rows) {
    fc_rt_body<AL, MG, XR4, 0>(in, out, p, rows, F32Edge{});
}

// ---- host side ----------------------------------------------------------------------------------------------------
std::vector<int8_t> fc_rt_weight_image(const int8_t *w /*[N][K]*/, int K, int N) {
    const int KS = (K + 63) / 64, NT = (N + 15) / 16;
    std::vector<int8_t> img((size_t)NT * KS * 1024, 0);
    for (int nt = 0; nt < NT; ++nt)
        for (int ks = 0; ks < KS; ++ks)
            for (int lane = 0; lane < 64; ++lane) {
                const int n = nt * 16 + (lane & 15), k0 = ks * 64 + (lane >> 4) * 16;
                if (n >= N) continue;
                int8_t *dst = &img[(((size_t)nt * KS + ks) * 64 + lane) * 16];
                for (int i = 0; i < 16 && k0 + i < K; ++i) dst[i] = w[(size_t)n * K + k0 + i];
            }
    return img;
}

// Geometry: the widest N slice (most tiles resident) first; for it two row buffers if they fit, else one; rows per step
// aimed at ~32 KiB of input per buffer, at least enough 16-row chunks to give each of the 4 waves a unit, at most 1024 rows
// and 32 KiB of output patch; then as few rows as it takes to fit the LDS budget.
bool fc_rt_plan(FcRtArgs &a, int K, int N) {
    if (K < 1 || N < 1) return false;
    const int KS = (K + 63) / 64, NT = (N + 15) / 16;
    a.K = K, a.N = N, a.KS = KS, a.NT = NT;
    auto xbytes = [&](int R) { return (int)(((long long)R * K + 112 + 15) & ~15ll); };
    for (int NTS = NT; NTS >= 1; --NTS) {
        const int NSL = (NT + NTS - 1) / NTS;
        if (NSL > 1 && (NT + NSL - 1) / NSL != NTS) continue; // (the same slicing as a wider NTS: balanced slices only)
        const long long W = (long long)NTS * KS * 1024;
        const int pw = NSL == 1 ? N : NTS * 16;              // patch bytes per row
        for (int NBUF = 2; NBUF >= 1; --NBUF) {
            int R = std::max(32768 / K / 16 * 16, 16 * ((4 + NTS - 1) / NTS));
            R = std::min(R, 1024);
            while (R > 16 && (long long)R * pw > 32768) R -= 16;
            for (; R >= 16; R -= 16) {
                const long long patch = NSL == 1 ? (((long long)R * N + 32 + 15) & ~15ll) : (long long)R * pw;
                const long long total = W + (long long)NBUF * xbytes(R) + patch;
                if (total > FC_RT_LDS_MAX) continue;
                int TB = std::min(4, NTS);
                while (TB > 1 && (R / 16) * ((NTS + TB - 1) / TB) < 4) TB /= 2;
                a.R = R, a.NTS = NTS, a.NSL = NSL, a.TB = TB, a.NBUF = NBUF;
                a.xoff = (int)W, a.xbytes = xbytes(R), a.poff = (int)(W + (long long)NBUF * xbytes(R)), a.lds = (int)total;
                return true;
            }
        }
    }
    return false;
}

template <int AL, int MG, uint32_t XR4>
static void launch_fc_rt_t(const int8_t *in, int8_t *out, const FcRtArgs &a, long long rows, hipStream_t s) {
    static LaunchState st[FC_RT_LDS_MAX / 1024 + 2]; // occupancy per (device, LDS KiB): asked once, never during a capture
    const int per_cu = prepared(st[(a.lds + 1023) / 1024], fc_rt<AL, MG, XR4>, 256, a.lds);
    // fewer rows per step than planned when the batch would otherwise give fewer than ~1024 steps (a small K plans up to 1024
    // rows: 64 steps for 65 536 rows would leave most CUs idle); the planned LDS layout holds any smaller step
    FcRtArgs b = a;
    b.R = (int)std::min<long long>(a.R, std::max<long long>(16, rows / 1024 / 16 * 16));
    const long long ntiles = (rows + b.R - 1) / b.R;
    long long walkers = std::max(1LL, 256LL * per_cu / a.NSL); // persistent: the resident slice is staged once per workgroup
    walkers = std::min(walkers, ntiles);
    MF_LAUNCH((fc_rt<AL, MG, XR4>), dim3((unsigned)(walkers * a.NSL)), dim3(256), a.lds, s, in, out, b, rows);
}
void launch_fc_rt(const int8_t *in, int8_t *out, const FcRtArgs &a, long long rows, hipStream_t s) {
    if (rows <= 0) return;
    if (a.K % 4 == 0) MF_DISPATCH4(a.magic, a.xr, launch_fc_rt_t, (in, out, a, rows, s), 4)
    else MF_DISPATCH4(a.magic, a.xr, launch_fc_rt_t, (in, out, a, rows, s), 1)
}

// ------------------------------------------------------------------------
// fc_chain -- L consecutive FullyConnected layers (+ a Softmax over one row) in one launch.  The structure is fc_rt's with one
// N slice: every layer's whole image resident in LDS, the step's R input rows staged by LDS-DMA (from the 16-byte-aligned
// ABSOLUTE address below them, so that no pointer needs any alignment), and then per layer: products over the source rows in LDS
// -> the layer's own epilogue (requant_pack4, same bytes as its layer-wise launch) -> its int8 [R][N_l] tile in an LDS activation
// buffer, which is the next layer's operand.  Only the first input and the last output touch HBM.  (The layer step, the Softmax and
// the patch store are k_fc_layer.hpp's: pool_fc_chain, k_pool_fc.hip, runs the same ones behind its pool phase.)
// ------------------------------------------------------------------------
template <int MG, uint32_t XR4>
__global__ __launch_bounds__(256) void fc_chain(const int8_t *__restrict__ in, int8_t *__restrict__ out, FcChainArgs p, long long rows) {
    fc_chain_body<MG, XR4, 0>(in, out, p, rows, F32Edge{});
}

bool fc_chain_plan(FcChainArgs &a) {
    if (a.L < 2 || a.L > FC_CHAIN_MAX) return false;
    long long W = 0;
    int nmax = 0;                                    // widest tensor kept in an activation buffer
    for (int l = 0; l < a.L; ++l) {
        FcChainLayer &y = a.l[l];
        y.KS = (y.K + 63) / 64, y.NT = (y.N + 15) / 16;
        if (l > 0 && y.K != a.l[l - 1].N) return false;
        y.woff = (int)W;
        W += (long long)y.NT * y.KS * 1024;
        if (l < a.L - 1 || a.softmax) nmax = std::max(nmax, y.N);
    }
    const int K0 = a.l[0].K, NL = a.l[a.L - 1].N;
    auto rb = [](long long bytes) { return (int)((bytes + 112 + 15) & ~15ll); }; // (+ the over-read of a 16-byte operand piece)
    // rows per step as fc_rt aims them (~32 KiB of input, >= 64 rows, <= 32 KiB per activation tile).  A chain whose weights leave
    // room for fewer rows than that is not formed: with fewer bytes in flight it was slower than its layers' own launches (784 ->
    // 128 -> 10 at 16 rows per step: 0.140 against 0.066 ms at 65 536 rows), so those layers keep their launches.
    int R0 = std::min(std::max(32768 / K0 / 16 * 16, 64), 1024);
    while (R0 > 16 && ((long long)R0 * std::max(nmax, NL) > 32768)) R0 -= 16;
    for (int NBUF = 2; NBUF >= 1; --NBUF) {
        {
            const int R = R0;
            const long long total = W + (long long)NBUF * rb((long long)R * K0) + 2LL * rb((long long)R * nmax) + (((long long)R * NL + 32 + 15) & ~15ll);
            if (total > FC_RT_LDS_MAX) continue;
            a.R = R, a.NBUF = NBUF;
            a.xoff = (int)W, a.xbytes = rb((long long)R * K0);
            a.aoff = a.xoff + NBUF * a.xbytes, a.abytes = rb((long long)R * nmax);
            a.poff = a.aoff + 2 * a.abytes, a.lds = (int)total;
            for (int l = 0; l < a.L; ++l) {
                FcChainLayer &y = a.l[l];
                y.TB = std::min(4, y.NT);
                while (y.TB > 1 && (R / 16) * ((y.NT + y.TB - 1) / y.TB) < 4) y.TB /= 2;
            }
            return true;
        }
    }
    return false;
}

template <int MG, uint32_t XR4>
static void launch_fc_chain_t(const int8_t *in, int8_t *out, const FcChainArgs &a, long long rows, hipStream_t s) {
    static LaunchState st[FC_RT_LDS_MAX / 1024 + 2];
    const int per_cu = prepared(st[(a.lds + 1023) / 1024], fc_chain<MG, XR4>, 256, a.lds);
    FcChainArgs b = a;
    b.R = (int)std::min<long long>(a.R, std::max<long long>(16, rows / 1024 / 16 * 16)); // (as launch_fc_rt_t)
    const long long ntiles = (rows + b.R - 1) / b.R;
    const long long grid = std::min(ntiles, 256LL * per_cu);
    MF_LAUNCH((fc_chain<MG, XR4>), dim3((unsigned)grid), dim3(256), a.lds, s, in, out, b, rows);
}
void launch_fc_chain(const int8_t *in, int8_t *out, const FcChainArgs &a, long long rows, hipStream_t s) {
    if (rows <= 0) return;
    if (a.xr) {
        if (a.magic == 2) launch_fc_chain_t<2, 0x80808080u>(in, out, a, rows, s);
        else if (a.magic) launch_fc_chain_t<1, 0x80808080u>(in, out, a, rows, s);
        else launch_fc_chain_t<0, 0x80808080u>(in, out, a, rows, s);
    } else {
        if (a.magic == 2) launch_fc_chain_t<2, 0u>(in, out, a, rows, s);
        else if (a.magic) launch_fc_chain_t<1, 0u>(in, out, a, rows, s);
        else launch_fc_chain_t<0, 0u>(in, out, a, rows, s);
    }
}

} // namespace k
} // namespace mf
