// k_pair_band.hip -- ONE DepthwiseConv2D 3x3 SAME (stride 1 or 2) + Conv2D 1x1 pair of ANY image size in one launch, walked in
// row bands: the pairs whose halo'd image + intermediate tensor do not fit chain_rt's LDS budget (k_chain.hip).
//
// (src/ops/depthwise_conv_2d.rs:28-105 + src/ops/conv_2d.rs:28-108; the arithmetic is chain_rt's -- depthwise taps as three
// v_mfma_i32_16x16x64_i8 against block-diagonal weights, the depthwise operator's requantisation, the 1x1 convolution as an MFMA
// product over the pixel matrix, the 1x1 operator's requantisation -- and so is every operand image.  What differs is the step.)
//
//   step      : (image, band) = RB output rows of one image; the bands of an image are consecutive steps, so the workgroups
//               that run neighbouring bands run them at about the same time and the halo rows they share are L2 hits.
//   tile      : the band's (RB - 1) S + 3 input rows, (W + 2) C bytes each + pad, chain_rt's pixel layout and 16-byte-group XOR
//               swizzle (applied on the DMA source).  Input rows S o0 - 1 .. S (o0 + RB - 1) + 1 are one contiguous HBM range.
//   halo      : the left and right halo columns hold the depthwise input zero point from one fill per launch (no DMA writes
//               them).  A tile ROW outside the image is rewritten with the zero point by the staging of EVERY step that has
//               one -- the same routine that issues the DMAs of the rows inside, so a tile row is always written by exactly
//               one of the two: a persistent workgroup that goes from an interior band (rows of real pixels) to a border band
//               never meets a stale row.
//   depthwise : unit = 16 MFMA columns (CY band rows x CX columns, CX the largest power of two <= 16 dividing OW) x one
//               16-channel group; the unit list (channel group, column, row) is cut into 8 contiguous ranges, one per wave.
//               Result -> the depthwise operator's requantisation -> planar MID [C / 16][band pixels padded to 16][16 B].
//   pointwise : a block = TB <= 2 output tiles; a wave fetches its block's operand A (L2 hits) and sweeps the band's 16-pixel
//               chunks (B = ds_read_b128 of the MID planes), SLOTS waves per block; blocks beyond the 8 waves are further
//               passes of the same loop, so N is a loop count.  A lane ends with 4 TB consecutive output bytes of one pixel
//               and stores them to HBM; the ragged last chunk and the rows past OH of the last band are never stored.
//   barriers  : top of step (tile landed, MID free) | depthwise -> pointwise: two per step, both wg_sync().
//   staging   : two tile regions where the plan has room (the next step's tile flies under this whole step), else the next
//               tile is issued behind the depthwise phase's barrier and flies under the pointwise phase.
//
// The kernel's statements are in k_pair_band_body.inc, which pair_band_deep_rt (k_pair_band_deep.hip: 256 < C <= 512) includes too.
#include "k_pair_band_body.hpp"

#include <algorithm>

namespace mf {
namespace k {

template <int KSC, int MG, uint32_t XR4>
__global__ __launch_bounds__(512, KSC == 4 ? 2 : 4) void pair_band_rt(const int8_t *__restrict__ in, int8_t *__restrict__ out, PairBandArgs p, int batch) {
#include "k_pair_band_body.inc"
}

// ------------------------------------------------------------------------
// host: plan + launch
// ------------------------------------------------------------------------
static int pb_lg2(int v) {
    for (int i = 0; i < 31; ++i)
        if ((1 << i) == v) return i;
    return -1;
}
bool pair_band_plan(const ChainGeom &g, PairBandArgs &a) {
    if (g.C % 16 != 0 || g.C < 16 || g.C > 256 || g.N % 16 != 0 || g.N < 16 || g.N > 1024) return false;
    if ((g.S != 1 && g.S != 2) || g.H < 1 || g.W < 1) return false;
    if (g.OH != (g.H + g.S - 1) / g.S || g.OW != (g.W + g.S - 1) / g.S) return false;
    if (g.S == 2 && g.W % 2 != 0) return false;
    // a lower bound of what chain_plan needs at one image per step: a pair below it is chain_rt's (or nobody's), never a band pair
    if ((long long)(g.H + 2) * (g.W + 2) * g.C + (long long)g.OH * g.OW * g.C <= 150 * 1024) return false;
    a.H = g.H, a.W = g.W, a.C = g.C, a.S = g.S, a.OH = g.OH, a.OW = g.OW, a.N = g.N, a.izp4 = g.izp4;
    a.NQ = g.C / 16, a.lgNQ = pb_lg2(a.NQ), a.KS = (g.C + 63) / 64, a.KSC = a.KS <= 1 ? 1 : (a.KS == 2 ? 2 : 4);
    a.swz_sh = 0, a.swz_mask = 0;
    if (a.lgNQ > 0) a.swz_sh = 4 - a.lgNQ, a.swz_mask = a.NQ - 1;
    // depthwise columns: CX divides OW (no overhang along a row); CY band rows fill the 16 columns, and RB is a multiple of CY
    int CX = 1;
    while (CX * 2 <= 16 && g.OW % (CX * 2) == 0) CX *= 2;
    const int CY = 16 / CX;
    a.lgCX = pb_lg2(CX), a.lgCY = pb_lg2(CY);
    const int row0 = (g.W + 2) * g.C;
    int rp = 0, ip = 0; // the row pitch pad when a unit spans CY > 1 rows: chain_plan's bank model (k_chain.hip), one image
    tile_bank_pads(g.H, g.W, g.C, g.S, a.NQ, a.lgCX, a.lgCY, 1, a.swz_sh, a.swz_mask, rp, ip);
    a.ROW = row0 + 16 * rp;
    // output tiles per block: two where N / 16 is even (a lane then stores 8 consecutive bytes), else one
    const int NT = g.N / 16;
    a.TB = NT % 2 == 0 ? 2 : 1, a.NBLK = NT / a.TB;
    a.SLOTS = std::max(1, 8 / a.NBLK), a.NWB = 8 / a.SLOTS;
    auto tile_bytes = [&](int RB) { return (((RB - 1) * g.S + 3) * a.ROW + 255) & ~255; };
    auto mid_bytes = [&](int RB) { return a.NQ * ((RB * g.OW + 15) / 16) * 256; };
    auto total = [&](int RB, bool dbuf) { return (dbuf ? 2 : 1) * tile_bytes(RB) + mid_bytes(RB) + 16; };
    const int cap = (g.OH + CY - 1) / CY * CY;
    auto fit = [&](int budget) { // the largest band (a multiple of CY, at most the image) whose single-tile plan fits
        int rb = 0;
        for (int RB = CY; RB <= cap && total(RB, false) <= budget; RB += CY) rb = RB;
        return rb;
    };
    // Two workgroups per CU are preferred as long as a band keeps at least four rows (a band re-reads two halo rows per S RB
    // it owns, and a step has two barriers to pay for); below that the whole 159 KiB go to one workgroup's band.
    // The four-k-step instances hold 180 registers: one workgroup per CU whatever the LDS, so their band takes the whole budget.
    const int rb_min = std::min(cap, std::max(CY, 4));
    int rb = a.KSC == 4 ? 0 : fit(PAIR_BAND_LDS_HALF);
    int budget = PAIR_BAND_LDS_HALF;
    if (a.KSC == 4 || rb < rb_min) rb = fit(PAIR_BAND_LDS_MAX), budget = PAIR_BAND_LDS_MAX;
    if (rb < CY) return false; // the smallest band does not fit
    // even bands: the same band count with the fewest rows per band
    a.NB = (g.OH + rb - 1) / rb;
    rb = ((g.OH + a.NB - 1) / a.NB + CY - 1) / CY * CY;
    a.RB = rb, a.NB = (g.OH + rb - 1) / rb, a.TR = (rb - 1) * g.S + 3;
    a.dbuf = total(rb, true) <= budget ? 1 : 0;
    a.TILE = tile_bytes(rb);
    a.NCH = (rb * g.OW + 15) / 16, a.PLANE = a.NCH * 256, a.mid_bytes = a.NQ * a.PLANE;
    a.UX = g.OW / CX, a.UY = rb / CY;
    a.tile_off = 0, a.mid_off = (a.dbuf ? 2 : 1) * a.TILE, a.q_off = a.mid_off + a.mid_bytes, a.lds_bytes = a.q_off + 16;
    a.wgs = (a.KSC != 4 && a.lds_bytes <= PAIR_BAND_LDS_HALF) ? 2 : 1;
    return true;
}

bool pair_band_instance(int KSC, int magic) {
    // the v_cvt epilogue (mode 0) exists for four k steps only: below 256 input channels |acc| <= K * 128 * 255 < 2^22 always holds,
    // so an operator is in mode 0 there only when a switch forces it
    return (KSC == 1 || KSC == 2 || KSC == 4) && (magic == 1 || magic == 2 || (magic == 0 && KSC == 4));
}

template <int KSC, int MG, uint32_t XR4>
static void launch_pair_band_t(const int8_t *in, int8_t *out, const PairBandArgs &a, int batch, hipStream_t s) {
    static std::atomic<int> cache[LaunchState::MAX_DEV][161]; // occupancy per (device, LDS size in KiB), as launch_chain_t
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= LaunchState::MAX_DEV) dev = 0;
    std::atomic<int> &slot = cache[dev][(a.lds_bytes + 1023) / 1024];
    int per_cu = slot.load(std::memory_order_relaxed);
    if (per_cu <= 0) {
        (void)hipFuncSetAttribute((const void *)pair_band_rt<KSC, MG, XR4>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pair_band_rt<KSC, MG, XR4>, 512, (size_t)a.lds_bytes) != hipSuccess || per_cu < 1) {
            (void)hipGetLastError();
            per_cu = 1;
        }
        slot.store(per_cu, std::memory_order_relaxed);
    }
    const int nsteps = batch * a.NB;
    const int grid = nsteps < 256 * per_cu ? nsteps : 256 * per_cu;
    PairBandArgs b = a;
    const double hbm = (double)a.H * a.W * a.C + (double)a.OH * a.OW * a.N, rq = (double)a.OH * a.OW * (a.C + a.N);
    b.qcfg = dq_config(nsteps, grid, dq_est_us((double)batch * hbm, (double)batch * rq));
    b.queue = dq_slot(b.queue, b.qlaunch);
    MF_LAUNCH((pair_band_rt<KSC, MG, XR4>), dim3(grid), dim3(512), a.lds_bytes, s, in, out, b, batch);
}

void launch_pair_band(const int8_t *in, int8_t *out, const PairBandArgs &a, int batch, hipStream_t s) {
#define MF_PB_GO(KSC, MG)                                                           \
    do {                                                                            \
        if (a.xr) launch_pair_band_t<KSC, MG, 0x80808080u>(in, out, a, batch, s);   \
        else launch_pair_band_t<KSC, MG, 0u>(in, out, a, batch, s);                 \
    } while (0)
#define MF_PB_MODES(KSC)                  \
    do {                                  \
        if (a.magic == 2) MF_PB_GO(KSC, 2); \
        else MF_PB_GO(KSC, 1);            \
    } while (0)
    if (a.KSC == 1) MF_PB_MODES(1);
    else if (a.KSC == 2) MF_PB_MODES(2);
    else if (a.magic == 0) MF_PB_GO(4, 0);
    else MF_PB_MODES(4);
#undef MF_PB_MODES
#undef MF_PB_GO
}

} // namespace k
} // namespace mf
