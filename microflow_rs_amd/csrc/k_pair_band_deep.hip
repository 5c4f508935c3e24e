// k_pair_band_deep.hip -- pair_band_rt (k_pair_band.hip) for 256 < C <= 512 input channels: ONE DepthwiseConv2D 3x3 SAME (stride 1 or 2)
// + Conv2D 1x1 pair in one launch, walked in row bands, with EIGHT k steps of v_mfma_i32_16x16x64_i8 in the 1x1 product.
//
// Arithmetic, operand images, step, tile, halo rule, phases and barriers are pair_band_rt's: the kernel's statements are the same text
// (k_pair_band_body.inc, included below with KSC = 8).  What differs:
//   registers : a wave keeps operand A of its block for a pass over the band's chunks: TB <= 2 tiles x 8 k steps = 64 registers, B is
//               eight ds_read_b128 = 32.  __launch_bounds__(512, 2): 256 registers, one 8-wave workgroup per CU, so the plan always
//               takes the whole LDS budget.  The depthwise operands are not resident: a wave fetches its first channel group's at
//               the top of each step in front of the tile wait, and again where its unit range crosses into the next group.
//   k steps   : KS = 5 .. 7 (C = 272 .. 448) run the same instance with zeroed trailing k steps and clamped MID planes.
//   swizzle   : a pixel of C = 512 is 32 16-byte groups = 512 B, two rows of the 64 banks: the 16 columns of a depthwise unit read the
//               same group q of 16 consecutive pixels, all in one 16-byte bank slot (q & 15).  The group index is XOR-ed with the low
//               four bits of the tile column (swz_sh 0, swz_mask 15): slot (q ^ x) & 15 takes 16 values over 16 consecutive columns,
//               and bit 4 of q stays, so the XOR is a permutation inside each half of the pixel.  Channel-group counts that are not
//               a power of two (20, 24, 28: C = 320, 384, 448) get none, as 96 and 192 channels in pair_band_rt.  The DMA source
//               lane and the tap reads use the same (x >> swz_sh) & swz_mask; only the conflict count depends on it.
//   plan      : no lower size bound (chain_rt never takes C > 256): an image that fits whole is one band, NB = 1.
//   passes    : N = 512 is 16 blocks of two tiles over eight waves = two passes; operand A (16 KiB per wave and pass) is fetched from
//               L2 in every pass of every step.
#include "k_pair_band_body.hpp"

#include <algorithm>

namespace mf {
namespace k {

template <int MG, uint32_t XR4>
__global__ __launch_bounds__(512, 2) void pair_band_deep_rt(const int8_t *__restrict__ in, int8_t *__restrict__ out, PairBandArgs p, int batch) {
    constexpr int KSC = 8;
#include "k_pair_band_body.inc"
}

// ------------------------------------------------------------------------
// host: plan + launch
// ------------------------------------------------------------------------
bool pair_band_deep_plan(const ChainGeom &g, PairBandArgs &a) {
    if (g.C % 16 != 0 || g.C <= 256 || g.C > 512 || g.N % 16 != 0 || g.N < 16 || g.N > 1024) return false;
    if ((g.S != 1 && g.S != 2) || g.H < 1 || g.W < 1) return false;
    if (g.OH != (g.H + g.S - 1) / g.S || g.OW != (g.W + g.S - 1) / g.S) return false;
    if (g.S == 2 && g.W % 2 != 0) return false;
    a.H = g.H, a.W = g.W, a.C = g.C, a.S = g.S, a.OH = g.OH, a.OW = g.OW, a.N = g.N, a.izp4 = g.izp4;
    a.NQ = g.C / 16, a.lgNQ = a.NQ == 32 ? 5 : -1, a.KS = (g.C + 63) / 64, a.KSC = 8;
    // 32 channel groups: the XOR comes from the low four bits of the tile column (see the top of the file); 20, 24, 28: none
    a.swz_sh = 0, a.swz_mask = a.NQ == 32 ? 15 : 0;
    // depthwise columns: CX divides OW (no overhang along a row); CY band rows fill the 16 columns, and RB is a multiple of CY
    int CX = 1, lgCX = 0;
    while (CX * 2 <= 16 && g.OW % (CX * 2) == 0) CX *= 2, ++lgCX;
    const int CY = 16 / CX;
    a.lgCX = lgCX, a.lgCY = 4 - lgCX;
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
    auto total = [&](int RB, bool dbuf) { return (long long)(dbuf ? 2 : 1) * tile_bytes(RB) + mid_bytes(RB) + 16; };
    // 256 registers: one workgroup per CU whatever the LDS, so the band always takes the whole budget.  The largest band (a multiple
    // of CY, at most the image rounded up to CY) whose single-tile plan fits:
    const int cap = (g.OH + CY - 1) / CY * CY;
    int rb = 0;
    for (int RB = CY; RB <= cap && total(RB, false) <= PAIR_BAND_LDS_MAX; RB += CY) rb = RB;
    if (rb < CY) return false; // the smallest band does not fit
    // even bands: the same band count with the fewest rows per band
    a.NB = (g.OH + rb - 1) / rb;
    rb = ((g.OH + a.NB - 1) / a.NB + CY - 1) / CY * CY;
    a.RB = rb, a.NB = (g.OH + rb - 1) / rb, a.TR = (rb - 1) * g.S + 3;
    a.dbuf = total(rb, true) <= PAIR_BAND_LDS_MAX ? 1 : 0;
    a.TILE = tile_bytes(rb);
    a.NCH = (rb * g.OW + 15) / 16, a.PLANE = a.NCH * 256, a.mid_bytes = a.NQ * a.PLANE;
    a.UX = g.OW / CX, a.UY = rb / CY;
    a.tile_off = 0, a.mid_off = (a.dbuf ? 2 : 1) * a.TILE, a.q_off = a.mid_off + a.mid_bytes, a.lds_bytes = a.q_off + 16;
    a.wgs = 1;
    return true;
}

template <int MG, uint32_t XR4>
static void launch_pair_band_deep_t(const int8_t *in, int8_t *out, const PairBandArgs &a, int batch, hipStream_t s) {
    static std::atomic<int> cache[LaunchState::MAX_DEV][161]; // occupancy per (device, LDS size in KiB), as launch_pair_band_t
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= LaunchState::MAX_DEV) dev = 0;
    std::atomic<int> &slot = cache[dev][(a.lds_bytes + 1023) / 1024];
    int per_cu = slot.load(std::memory_order_relaxed);
    if (per_cu <= 0) {
        (void)hipFuncSetAttribute((const void *)pair_band_deep_rt<MG, XR4>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pair_band_deep_rt<MG, XR4>, 512, (size_t)a.lds_bytes) != hipSuccess || per_cu < 1) {
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
    MF_LAUNCH((pair_band_deep_rt<MG, XR4>), dim3(grid), dim3(512), a.lds_bytes, s, in, out, b, batch);
}

void launch_pair_band_deep(const int8_t *in, int8_t *out, const PairBandArgs &a, int batch, hipStream_t s) {
#define MF_PBD_GO(MG)                                                               \
    do {                                                                            \
        if (a.xr) launch_pair_band_deep_t<MG, 0x80808080u>(in, out, a, batch, s);   \
        else launch_pair_band_deep_t<MG, 0u>(in, out, a, batch, s);                 \
    } while (0)
    if (a.magic == 0) MF_PBD_GO(0);
    else if (a.magic == 2) MF_PBD_GO(2);
    else MF_PBD_GO(1);
#undef MF_PBD_GO
}

} // namespace k
} // namespace mf
