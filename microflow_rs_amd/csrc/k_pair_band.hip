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
#include "k_common.hpp"

#include <algorithm>

namespace mf {
namespace k {

namespace {
struct BDwW { // depthwise operands of one 16-channel group
    v4i A[3];
    float4 a, s;
    int4 k;
};
template <int KSC> struct BPwW { // pointwise operands of one block of (at most two) output tiles
    v4i A[2][KSC];
    float4 a[2], s[2];
    int4 k[2];
};
} // namespace

template <int KSC, int MG, uint32_t XR4>
__global__ __launch_bounds__(512, KSC == 4 ? 2 : 4) void pair_band_rt(const int8_t *__restrict__ in, int8_t *__restrict__ out, PairBandArgs p, int batch) {
    constexpr int NTHR = 512, NWAVE = 8;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, g = lane >> 4;
    typedef __attribute__((address_space(1))) const v4i g_v4i;
    auto ld16 = [](const void *base, uint32_t off) { return *(g_v4i *)((uintptr_t)base + off); };
    auto ldf4 = [&](const void *base, uint32_t off) {
        const v4i v = ld16(base, off);
        return make_float4(__int_as_float(v[0]), __int_as_float(v[1]), __int_as_float(v[2]), __int_as_float(v[3]));
    };
    auto ldi4 = [&](const void *base, uint32_t off) {
        const v4i v = ld16(base, off);
        return magic4<MG>(make_int4(v[0], v[1], v[2], v[3]));
    };
    const int H = p.H, C = p.C, S = p.S, OH = p.OH, OW = p.OW, N = p.N, NQ = p.NQ;
    const int RB = p.RB, NB = p.NB, TR = p.TR, ROW = p.ROW, PLANE = p.PLANE, NCH = p.NCH;
    const int sh = p.swz_sh, mask = p.swz_mask;
    const uint4 z4 = make_uint4(p.izp4, p.izp4, p.izp4, p.izp4);

    DynSteps dq;
    dq.init(lds + p.q_off, p.queue, tid, p.qcfg);
    // once per launch: every tile byte holds the depthwise input zero point (what stays of it are the halo columns)
    {
        uint4 *dst = (uint4 *)(lds + p.tile_off);
        const int n16 = ((p.dbuf ? 2 : 1) * p.TILE) >> 4;
        for (int i = tid; i < n16; i += NTHR) dst[i] = z4;
    }

    // ---- staging of one step's tile: rows inside the image by LDS-DMA, rows outside rewritten with the zero point ----
    auto stage = [&](int st, int buf) {
        const int img = st / NB, band = st - img * NB;
        const int ROWB = p.W * C, ROWCH = ROWB >> 4, lgNQ = p.lgNQ, nqm = NQ - 1;
        const int iy0 = S * band * RB - 1; // input row of tile row 0 (the reference's SAME shift is (K - 1) / 2 for both strides)
        const int8_t *src0 = in + (long)img * ((long)H * ROWB);
        uint8_t *t0 = lds + p.tile_off + buf * p.TILE;
        for (int r = wave; r < TR; r += NWAVE) {
            const int iy = iy0 + r;
            uint8_t *row = t0 + r * ROW;
            if (iy >= 0 && iy < H) {
                const int8_t *src = src0 + (long)iy * ROWB;
                uint8_t *dst = row + C;
                for (int o = 0; o < ROWCH; o += 64) {
                    const int i = o + lane; // 16-byte group i of the row lands at LDS group i; it must hold source group (x, c ^ swz(x))
                    int sidx = i;
                    if (mask != 0) {
                        const int x = i >> lgNQ, c = i & nqm;
                        sidx = (x << lgNQ) + (c ^ (((x + 1) >> sh) & mask));
                    }
                    if (i < ROWCH) dma16(src + sidx * 16, dst + o * 16);
                }
            } else {
                uint4 *d = (uint4 *)row;
                for (int i = lane; i < (ROW >> 4); i += 64) d[i] = z4;
            }
        }
    };

    auto load_dw = [&](int q) {
        BDwW w;
#pragma unroll
        for (int ty = 0; ty < 3; ++ty) w.A[ty] = ld16(p.dw_wmm, (uint32_t)(((q * 3 + ty) * 64 + lane) * 16));
        const uint32_t co = (uint32_t)((4 * q + g) * 16);
        w.a = ldf4(p.dwA, co), w.s = ldf4(p.dwS, co), w.k = ldi4(p.dwK, co);
        return w;
    };
    auto load_pw = [&](int blk) {
        BPwW<KSC> w;
        const int TB = p.TB, KS = p.KS;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int ks = 0; ks < KSC; ++ks) {
                w.A[t][ks] = v4i{0, 0, 0, 0};
                if (t < TB && ks < KS) w.A[t][ks] = ld16(p.pw_w, (uint32_t)((((blk * TB + t) * KS + ks) * 64 + lane) * 16));
            }
            const uint32_t co = (uint32_t)((blk * 16 * TB + g * 4 * TB + 4 * t) * 4);
            if (t < TB) w.a[t] = ldf4(p.pwA, co), w.s[t] = ldf4(p.pwS, co), w.k[t] = ldi4(p.pwK, co);
            else w.a[t] = w.s[t] = make_float4(0.f, 0.f, 0.f, 0.f), w.k[t] = make_int4(0, 0, 0, 0);
        }
        return w;
    };

    // ---- this wave's contiguous range of the depthwise unit list (channel group, then column, then row: the row varies fastest) ----
    const int UX = p.UX, UY = p.UY, U = NQ * UX * UY;
    const int u0 = (wave * U) >> 3, ucnt = (((wave + 1) * U) >> 3) - u0;
    const int us_q = u0 / (UX * UY), us_r = u0 - us_q * (UX * UY), us_x = us_r / UY, us_y = us_r - us_x * UY;
    // The depthwise operands of the wave's first channel group stay in registers for the whole launch -- except with two k steps, where
    // the pointwise phase (two tiles x two k steps of operand A, their constants, B, accumulators) leaves no room for them inside the
    // 128 registers of two workgroups per CU: there they are fetched again at the top of every step, in front of the wait for the tile.
    constexpr bool DWRES = KSC != 2;
    BDwW wd;
    int qcur = -1;
    if (DWRES && ucnt > 0) wd = load_dw(us_q), qcur = us_q;

    // ---- depthwise phase: tile -> MID ----
    auto dw_phase = [&](int tile_base) {
        const int lgCX = p.lgCX, lgCY = p.lgCY, CXv = 1 << lgCX;
        const int gg = g < 2 ? g : 2; // tap column of this lane group (g == 3 meets zero weights: any readable bytes will do)
        const int cx = col & (CXv - 1), cy = col >> lgCX;
        const int xin0 = cx * S + gg;
        const int tb0 = tile_base + cy * S * ROW + xin0 * C;
        const int mb0 = p.mid_off + ((cy * OW + cx) << 4) + 4 * g;
        const int T_UX = CXv * S * C, XSTEP = CXv * S, M_UX = CXv * 16;
        const int TSTEP = (S * ROW) << lgCY, MSTEP = (OW * 16) << lgCY;
        const float lo = p.dw_lo, hi = p.dw_hi;
        int q = us_q, ux = us_x, uy = us_y, n = ucnt;
        while (n > 0) {
            const int seg = min(n, UY - uy);
            if (q != qcur) wd = load_dw(q), qcur = q; // (a wave's range crosses into the next channel group)
            const int xin = xin0 + ux * XSTEP;
            int a = tb0 + ux * T_UX + ((q ^ ((xin >> sh) & mask)) << 4) + uy * TSTEP;
            int m = mb0 + q * PLANE + ux * M_UX + uy * MSTEP;
            v4i t0 = *(const v4i *)(lds + a), t1 = *(const v4i *)(lds + a + ROW), t2 = *(const v4i *)(lds + a + 2 * ROW);
            for (int k = 0; k < seg; ++k) {
                v4i acc = {wd.k.x, wd.k.y, wd.k.z, wd.k.w};
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(wd.A[0], t0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(wd.A[1], t1, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(wd.A[2], t2, acc, 0, 0, 0);
                a += k + 1 < seg ? TSTEP : 0; // the next unit's taps (the last unit of a segment prefetches itself: no branch)
                t0 = *(const v4i *)(lds + a), t1 = *(const v4i *)(lds + a + ROW), t2 = *(const v4i *)(lds + a + 2 * ROW);
                *(uint32_t *)(lds + m) = requant_pack4<MG, XR4>(acc[0], acc[1], acc[2], acc[3], wd.a, wd.s, lo, hi);
                m += MSTEP;
            }
            n -= seg, uy = 0;
            if (++ux == UX) ux = 0, ++q;
        }
    };

    // ---- pointwise phase: MID -> HBM ----
    const int SLOTS = p.SLOTS, NWB = p.NWB, NBLK = p.NBLK;
    const int blk0 = wave / SLOTS, slot = wave - blk0 * SLOTS;
    const bool persist = NBLK <= NWB; // one pass: a wave's block never changes, its operands are fetched once per launch
    BPwW<KSC> wp;
    if (persist && blk0 < NBLK) wp = load_pw(blk0);
    auto pw_items = [&](int step, auto tbc) {
        constexpr int TB = decltype(tbc)::value;
        const int img = step / NB, band = step - img * NB, o0 = band * RB;
        const int pvalid = min(RB, OH - o0) * OW; // rows past OH of the last band are computed and never stored
        int8_t *obase = out + ((size_t)img * OH + (size_t)o0) * OW * N;
        const float lo = p.pw_lo, hi = p.pw_hi;
        int poff[KSC];
#pragma unroll
        for (int ks = 0; ks < KSC; ++ks) {
            const int pl = 4 * ks + g; // plane = 16-channel group; a k step hanging over K meets zero weights
            poff[ks] = p.mid_off + (pl < NQ ? pl : NQ - 1) * PLANE + col * 16;
        }
        for (int b = blk0; b < NBLK; b += NWB) {
            if (!persist) wp = load_pw(b);
            const int ch0 = b * 16 * TB + g * 4 * TB;
            v4i B[KSC], Bn[KSC];
            auto fetch = [&](int c, v4i(&d)[KSC]) {
#pragma unroll
                for (int ks = 0; ks < KSC; ++ks) d[ks] = *(const v4i *)(lds + poff[ks] + c * 256);
            };
            constexpr bool PF = KSC == 1; // operand prefetch of the next chunk while the registers allow it (128 for two workgroups per CU)
            if constexpr (PF) fetch(slot < NCH ? slot : NCH - 1, B);
            for (int c = slot; c < NCH; c += SLOTS) {
                const int pix = 16 * c + col;
                if constexpr (PF) fetch(c + SLOTS < NCH ? c + SLOTS : c, Bn); // the next chunk's operand (the last chunk re-reads itself)
                else fetch(c, B);
                v4i acc[TB];
#pragma unroll
                for (int t = 0; t < TB; ++t) acc[t] = v4i{wp.k[t].x, wp.k[t].y, wp.k[t].z, wp.k[t].w};
#pragma unroll
                for (int ks = 0; ks < KSC; ++ks)
#pragma unroll
                    for (int t = 0; t < TB; ++t) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wp.A[t][ks], B[ks], acc[t], 0, 0, 0);
                uint32_t packed[TB];
#pragma unroll
                for (int t = 0; t < TB; ++t) packed[t] = requant_pack4<MG, XR4>(acc[t][0], acc[t][1], acc[t][2], acc[t][3], wp.a[t], wp.s[t], lo, hi);
                if (pix < pvalid) { // (the ragged last chunk's columns past the band hold whatever MID's pad held)
                    int8_t *o = obase + pix * N + ch0;
                    if constexpr (TB == 2) st_out(o, make_uint2(packed[0], packed[1]));
                    else st_out(o, packed[0]);
                }
                if constexpr (PF) {
#pragma unroll
                    for (int ks = 0; ks < KSC; ++ks) B[ks] = Bn[ks];
                }
            }
        }
    };

    wg_sync(); // the fill is complete before any DMA lands
    const int nsteps = batch * NB;
    if (dq.step < nsteps) stage(dq.step, 0);
    const bool dbuf = p.dbuf != 0;
    int cur = 0;
    for (; dq.step < nsteps; dq.advance(tid)) {
        const int step = dq.step;
        if constexpr (!DWRES) {
            int q0 = us_q < NQ ? us_q : NQ - 1; // (a wave without units fetches the last group's: unconditional, so nothing of the step before stays live)
            asm volatile("" : "+s"(q0)); // (an address the compiler cannot prove loop-invariant: the loads stay here)
            wd = load_dw(q0), qcur = q0;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        wg_sync(); // this step's tile is in LDS; every wave has left the previous step's pointwise phase (MID is free)
        dq.top(tid);
        if (dbuf && dq.nxt < nsteps) stage(dq.nxt, cur ^ 1); // the other region was last read in the previous step's depthwise phase
        dw_phase(p.tile_off + cur * p.TILE);
        wg_sync(); // MID complete; the tile has been read
        if (!dbuf && dq.nxt < nsteps) stage(dq.nxt, 0); // the tile region is free: the next step's rows fly under the pointwise phase
        if (p.TB == 2) pw_items(step, std::integral_constant<int, 2>{});
        else pw_items(step, std::integral_constant<int, 1>{});
        if (dbuf) cur ^= 1;
    }
    dq.finish(tid);
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
    hipLaunchKernelGGL((pair_band_rt<KSC, MG, XR4>), dim3(grid), dim3(512), a.lds_bytes, s, in, out, b, batch);
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
