// k_block_band.hip -- ONE inverted-residual block in one launch: Conv2D 1x1 CI -> E (expand), DepthwiseConv2D 3x3 SAME (stride 1 or 2)
// on E, Conv2D 1x1 E -> N (project), E wider than both ends.  The E-channel tensors never leave the chip.
//
// (src/ops/conv_2d.rs:28-108 + src/ops/depthwise_conv_2d.rs:28-105 + src/ops/conv_2d.rs:28-108; the arithmetic of every member is
// pair_band_rt's / pw_rt's: an MFMA product, the member's own folded constants, its own requantisation and activation clamp.)
//
// The kernel is pair_band_rt (k_pair_band.hip) with the band's depthwise input tile COMPUTED instead of staged:
//
//   step      : (image, band) = RB output rows of one image, dealt by DynSteps; tile rows = input rows S o0 - 1 .. S (o0 + RB - 1) + 1.
//   stage     : the band's input rows that lie inside the image are ONE contiguous range of the CI-channel tensor.  It is staged as it
//               lies, from the 16-byte boundary at or below its start (`in` is 16-byte aligned, so that boundary is inside the tensor):
//               dma16 for every 16-byte group that ends inside the tensor, guarded dword loads for the one group that may hang over the
//               tensor's last byte.  No alignment class is left out.
//   expand    : unit = 16 staged pixels x one 16-channel tile of E.  B = the pixel's CI bytes per k step (bytes past CI belong to the next
//               pixel and meet zero weights), A = build_pw_rt_reg_weights(CI, E, 1, 1, E / 16).  The unit list (tile, then chunk) is cut
//               into 8 contiguous ranges, one per wave.  A lane ends with 4 consecutive channels of one pixel: the expand's own
//               requantisation, then one dword into the tile at chain_rt's pixel layout and 16-byte-group swizzle.
//   halo      : the expand writes image pixels only.  The two halo columns hold the depthwise's input zero point from one fill per
//               launch; a tile ROW outside the image is rewritten with the zero point by the expand phase of EVERY step that has one
//               (never "expand of padding": the reference pads the depthwise's input, not the expand's).  A persistent workgroup that
//               goes from an interior band to a border band never meets a stale row.
//   depthwise : pair_band_rt's phase on C = E, tile -> MID.  Where the plan's column grid hangs over the row (block_band_plan: an odd OW), the
//               columns past OW read what lies behind the row and are not stored.
//   project   : pair_band_rt's phase, MID -> HBM, with N any multiple of 4: the operand and the constants are padded to whole 16-channel
//               tiles with zeros, a lane's dword is stored only where its first channel is below N.
//   barriers  : top of step (input band landed, MID and tile free) | expand -> depthwise (tile complete, input band read: the next step's
//               band is issued here and flies under the two phases that follow) | depthwise -> project.  Three, all wg_sync().
//
// The depthwise and project phases are COPIES of k_pair_band_body.inc's, not the include: the project's store is masked on N here and the
// step has a third barrier and no tile staging, so the shared text would need switches inside both of its phases and its step loop.
#include "k_pair_band_body.hpp"

#include <algorithm>

namespace mf {
namespace k {

namespace {
template <int KSI> struct BExW { // expand operands of one 16-channel tile of E
    v4i A[KSI];
    float4 a, s;
    int4 k;
};
template <int KSC, int TBM> struct BPrW { // project operands of one block of TBM output tiles
    v4i A[TBM][KSC];
    float4 a[TBM], s[TBM];
    int4 k[TBM];
};
typedef v4i v4i_a4 __attribute__((aligned(4))); // a staged pixel's bytes start at any multiple of 4
} // namespace

template <int KSC, int KSI, int MG, uint32_t XR4>
__global__ __launch_bounds__(512, 4) void block_band_rt(const int8_t *__restrict__ in, int8_t *__restrict__ out, BlockBandArgs bp, int batch) {
    constexpr int NTHR = 512, NWAVE = 8;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const PairBandArgs &p = bp.b;
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
    const int CI = bp.CI, ROWB = p.W * CI;
    const uint4 z4 = make_uint4(p.izp4, p.izp4, p.izp4, p.izp4);

    DynSteps dq;
    dq.init(lds + p.q_off, p.queue, tid, p.qcfg);
    // once per launch: every tile byte holds the depthwise input zero point (what stays of it are the halo columns)
    {
        uint4 *dst = (uint4 *)(lds + p.tile_off);
        const int n16 = p.TILE >> 4;
        for (int i = tid; i < n16; i += NTHR) dst[i] = z4;
    }

    // ---- staging of one step's input band: the rows inside the image, as they lie in HBM ----
    const long long total = (long long)batch * H * ROWB; // bytes of the input tensor: nothing at or past it is read
    auto stage = [&](int st) {
        const int img = st / NB, band = st - img * NB;
        int lo_r, hi_r;
        block_band_rows(H, S, RB, TR, band, lo_r, hi_r);
        const long long gs = ((long long)img * H + (S * band * RB - 1 + lo_r)) * ROWB; // first staged byte; the DMA starts at gs & ~15
        const long long ga = gs & ~15ll;
        const int n16 = (int)(gs - ga + (long long)(hi_r - lo_r) * ROWB + 15) >> 4;
        for (int o = wave * 64; o < n16; o += NTHR) {
            const int i = o + lane;
            if (i < n16) {
                const long long goff = ga + (long long)i * 16;
                if (goff + 16 <= total) {
                    dma16(in + goff, lds + bp.in_off + o * 16);
                } else { // the one group that hangs over the tensor's last byte: its dwords inside the tensor, through registers
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (goff + 4 * j < total) *(uint32_t *)(lds + bp.in_off + i * 16 + 4 * j) = *(const uint32_t *)(in + goff + 4 * j);
                }
            }
        }
    };

    auto load_ex = [&](int t) {
        BExW<KSI> w;
#pragma unroll
        for (int ks = 0; ks < KSI; ++ks) w.A[ks] = ld16(bp.ex_w, (uint32_t)(((t * KSI + ks) * 64 + lane) * 16));
        const uint32_t co = (uint32_t)((16 * t + 4 * g) * 4);
        w.a = ldf4(bp.exA, co), w.s = ldf4(bp.exS, co), w.k = ldi4(bp.exK, co);
        return w;
    };
    // ---- expand phase: input band -> tile ----
    auto expand = [&](int st) {
        const int img = st / NB, band = st - img * NB;
        int lo_r, hi_r;
        block_band_rows(H, S, RB, TR, band, lo_r, hi_r);
        for (int r = wave; r < TR; r += NWAVE) // the rows outside the image: the depthwise's input zero point, every step
            if (r < lo_r || r >= hi_r) {
                uint4 *d = (uint4 *)(lds + p.tile_off + r * ROW);
                for (int i = lane; i < (ROW >> 4); i += 64) d[i] = z4;
            }
        const long long gs = ((long long)img * H + (S * band * RB - 1 + lo_r)) * ROWB;
        const int W = p.W, npix = (hi_r - lo_r) * W, nch = (npix + 15) >> 4;
        const int U = NQ * nch, u0 = (wave * U) >> 3, u1 = ((wave + 1) * U) >> 3;
        int t = u0 / nch, c = u0 - t * nch;
        const int ib = bp.in_off + (int)(gs & 15) + 16 * g;
        const int tb = p.tile_off + lo_r * ROW + 4 * g;
        const float lo = bp.ex_lo, hi = bp.ex_hi;
        // one unit's operand B and where its dword goes; two units of one tile are in flight (their MFMAs back to back, their epilogues
        // interleaved by requant_pack4x2): with two waves per SIMD a single unit's LDS read -> MFMA -> epilogue chain is all latency
        auto product = [&](const BExW<KSI> &we, int t, int c, int &dst) { // dst: the LDS byte of the lane's dword, -1: nothing to store
            const int pr = 16 * c + col;
            const int pp = pr < npix ? pr : npix - 1; // the ragged last chunk computes its last pixel again and stores nothing
            const int rr = (int)__umulhi((uint32_t)pp, bp.wmagic), x1 = pp - rr * W + 1; // tile row (from lo_r), tile column
            dst = pr < npix ? tb + rr * ROW + x1 * C + ((t ^ ((x1 >> sh) & mask)) << 4) : -1;
            v4i acc = {we.k.x, we.k.y, we.k.z, we.k.w};
#pragma unroll
            for (int ks = 0; ks < KSI; ++ks) {
                const v4i B = *(const v4i_a4 *)(lds + ib + pp * CI + 64 * ks);
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(we.A[ks], B, acc, 0, 0, 0);
            }
            return acc;
        };
        auto put = [&](int dst, uint32_t pk) {
            if (dst >= 0) *(uint32_t *)(lds + dst) = pk;
        };
        int u = u0;
        while (u < u1) {
            const int seg = min(u1 - u, nch - c); // the rest of this tile's chunks, or of the wave's range
            const BExW<KSI> we = load_ex(t);
            int k = 0;
            for (; k + 1 < seg; k += 2) {
                int d0, d1;
                const v4i a0 = product(we, t, c + k, d0), a1 = product(we, t, c + k + 1, d1);
                uint32_t p0, p1;
                requant_pack4x2<MG, XR4>(a0, we.a, we.s, a1, we.a, we.s, lo, hi, p0, p1);
                put(d0, p0), put(d1, p1);
            }
            if (k < seg) {
                int d0;
                const v4i a0 = product(we, t, c + k, d0);
                put(d0, requant_pack4<MG, XR4>(a0[0], a0[1], a0[2], a0[3], we.a, we.s, lo, hi));
            }
            u += seg, c = 0, ++t;
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
    constexpr int TBM = KSC == 4 ? 1 : 2; // output tiles per block at most (the plan's TB): one with four k steps, whose operand A is 16 registers a tile
    auto load_pw = [&](int blk) {
        BPrW<KSC, TBM> w;
        const int TB = p.TB, KS = p.KS;
#pragma unroll
        for (int t = 0; t < TBM; ++t) {
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
    // Registers: every instance fits 128, two workgroups per CU wherever the LDS plan leaves room.  The expand phase's operands, B and
    // accumulators come on top of whatever stays live through the step, so less stays than in pair_band_rt: the depthwise operands of
    // the wave's first channel group are fetched at the top of every step, in front of the wait for the input band; the project
    // operands are resident with four k steps only (one tile per block: 28 registers); the two-tile blocks below (32 and 40) are fetched by each step's project phase.
    constexpr bool PWRES = KSC == 4;
    BDwW wd;
    int qcur = -1;

    // ---- depthwise phase: tile -> MID (pair_band_rt's) ----
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
            const bool live = ux * CXv + cx < OW; // (a column grid that hangs over the row, where no CX divides OW: computed, never stored)
            v4i t0 = *(const v4i *)(lds + a), t1 = *(const v4i *)(lds + a + ROW), t2 = *(const v4i *)(lds + a + 2 * ROW);
            for (int k = 0; k < seg; ++k) {
                v4i acc = {wd.k.x, wd.k.y, wd.k.z, wd.k.w};
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(wd.A[0], t0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(wd.A[1], t1, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(wd.A[2], t2, acc, 0, 0, 0);
                a += k + 1 < seg ? TSTEP : 0; // the next unit's taps (the last unit of a segment prefetches itself: no branch)
                t0 = *(const v4i *)(lds + a), t1 = *(const v4i *)(lds + a + ROW), t2 = *(const v4i *)(lds + a + 2 * ROW);
                const uint32_t pk = requant_pack4<MG, XR4>(acc[0], acc[1], acc[2], acc[3], wd.a, wd.s, lo, hi);
                if (live) *(uint32_t *)(lds + m) = pk;
                m += MSTEP;
            }
            n -= seg, uy = 0;
            if (++ux == UX) ux = 0, ++q;
        }
    };

    // ---- project phase: MID -> HBM (pair_band_rt's, the store masked on N) ----
    const int SLOTS = p.SLOTS, NWB = p.NWB, NBLK = p.NBLK;
    const int blk0 = wave / SLOTS, slot = wave - blk0 * SLOTS;
    const bool persist = PWRES && NBLK <= NWB; // one pass and room: a wave's block never changes, its operands are fetched once per launch
    const bool nfull = bp.nfull != 0;
    BPrW<KSC, TBM> wp;
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
            for (int c = slot; c < NCH; c += SLOTS) {
                const int pix = 16 * c + col;
                v4i B[KSC];
#pragma unroll
                for (int ks = 0; ks < KSC; ++ks) B[ks] = *(const v4i *)(lds + poff[ks] + c * 256);
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
                    int8_t *o = obase + (size_t)pix * N + ch0;
                    if (nfull) { // whole tiles: N % 16 == 0, a lane's 4 TB bytes are inside N and 4 TB-byte aligned
                        if constexpr (TB == 2) st_out(o, make_uint2(packed[0], packed[1]));
                        else st_out(o, packed[0]);
                    } else { // the last tile hangs over N: a dword is stored where its first channel is below N (N % 4 == 0)
#pragma unroll
                        for (int t = 0; t < TB; ++t)
                            if (ch0 + 4 * t < N) st_out(o + 4 * t, packed[t]);
                    }
                }
            }
        }
    };

    const int nsteps = batch * NB;
    if (dq.step < nsteps) stage(dq.step);
    for (; dq.step < nsteps; dq.advance(tid)) {
        const int step = dq.step;
        {
            int q0 = us_q < NQ ? us_q : NQ - 1; // (a wave without units fetches the last group's: unconditional, so nothing of the step before stays live)
            asm volatile("" : "+s"(q0)); // (an address the compiler cannot prove loop-invariant: the loads stay here)
            wd = load_dw(q0), qcur = q0;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        wg_sync(); // this step's input band is in LDS; every wave has left the previous step's project phase (MID is free; the tile has been free since its depthwise -> project barrier)
        dq.top(tid);
        expand(step);
        wg_sync(); // the tile is complete; the input band has been read
        if (dq.nxt < nsteps) stage(dq.nxt); // the input region is free: the next step's band flies under the two phases below
        dw_phase(p.tile_off);
        wg_sync(); // MID complete; the tile has been read
        if (TBM == 2 && p.TB == 2) pw_items(step, std::integral_constant<int, TBM>{});
        else pw_items(step, std::integral_constant<int, 1>{});
    }
    dq.finish(tid);
}

// ------------------------------------------------------------------------
// host: plan + launch
// ------------------------------------------------------------------------
static int bb_lg2(int v) {
    for (int i = 0; i < 31; ++i)
        if ((1 << i) == v) return i;
    return -1;
}
// the LDS plan for one choice of the depthwise column grid (CX columns x 16 / CX band rows); false: the smallest band does not fit
static bool block_band_layout(const ChainGeom &g, int CI, int CX, BlockBandArgs &bb) {
    PairBandArgs &a = bb.b;
    const int E = g.C;
    const int CY = 16 / CX, UX = (g.OW + CX - 1) / CX;
    const int over = (UX * CX - g.OW) * g.S * E; // bytes behind the tile's last row that a column grid hanging over the row reads
    a.lgCX = bb_lg2(CX), a.lgCY = bb_lg2(CY);
    const int row0 = (g.W + 2) * E;
    int rp = 0, ip = 0; // the row pitch pad when a unit spans CY > 1 rows: chain_plan's bank model (k_chain.hip), one image
    tile_bank_pads(g.H, g.W, E, g.S, a.NQ, a.lgCX, a.lgCY, 1, a.swz_sh, a.swz_mask, rp, ip);
    a.ROW = row0 + 16 * rp;
    // output tiles per block: two where the (padded) tile count is even and the instance has room (below four k steps), else one
    const int NT = (g.N + 15) / 16;
    a.TB = (NT % 2 == 0 && a.KSC != 4) ? 2 : 1, a.NBLK = NT / a.TB;
    a.SLOTS = std::max(1, 8 / a.NBLK), a.NWB = 8 / a.SLOTS;
    auto rows = [&](int RB) { return (RB - 1) * g.S + 3; };
    // up to 15 bytes in front (the DMA starts at a 16-byte boundary), and behind the band what the last pixel's operand B reads past its CI
    // bytes (64 KSI - CI, met by zero weights) plus the DMA's round-up to 16: no operand read reaches the tile region other waves write
    auto in_bytes = [&](int RB) { return (rows(RB) * g.W * CI + 15 + 64 * bb.KSI + 16 + 255) & ~255; };
    auto tile_bytes = [&](int RB) { return (rows(RB) * a.ROW + over + 255) & ~255; };
    auto mid_bytes = [&](int RB) { return a.NQ * ((RB * g.OW + 15) / 16) * 256; };
    auto total = [&](int RB) { return in_bytes(RB) + tile_bytes(RB) + mid_bytes(RB) + 16; };
    const int cap = (g.OH + CY - 1) / CY * CY;
    auto fit = [&](int budget) { // the largest band (a multiple of CY, at most the image) whose plan fits
        int rb = 0;
        for (int RB = CY; RB <= cap && total(RB) <= budget; RB += CY) rb = RB;
        return rb;
    };
    // pair_band_plan's choice: two workgroups per CU as long as a band keeps max(CY, 4) rows (a band recomputes two halo rows of the
    // expand per S RB rows it owns), else the whole budget.  The four-k-step instances too: unlike pair_band_rt's they fit 128 registers
    const int rb_min = std::min(cap, std::max(CY, 4));
    int rb = fit(PAIR_BAND_LDS_HALF);
    if (rb < rb_min) rb = fit(PAIR_BAND_LDS_MAX);
    if (rb < CY) return false; // the smallest band does not fit
    // even bands: the same band count with the fewest rows per band
    a.NB = (g.OH + rb - 1) / rb;
    rb = ((g.OH + a.NB - 1) / a.NB + CY - 1) / CY * CY;
    a.RB = rb, a.NB = (g.OH + rb - 1) / rb, a.TR = rows(rb);
    if ((long long)(a.TR * g.W + 16) * g.W >= (1ll << 31)) return false; // (wmagic's exactness: index x W < 2^32)
    bb.wmagic = (uint32_t)(((1ull << 32) + (unsigned)g.W - 1) / (unsigned)g.W);
    a.dbuf = 0;
    a.TILE = tile_bytes(rb);
    a.NCH = (rb * g.OW + 15) / 16, a.PLANE = a.NCH * 256, a.mid_bytes = a.NQ * a.PLANE;
    a.UX = UX, a.UY = rb / CY;
    bb.in_off = 0, bb.in_bytes = in_bytes(rb);
    a.tile_off = bb.in_bytes, a.mid_off = a.tile_off + a.TILE, a.q_off = a.mid_off + a.mid_bytes, a.lds_bytes = a.q_off + 16;
    a.wgs = a.lds_bytes <= PAIR_BAND_LDS_HALF ? 2 : 1;
    return true;
}

bool block_band_plan(const ChainGeom &g, int CI, BlockBandArgs &bb) {
    PairBandArgs &a = bb.b;
    const int E = g.C;
    if (E % 16 != 0 || E < 32 || E > 256 || CI % 4 != 0 || CI < 4 || CI > 128 || g.N % 4 != 0 || g.N < 4 || g.N > 256) return false;
    if ((g.S != 1 && g.S != 2) || g.H < 1 || g.W < 2) return false; // (W == 1: ceil(2^32 / W) is no 32-bit multiplier)
    if (g.OH != (g.H + g.S - 1) / g.S || g.OW != (g.W + g.S - 1) / g.S) return false;
    if (g.S == 2 && g.W % 2 != 0) return false;
    a.H = g.H, a.W = g.W, a.C = E, a.S = g.S, a.OH = g.OH, a.OW = g.OW, a.N = g.N, a.izp4 = g.izp4;
    a.NQ = E / 16, a.lgNQ = bb_lg2(a.NQ), a.KS = (E + 63) / 64, a.KSC = a.KS <= 1 ? 1 : (a.KS == 2 ? 2 : 4);
    bb.CI = CI, bb.KSI = (CI + 63) / 64, bb.nfull = g.N % 16 == 0 ? 1 : 0;
    a.swz_sh = 0, a.swz_mask = 0;
    if (a.lgNQ > 0) a.swz_sh = 4 - a.lgNQ, a.swz_mask = a.NQ - 1;
    // depthwise columns.  pair_band_plan's grid: CX the largest power of two that divides OW (no overhang along a row), CY = 16 / CX band
    // rows, RB a multiple of CY.  An odd OW makes that CX 1 and CY 16: a 3 x 3 output computes 16 rows of 3, and sixteen output rows of a
    // wide E at stride 2 are more than the LDS.  The other grid hangs over the row: CX the power of two at or above min(OW, 16),
    // UX = ceil(OW / CX); the columns past OW read whatever lies behind the row (the tile region is extended by what the last row's
    // overhang reaches) and are never stored.  The grid with fewer computed pixels per image wins; one that has no plan loses.
    int CX = 1, RX = 1;
    while (CX * 2 <= 16 && g.OW % (CX * 2) == 0) CX *= 2;
    while (RX < 16 && RX < g.OW) RX *= 2;
    auto computed = [&](int cx) { return (long long)((g.OW + cx - 1) / cx * cx) * ((g.OH + 16 / cx - 1) / (16 / cx) * (16 / cx)); };
    const int first = (RX != CX && computed(RX) < computed(CX)) ? RX : CX, second = first == CX ? RX : CX;
    if (block_band_layout(g, CI, first, bb)) return true;
    return second != first && block_band_layout(g, CI, second, bb);
}

bool block_band_instance(int KSC, int KSI, int magic) {
    // pair_band_instance's modes: the v_cvt epilogue (mode 0) exists for four k steps of E only
    return (KSC == 1 || KSC == 2 || KSC == 4) && (KSI == 1 || KSI == 2) && (magic == 1 || magic == 2 || (magic == 0 && KSC == 4));
}

template <int KSC, int KSI, int MG, uint32_t XR4>
static void launch_block_band_t(const int8_t *in, int8_t *out, const BlockBandArgs &a, int batch, hipStream_t s) {
    static std::atomic<int> cache[LaunchState::MAX_DEV][161]; // occupancy per (device, LDS size in KiB), as launch_pair_band_t
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= LaunchState::MAX_DEV) dev = 0;
    std::atomic<int> &slot = cache[dev][(a.b.lds_bytes + 1023) / 1024];
    int per_cu = slot.load(std::memory_order_relaxed);
    if (per_cu <= 0) {
        (void)hipFuncSetAttribute((const void *)block_band_rt<KSC, KSI, MG, XR4>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, block_band_rt<KSC, KSI, MG, XR4>, 512, (size_t)a.b.lds_bytes) != hipSuccess || per_cu < 1) {
            (void)hipGetLastError();
            per_cu = 1;
        }
        slot.store(per_cu, std::memory_order_relaxed);
    }
    const PairBandArgs &p = a.b;
    const int nsteps = batch * p.NB;
    const int grid = nsteps < 256 * per_cu ? nsteps : 256 * per_cu;
    BlockBandArgs b = a;
    const double hbm = (double)p.H * p.W * a.CI + (double)p.OH * p.OW * p.N, rq = (double)p.H * p.W * p.C + (double)p.OH * p.OW * (p.C + p.N);
    b.b.qcfg = dq_config(nsteps, grid, dq_est_us((double)batch * hbm, (double)batch * rq));
    b.b.queue = dq_slot(b.b.queue, b.b.qlaunch);
    MF_LAUNCH((block_band_rt<KSC, KSI, MG, XR4>), dim3(grid), dim3(512), p.lds_bytes, s, in, out, b, batch);
}

void launch_block_band(const int8_t *in, int8_t *out, const BlockBandArgs &a, int batch, hipStream_t s) {
    const PairBandArgs &p = a.b;
#define MF_BB_GO(KSC, KSI, MG)                                                           \
    do {                                                                                 \
        if (p.xr) launch_block_band_t<KSC, KSI, MG, 0x80808080u>(in, out, a, batch, s);  \
        else launch_block_band_t<KSC, KSI, MG, 0u>(in, out, a, batch, s);                \
    } while (0)
#define MF_BB_KSI(KSC, MG)                    \
    do {                                      \
        if (a.KSI == 2) MF_BB_GO(KSC, 2, MG); \
        else MF_BB_GO(KSC, 1, MG);            \
    } while (0)
#define MF_BB_MODES(KSC)                      \
    do {                                      \
        if (p.magic == 2) MF_BB_KSI(KSC, 2);  \
        else MF_BB_KSI(KSC, 1);               \
    } while (0)
    if (p.KSC == 1) MF_BB_MODES(1);
    else if (p.KSC == 2) MF_BB_MODES(2);
    else if (p.magic == 0) MF_BB_KSI(4, 0);
    else MF_BB_MODES(4);
#undef MF_BB_MODES
#undef MF_BB_KSI
#undef MF_BB_GO
}

} // namespace k
} // namespace mf
