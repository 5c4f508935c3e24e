// k_block_slice.hip -- ONE inverted-residual block wider than block_band_rt's 256 channels in one launch: Conv2D 1x1 CI -> E (expand),
// DepthwiseConv2D 3x3 SAME (stride 1 or 2) on E, Conv2D 1x1 E -> N (project), 320 <= E <= 1024 in whole sixty-fours.  The E-channel
// tensors never leave the chip, and never exist whole: the step cuts E, not the image.
//
// (src/ops/conv_2d.rs:28-108 + src/ops/depthwise_conv_2d.rs:28-105 + src/ops/conv_2d.rs:28-108; the arithmetic of every member is
// block_band_rt's: an MFMA product, the member's own folded constants, its own requantisation and activation clamp.)
//
// The depthwise is per channel and the project is a sum over E, so a step walks E in SLICES of 64 channels -- one k step of
// v_mfma_i32_16x16x64_i8 -- and only the project's i32 accumulators outlive a slice:
//
//   step      : (image, band) = RB output rows of one image, dealt by DynSteps, staged as block_band_rt stages it (the band's input rows
//               inside the image as they lie in HBM, dma16 from the 16-byte boundary below, guarded dwords over the tensor's last byte).
//   slice s   : expand    input band x the slice's four 16-channel tiles of the expand filter -> a 64-channel tile in chain_rt's pixel
//                         layout and swizzle (block_band_rt's phase with C = 64); the expand's own constants and clamp.
//               depthwise the slice's tile -> a 64-channel MID (four planes), block_band_rt's phase on NQ = 4; its own requantisation.
//               project   MID x the slice's k step of the project filter, ACCUMULATED: wave w owns the same PC x PT rectangle of
//                         (16-pixel chunk, 16-channel tile of N) units in every slice, UPW = PC PT accumulator quads that stay in
//                         registers from slice 0 to the last and are indexed statically.  The filter streams: one k step of the wave's
//                         PT tiles per slice (the image is slice-major), never resident.
//   store     : after the last slice the accumulators take the project's folded constant (the integer sum is exact in any order, so
//               adding it last changes no bit), are requantised once and stored; a lane's dword is stored where its first channel is
//               below N and its pixel inside the band.
//   halo      : block_band_rt's rule.  The expand writes image pixels only; the halo columns hold the depthwise's input zero point from
//               one fill per launch, a tile row outside the image is rewritten by the first slice's expand of every step that has one (no
//               later slice writes it).
//   LDS       : input band | slice tile | slice MID | queue slot -- one slice of tile and MID whatever E is.
//   barriers  : top of step (the input band landed) and, per slice, expand -> depthwise (the tile is complete; every wave has left the
//               previous slice's project, so MID is free) and depthwise -> project (MID complete; the tile is free for the next slice's
//               expand, which therefore needs no barrier of its own in front).  1 + 2 slices per step, all wg_sync().  The next step's
//               input band is issued behind the last slice's expand -> depthwise barrier and flies under that slice's two phases.
//
// The expand and depthwise phases are COPIES of block_band_rt's with the slice's offsets, as that kernel's are of pair_band_rt's.
#include "k_pair_band_body.hpp"

#include <algorithm>

namespace mf {
namespace k {

namespace {
template <int KSI> struct SExW { // expand operands of one 16-channel tile of E
    v4i A[KSI];
    float4 a, s;
    int4 k;
};
typedef v4i v4i_s4 __attribute__((aligned(4))); // a staged pixel's bytes start at any multiple of 4
} // namespace

template <int UPW, int KSI, int MG, uint32_t XR4>
__global__ __launch_bounds__(512, UPW >= 8 ? 2 : 4) void block_slice_rt(const int8_t *__restrict__ in, int8_t *__restrict__ out, BlockSliceArgs bp, int batch) {
    constexpr int NTHR = 512, NWAVE = 8;
    constexpr int PC = block_slice_pc(UPW), PT = block_slice_pt(UPW); // the wave's rectangle: PC chunks x PT output tiles
    constexpr int C = 64, NQ = 4;                                     // the slice: channels, 16-channel groups
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
    const int H = p.H, S = p.S, OH = p.OH, OW = p.OW, N = p.N;
    const int RB = p.RB, NB = p.NB, TR = p.TR, ROW = p.ROW, PLANE = p.PLANE, NCH = p.NCH;
    const int sh = p.swz_sh, mask = p.swz_mask;
    const int CI = bp.CI, ROWB = p.W * CI, NS = bp.NS, NT = bp.NT;
    const uint4 z4 = make_uint4(p.izp4, p.izp4, p.izp4, p.izp4);

    DynSteps dq;
    dq.init(lds + p.q_off, p.queue, tid, p.qcfg);
    // once per launch: every tile byte holds the depthwise input zero point (what stays of it are the halo columns)
    {
        uint4 *dst = (uint4 *)(lds + p.tile_off);
        const int n16 = p.TILE >> 4;
        for (int i = tid; i < n16; i += NTHR) dst[i] = z4;
    }

    // ---- staging of one step's input band: the rows inside the image, as they lie in HBM (block_band_rt's) ----
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

    auto load_ex = [&](int t) { // t: the tile of E, 4 slice + (tile of the slice)
        SExW<KSI> w;
#pragma unroll
        for (int ks = 0; ks < KSI; ++ks) w.A[ks] = ld16(bp.ex_w, (uint32_t)(((t * KSI + ks) * 64 + lane) * 16));
        const uint32_t co = (uint32_t)((16 * t + 4 * g) * 4);
        w.a = ldf4(bp.exA, co), w.s = ldf4(bp.exS, co), w.k = ldi4(bp.exK, co);
        return w;
    };
    // ---- expand phase of slice sl: input band -> the slice's tile ----
    auto expand = [&](int st, int sl) {
        const int img = st / NB, band = st - img * NB;
        int lo_r, hi_r;
        block_band_rows(H, S, RB, TR, band, lo_r, hi_r);
        if (sl == 0)
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
        // one unit = 16 staged pixels x one 16-channel tile; two units of one tile are in flight, as in block_band_rt
        auto product = [&](const SExW<KSI> &we, int t, int c, int &dst) { // dst: the LDS byte of the lane's dword, -1: nothing to store
            const int pr = 16 * c + col;
            const int pp = pr < npix ? pr : npix - 1; // the ragged last chunk computes its last pixel again and stores nothing
            const int rr = (int)__umulhi((uint32_t)pp, bp.wmagic), x1 = pp - rr * W + 1; // tile row (from lo_r), tile column
            dst = pr < npix ? tb + rr * ROW + x1 * C + ((t ^ ((x1 >> sh) & mask)) << 4) : -1;
            v4i acc = {we.k.x, we.k.y, we.k.z, we.k.w};
#pragma unroll
            for (int ks = 0; ks < KSI; ++ks) {
                const v4i B = *(const v4i_s4 *)(lds + ib + pp * CI + 64 * ks);
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
            const SExW<KSI> we = load_ex(NQ * sl + t);
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

    auto load_dw = [&](int q) { // q: the 16-channel group of E
        BDwW w;
#pragma unroll
        for (int ty = 0; ty < 3; ++ty) w.A[ty] = ld16(p.dw_wmm, (uint32_t)(((q * 3 + ty) * 64 + lane) * 16));
        const uint32_t co = (uint32_t)((4 * q + g) * 16);
        w.a = ldf4(p.dwA, co), w.s = ldf4(p.dwS, co), w.k = ldi4(p.dwK, co);
        return w;
    };
    // ---- this wave's contiguous range of the slice's depthwise unit list (channel group, then column, then row: the row varies fastest) ----
    const int UX = p.UX, UY = p.UY, U = NQ * UX * UY;
    const int u0 = (wave * U) >> 3, ucnt = (((wave + 1) * U) >> 3) - u0;
    const int us_q = u0 / (UX * UY), us_r = u0 - us_q * (UX * UY), us_x = us_r / UY, us_y = us_r - us_x * UY;
    // ---- depthwise phase of slice sl: tile -> MID (block_band_rt's on four groups) ----
    auto dw_phase = [&](int sl) {
        const int lgCX = p.lgCX, lgCY = p.lgCY, CXv = 1 << lgCX;
        const int gg = g < 2 ? g : 2; // tap column of this lane group (g == 3 meets zero weights: any readable bytes will do)
        const int cx = col & (CXv - 1), cy = col >> lgCX;
        const int xin0 = cx * S + gg;
        const int tb0 = p.tile_off + cy * S * ROW + xin0 * C;
        const int mb0 = p.mid_off + ((cy * OW + cx) << 4) + 4 * g;
        const int T_UX = CXv * S * C, XSTEP = CXv * S, M_UX = CXv * 16;
        const int TSTEP = (S * ROW) << lgCY, MSTEP = (OW * 16) << lgCY;
        const float lo = p.dw_lo, hi = p.dw_hi;
        int q = us_q, ux = us_x, uy = us_y, n = ucnt;
        while (n > 0) {
            const int seg = min(n, UY - uy);
            const BDwW wd = load_dw(NQ * sl + q);
            const int xin = xin0 + ux * XSTEP;
            int a = tb0 + ux * T_UX + ((q ^ ((xin >> sh) & mask)) << 4) + uy * TSTEP;
            int m = mb0 + q * PLANE + ux * M_UX + uy * MSTEP;
            const bool live = ux * CXv + cx < OW; // (a column grid that hangs over the row: computed, never stored)
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

    // ---- project: the wave's rectangle of units, fixed for the launch: chunks wc + WC i (i < PC), output tiles wt + WT j (j < PT) ----
    const int lgWC = bp.lgWC, WC = 1 << lgWC, WT = NWAVE >> lgWC;
    const int wc = wave & (WC - 1), wt = wave >> lgWC;
    v4i acc[PC][PT];
    auto project = [&](int sl) { // acc += MID x the slice's k step of the wave's tiles
        v4i A[PT];
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const int nt = wt + WT * j;
            A[j] = v4i{0, 0, 0, 0};
            if (nt < NT) A[j] = ld16(p.pw_w, (uint32_t)(((sl * NT + nt) * 64 + lane) * 16));
        }
        const int mb = p.mid_off + g * PLANE + col * 16; // plane g = the slice's channels 16 g .. 16 g + 15 of pixel `col` of a chunk
#pragma unroll
        for (int i = 0; i < PC; ++i) {
            const int c = wc + WC * i;
            if (c < NCH) {
                const v4i B = *(const v4i *)(lds + mb + c * 256);
#pragma unroll
                for (int j = 0; j < PT; ++j) // (a tile past NT meets zero weights and is never stored: no branch per product)
                    acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[j], B, acc[i][j], 0, 0, 0);
            }
        }
    };
    auto store = [&](int step) { // the project's constant, its requantisation, the band's output rows
        const int img = step / NB, band = step - img * NB, o0 = band * RB;
        const int pvalid = min(RB, OH - o0) * OW; // rows past OH of the last band are computed and never stored
        int8_t *obase = out + ((size_t)img * OH + (size_t)o0) * OW * N;
        const float lo = p.pw_lo, hi = p.pw_hi;
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const int nt = wt + WT * j;
            if (nt < NT) {
                const int ch0 = 16 * nt + 4 * g;
                const float4 a = ldf4(p.pwA, (uint32_t)(ch0 * 4)), s = ldf4(p.pwS, (uint32_t)(ch0 * 4));
                const int4 k = ldi4(p.pwK, (uint32_t)(ch0 * 4)); // (the constants are padded to whole tiles)
#pragma unroll
                for (int i = 0; i < PC; ++i) {
                    const int c = wc + WC * i, pix = 16 * c + col;
                    if (c < NCH) {
                        const v4i v = acc[i][j];
                        const uint32_t pk = requant_pack4<MG, XR4>(v[0] + k.x, v[1] + k.y, v[2] + k.z, v[3] + k.w, a, s, lo, hi);
                        // (the ragged last chunk's pixels past the band hold whatever MID's pad held; N % 4 == 0: a dword is inside N or outside)
                        if (pix < pvalid && ch0 < N) st_out(obase + (size_t)pix * N + ch0, pk);
                    }
                }
            }
        }
    };

    const int nsteps = batch * NB;
    if (dq.step < nsteps) stage(dq.step);
    for (; dq.step < nsteps; dq.advance(tid)) {
        const int step = dq.step;
#pragma unroll
        for (int i = 0; i < PC; ++i)
#pragma unroll
            for (int j = 0; j < PT; ++j) acc[i][j] = v4i{0, 0, 0, 0};
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        wg_sync(); // this step's input band is in LDS; every wave has left the previous step (its tile and MID are free)
        dq.top(tid);
        for (int sl = 0; sl < NS; ++sl) {
            expand(step, sl);
            wg_sync(); // the tile is complete; every wave has left the previous slice's project: MID is free
            if (sl == NS - 1 && dq.nxt < nsteps) stage(dq.nxt); // the input band has been read for the last time: the next step's flies under the two phases below
            dw_phase(sl);
            wg_sync(); // MID complete; the tile has been read
            project(sl);
        }
        store(step);
    }
    dq.finish(tid);
}

// ------------------------------------------------------------------------
// host: plan + launch
// ------------------------------------------------------------------------
static int bs_lg2(int v) {
    for (int i = 0; i < 31; ++i)
        if ((1 << i) == v) return i;
    return -1;
}
// the smallest instance whose 8 rectangles cover NCH chunks x NT tiles, and the wave grid (WC waves along the chunks); 0: none does
static int block_slice_cover(int NCH, int NT, int &lgWC) {
    for (int UPW : {1, 2, 4, 8, 16})
        for (int lg = 3; lg >= 0; --lg) // (the most waves along the chunks first: they share a tile's operand)
            if ((block_slice_pc(UPW) << lg) >= NCH && block_slice_pt(UPW) * (8 >> lg) >= NT) {
                lgWC = lg;
                return UPW;
            }
    return 0;
}
// the LDS plan for one choice of the depthwise column grid (CX columns x 16 / CX band rows); false: the smallest band does not fit
static bool block_slice_layout(const ChainGeom &g, int CI, int CX, BlockSliceArgs &bs) {
    PairBandArgs &a = bs.b;
    constexpr int C = 64;
    const int CY = 16 / CX, UX = (g.OW + CX - 1) / CX, NT = (g.N + 15) / 16;
    const int over = (UX * CX - g.OW) * g.S * C; // bytes behind the tile's last row that a column grid hanging over the row reads
    a.lgCX = bs_lg2(CX), a.lgCY = bs_lg2(CY);
    int rp = 0, ip = 0; // the row pitch pad: chain_plan's bank model (k_chain.hip), one image of 64 channels
    tile_bank_pads(g.H, g.W, C, g.S, a.NQ, a.lgCX, a.lgCY, 1, a.swz_sh, a.swz_mask, rp, ip);
    a.ROW = (g.W + 2) * C + 16 * rp;
    auto rows = [&](int RB) { return (RB - 1) * g.S + 3; };
    // block_band_layout's input region: up to 15 bytes in front, and behind the band the last pixel's whole k steps and the DMA's round-up
    auto in_bytes = [&](int RB) { return (rows(RB) * g.W * CI + 15 + 64 * bs.KSI + 16 + 255) & ~255; };
    auto tile_bytes = [&](int RB) { return (rows(RB) * a.ROW + over + 255) & ~255; };
    auto nch = [&](int RB) { return (RB * g.OW + 15) / 16; };
    auto total = [&](int RB) { return in_bytes(RB) + tile_bytes(RB) + a.NQ * nch(RB) * 256 + 16; };
    const int cap = (g.OH + CY - 1) / CY * CY;
    auto fit = [&](int budget) { // the largest band (a multiple of CY, at most the image) that fits the budget and eight rectangles
        int rb = 0, lg = 0;
        for (int RB = CY; RB <= cap && total(RB) <= budget && block_slice_cover(nch(RB), NT, lg); RB += CY) rb = RB;
        return rb;
    };
    // block_band_layout's choice: two workgroups per CU as long as a band keeps max(CY, 4) rows, else the whole budget
    const int rb_min = std::min(cap, std::max(CY, 4));
    int rb = fit(PAIR_BAND_LDS_HALF);
    if (rb < rb_min) rb = fit(PAIR_BAND_LDS_MAX);
    if (rb < CY) return false;
    a.NB = (g.OH + rb - 1) / rb; // even bands: the same band count with the fewest rows per band
    rb = ((g.OH + a.NB - 1) / a.NB + CY - 1) / CY * CY;
    a.RB = rb, a.NB = (g.OH + rb - 1) / rb, a.TR = rows(rb);
    if ((long long)(a.TR * g.W + 16) * g.W >= (1ll << 31)) return false; // (wmagic's exactness: index x W < 2^32)
    bs.wmagic = (uint32_t)(((1ull << 32) + (unsigned)g.W - 1) / (unsigned)g.W);
    a.dbuf = 0;
    a.TILE = tile_bytes(rb);
    a.NCH = nch(rb), a.PLANE = a.NCH * 256, a.mid_bytes = a.NQ * a.PLANE;
    a.UX = UX, a.UY = rb / CY;
    bs.UPW = block_slice_cover(a.NCH, NT, bs.lgWC);
    bs.in_off = 0, bs.in_bytes = in_bytes(rb);
    a.tile_off = bs.in_bytes, a.mid_off = a.tile_off + a.TILE, a.q_off = a.mid_off + a.mid_bytes, a.lds_bytes = a.q_off + 16;
    a.wgs = (a.lds_bytes <= PAIR_BAND_LDS_HALF && bs.UPW < 8) ? 2 : 1; // (from eight units per wave on the accumulators leave no room for 128 registers: one workgroup per CU)
    return true;
}

bool block_slice_plan(const ChainGeom &g, int CI, BlockSliceArgs &bs) {
    PairBandArgs &a = bs.b;
    const int E = g.C;
    if (E % 64 != 0 || E < 320 || E > 1024 || CI % 4 != 0 || CI < 4 || CI > 192 || g.N % 4 != 0 || g.N < 4 || g.N > 320) return false;
    if ((g.S != 1 && g.S != 2) || g.H < 1 || g.W < 2) return false; // (W == 1: ceil(2^32 / W) is no 32-bit multiplier)
    if (g.OH != (g.H + g.S - 1) / g.S || g.OW != (g.W + g.S - 1) / g.S) return false;
    if (g.S == 2 && g.W % 2 != 0) return false;
    // the pair block_band_rt's phases see is ONE SLICE: 64 channels, four groups, one k step
    a.H = g.H, a.W = g.W, a.C = 64, a.S = g.S, a.OH = g.OH, a.OW = g.OW, a.N = g.N, a.izp4 = g.izp4;
    a.NQ = 4, a.lgNQ = 2, a.KS = 1, a.KSC = 1, a.swz_sh = 2, a.swz_mask = 3;
    a.TB = 1, a.NBLK = (g.N + 15) / 16, a.SLOTS = 1, a.NWB = 8;
    bs.E = E, bs.NS = E / 64, bs.NT = a.NBLK, bs.CI = CI, bs.KSI = (CI + 63) / 64;
    // the depthwise column grid: block_band_plan's two candidates, the one with fewer computed pixels first
    int CX = 1, RX = 1;
    while (CX * 2 <= 16 && g.OW % (CX * 2) == 0) CX *= 2;
    while (RX < 16 && RX < g.OW) RX *= 2;
    auto computed = [&](int cx) { return (long long)((g.OW + cx - 1) / cx * cx) * ((g.OH + 16 / cx - 1) / (16 / cx) * (16 / cx)); };
    const int first = (RX != CX && computed(RX) < computed(CX)) ? RX : CX, second = first == CX ? RX : CX;
    if (block_slice_layout(g, CI, first, bs)) return true;
    return second != first && block_slice_layout(g, CI, second, bs);
}

bool block_slice_instance(int UPW, int KSI, int magic) {
    return (UPW == 1 || UPW == 2 || UPW == 4 || UPW == 8 || UPW == 16) && KSI >= 1 && KSI <= 3 && magic >= 0 && magic <= 2;
}

template <int UPW, int KSI, int MG, uint32_t XR4>
static void launch_block_slice_t(const int8_t *in, int8_t *out, const BlockSliceArgs &a, int batch, hipStream_t s) {
    static std::atomic<int> cache[LaunchState::MAX_DEV][161]; // occupancy per (device, LDS size in KiB), as launch_block_band_t
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= LaunchState::MAX_DEV) dev = 0;
    std::atomic<int> &slot = cache[dev][(a.b.lds_bytes + 1023) / 1024];
    int per_cu = slot.load(std::memory_order_relaxed);
    if (per_cu <= 0) {
        (void)hipFuncSetAttribute((const void *)block_slice_rt<UPW, KSI, MG, XR4>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, block_slice_rt<UPW, KSI, MG, XR4>, 512, (size_t)a.b.lds_bytes) != hipSuccess || per_cu < 1) {
            (void)hipGetLastError();
            per_cu = 1;
        }
        slot.store(per_cu, std::memory_order_relaxed);
    }
    const PairBandArgs &p = a.b;
    const int nsteps = batch * p.NB;
    const int grid = nsteps < 256 * per_cu ? nsteps : 256 * per_cu;
    BlockSliceArgs b = a;
    const double hbm = (double)p.H * p.W * a.CI + (double)p.OH * p.OW * p.N, rq = (double)p.H * p.W * a.E + (double)p.OH * p.OW * (a.E + p.N);
    b.b.qcfg = dq_config(nsteps, grid, dq_est_us((double)batch * hbm, (double)batch * rq));
    b.b.queue = dq_slot(b.b.queue, b.b.qlaunch);
    MF_LAUNCH((block_slice_rt<UPW, KSI, MG, XR4>), dim3(grid), dim3(512), p.lds_bytes, s, in, out, b, batch);
}

void launch_block_slice(const int8_t *in, int8_t *out, const BlockSliceArgs &a, int batch, hipStream_t s) {
    const PairBandArgs &p = a.b;
#define MF_BS_GO(UPW, KSI, MG)                                                           \
    do {                                                                                 \
        if (p.xr) launch_block_slice_t<UPW, KSI, MG, 0x80808080u>(in, out, a, batch, s); \
        else launch_block_slice_t<UPW, KSI, MG, 0u>(in, out, a, batch, s);               \
    } while (0)
#define MF_BS_MODES(UPW, KSI)                      \
    do {                                           \
        if (p.magic == 2) MF_BS_GO(UPW, KSI, 2);   \
        else if (p.magic == 1) MF_BS_GO(UPW, KSI, 1); \
        else MF_BS_GO(UPW, KSI, 0);                \
    } while (0)
#define MF_BS_KSI(UPW)                         \
    do {                                       \
        if (a.KSI == 3) MF_BS_MODES(UPW, 3);   \
        else if (a.KSI == 2) MF_BS_MODES(UPW, 2); \
        else MF_BS_MODES(UPW, 1);              \
    } while (0)
    if (a.UPW == 1) MF_BS_KSI(1);
    else if (a.UPW == 2) MF_BS_KSI(2);
    else if (a.UPW == 4) MF_BS_KSI(4);
    else if (a.UPW == 8) MF_BS_KSI(8);
    else MF_BS_KSI(16);
#undef MF_BS_KSI
#undef MF_BS_MODES
#undef MF_BS_GO
}

} // namespace k
} // namespace mf
