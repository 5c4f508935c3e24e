// k_pair_wz.hip -- ONE DepthwiseConv2D 3x3 SAME (stride 1 or 2) + Conv2D 1x1 pair whose filters carry ZERO POINTS (per tensor or per
// channel, on either member or on both) in one launch, whole images in LDS: chain_rt's single-pair step (k_chain.hip)
// with the two zero-point terms of the reference's arithmetic added.
//
// (src/ops/depthwise_conv_2d.rs:57-105 + src/ops/conv_2d.rs:57-108.  With v' the stored bytes -- the halo holding the input zero
// point -- the reference's accumulator is  acc = dot(v', w) - wzp[c] * sum(v') + Kc[c]  (Kc holds -izp sum(w) + T izp wzp).
// chain_rt computes the first and the last term; the middle one is what this kernel adds, for both operators.)
//
//   step      : G whole images per workgroup of 8 waves (k::chain_plan with one pair: geometry, tile pitches, swizzle, MID, G); the
//               dynamic step queue deals the steps; LDS-DMA staging into the halo'd, swizzled tile, the next step's images under this one.
//   depthwise : unit = 16 MFMA columns x one 16-channel group, three v_mfma_i32_16x16x64_i8 against build_dw_mm_weights' image -- and
//               three more on the SAME B operands against the image of an all-ones filter: row c of that product is the window sum
//               of channel c (lane group 3 meets zeros in both images).  acc -= wzp[c] * sum: one integer multiply-add per value
//               (|sum| <= 9 * 128, |wzp| <= 128: 24-bit operands).  The three filter rows of the ones image are the same 1 KiB, so
//               one copy stays in registers for every channel group.
//   pointwise : item = 16 pixels x one block of TB <= 2 output tiles; one more MFMA per k step on the MID operand the item has
//               read, against a tile of ones that is ZERO beyond C (a padded k step and the clamped MID planes add nothing): every
//               row of that product is the pixel's sum over its C intermediate bytes.  acc[n] -= wzp[n] * rowsum for every tile of
//               the block (|rowsum| <= 256 * 128; the wzp of a padded column is 0).
//   barriers  : top of step | depthwise | pointwise: every one is wg_sync().
//   instances : k steps {1, 2, 4} x the epilogue modes each can reach x {depthwise operands resident, reloaded} x {i8, u8} = 32
//               (pair_wz_instance / launch_pair_wz at the end of the file).
// A member without filter zero points passes zeros.  Accumulator bounds (the epilogue modes) are the operators' own, computed over
// |w - wzp| (ops.hip): the integer arithmetic above is exact modulo 2^32 and ends inside the bound.
#include "k_common.hpp"

#include <algorithm>
#include <atomic>

namespace mf {
namespace k {

namespace {
struct WzDwW {       // depthwise operands of one 16-channel group
    v4i A[3];
    float4 a, s;
    int4 k, z;
};
template <int KSC> struct WzPwW { // pointwise operands of one block of output tiles
    v4i A[2][KSC];
    float4 a[2], s[2];
    int4 k[2], z[2];
};
} // namespace

// RES: the launcher's choice from the plan (ChainArgs::resident): the depthwise operands of every wave stay what they are for the whole
// launch.  The step loop of such an instance contains no vector-memory load at all, so the compiler's wait-count pass puts no vmcnt
// wait inside it and the next step's staging DMAs really fly under this step (chain_rt's RES instances).
template <int KSC, bool RES, int MG, uint32_t XR4>
__global__ __launch_bounds__(512, 2) void pair_wz_rt(const int8_t *__restrict__ in, int8_t *__restrict__ out, PairWzArgs pa, int batch) {
    constexpr int NTHR = 512, NWAVE = 8, TBM = 2;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const ChainArgs &p = pa.c;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    typedef __attribute__((address_space(4))) const ChainPair c_pair;
    c_pair *pairs = (c_pair *)(uintptr_t)p.pairs;
    typedef __attribute__((address_space(1))) const v4i g_v4i;
    auto ld16 = [](const void *base, uint32_t off) { return *(g_v4i *)((uintptr_t)base + off); };
    auto ldf4 = [&](const void *base, uint32_t off) {
        const v4i v = ld16(base, off);
        return make_float4(__int_as_float(v[0]), __int_as_float(v[1]), __int_as_float(v[2]), __int_as_float(v[3]));
    };
    auto ldi4 = [&](const void *base, uint32_t off) {
        const v4i v = ld16(base, off);
        return make_int4(v[0], v[1], v[2], v[3]);
    };
    const int G = p.G;
    const int col = lane & 15, g = lane >> 4;

    DynSteps dq;
    dq.init(lds + p.q_off, p.queue, tid, p.qcfg);
    { // the halo: the tile region(s) hold the depthwise's input zero point; the DMAs only ever write the interior
        const uint32_t z = p.fill_izp4[0];
        uint4 *dst = (uint4 *)(lds + p.fill_off[0]);
        for (int i = tid; i < p.fill_bytes[0] / 16; i += NTHR) dst[i] = make_uint4(z, z, z, z);
    }

    // the pair's record: fetched ONCE and kept in scalar registers (chain_rt's SOLO form)
    struct PR {
        int H, W, C, S, OH, OW, N, NQ, lgNQ, KS, TB, NBLK, ROW, TILE, tile_off, swz_sh, swz_mask, lgCX, lgCY, UG, UY, UX, P, NCH, PLANE, plimit_img;
        float dw_lo, dw_hi, pw_lo, pw_hi;
        int us0, us1, us2, ucnt;
        const int *rtab;
        const void *dw_wmm, *pw_w;
        const float *dwA, *dwS, *pwA, *pwS;
        const int *dwK, *pwK;
    };
    PR cp;
    {
        c_pair &c = pairs[0];
        PR &r = cp;
        r.H = c.H, r.W = c.W, r.C = c.C, r.S = c.S, r.OH = c.OH, r.OW = c.OW, r.N = c.N, r.NQ = c.NQ, r.lgNQ = c.lgNQ, r.KS = c.KS, r.TB = c.TB;
        r.NBLK = c.NBLK, r.ROW = c.ROW, r.TILE = c.TILE, r.tile_off = c.tile_off, r.swz_sh = c.swz_sh, r.swz_mask = c.swz_mask;
        r.lgCX = c.lgCX, r.lgCY = c.lgCY, r.UG = c.UG, r.UY = c.UY, r.UX = c.UX, r.P = c.P, r.NCH = c.NCH, r.PLANE = c.PLANE;
        r.plimit_img = c.plimit_img;
        r.dw_lo = c.dw_lo, r.dw_hi = c.dw_hi, r.pw_lo = c.pw_lo, r.pw_hi = c.pw_hi;
        r.us0 = c.ustart[wave][0], r.us1 = c.ustart[wave][1], r.us2 = c.ustart[wave][2], r.ucnt = c.ucount[wave];
        r.rtab = c.rtab, r.dw_wmm = c.dw_wmm, r.pw_w = c.pw_w, r.dwA = c.dwA, r.dwS = c.dwS, r.pwA = c.pwA, r.pwS = c.pwS, r.dwK = c.dwK, r.pwK = c.pwK;
#define MF_KEEP(x) asm volatile("" : "+s"(x))
        MF_KEEP(r.H); MF_KEEP(r.W); MF_KEEP(r.C); MF_KEEP(r.S); MF_KEEP(r.OH); MF_KEEP(r.OW); MF_KEEP(r.N); MF_KEEP(r.NQ); MF_KEEP(r.lgNQ);
        MF_KEEP(r.KS); MF_KEEP(r.TB); MF_KEEP(r.NBLK); MF_KEEP(r.ROW); MF_KEEP(r.TILE); MF_KEEP(r.tile_off); MF_KEEP(r.swz_sh);
        MF_KEEP(r.swz_mask); MF_KEEP(r.lgCX); MF_KEEP(r.lgCY); MF_KEEP(r.UG); MF_KEEP(r.UY); MF_KEEP(r.UX); MF_KEEP(r.P); MF_KEEP(r.NCH);
        MF_KEEP(r.PLANE); MF_KEEP(r.plimit_img);
        MF_KEEP(r.dw_lo); MF_KEEP(r.dw_hi); MF_KEEP(r.pw_lo); MF_KEEP(r.pw_hi);
        MF_KEEP(r.us0); MF_KEEP(r.us1); MF_KEEP(r.us2); MF_KEEP(r.ucnt); MF_KEEP(r.rtab);
#undef MF_KEEP
    }
    auto load_dw = [&](int q) {
        WzDwW w;
#pragma unroll
        for (int ty = 0; ty < 3; ++ty) w.A[ty] = ld16(cp.dw_wmm, (uint32_t)(((q * 3 + ty) * 64 + lane) * 16));
        const uint32_t co = (uint32_t)((4 * q + g) * 16);
        w.a = ldf4(cp.dwA, co), w.s = ldf4(cp.dwS, co), w.k = magic4<MG>(ldi4(cp.dwK, co)), w.z = ldi4(pa.dw_wzp, co);
        return w;
    };
    auto load_pw = [&]() {
        WzPwW<KSC> w;
        const int TB = cp.TB, KS = cp.KS, blk = wave & (cp.NBLK - 1);
#pragma unroll
        for (int t = 0; t < TBM; ++t) {
#pragma unroll
            for (int ks = 0; ks < KSC; ++ks) {
                w.A[t][ks] = v4i{0, 0, 0, 0};
                if (t < TB && ks < KS) w.A[t][ks] = ld16(cp.pw_w, (uint32_t)((((blk * TB + t) * KS + ks) * 64 + lane) * 16));
            }
            const uint32_t co = (uint32_t)((blk * 16 * TB + g * 4 * TB + 4 * t) * 4);
            if (t < TB) w.a[t] = ldf4(cp.pwA, co), w.s[t] = ldf4(cp.pwS, co), w.k[t] = magic4<MG>(ldi4(cp.pwK, co)), w.z[t] = ldi4(pa.pw_wzp, co);
            else w.a[t] = w.s[t] = make_float4(0.f, 0.f, 0.f, 0.f), w.k[t] = w.z[t] = make_int4(0, 0, 0, 0);
        }
        return w;
    };

    // ---- staging of the pair's input: rows of the step's G images are one contiguous run (chain_rt's generic walk) ----
    auto stage = [&](int st, int buf) {
        const int H = cp.H, ROWB = cp.W * cp.C, ROWCH = ROWB >> 4, IMG = H * ROWB;
        const int lgNQ = cp.lgNQ, nqm = cp.NQ - 1, sh = cp.swz_sh, mask = cp.swz_mask;
        const int nrows = (int)min((long)G, (long)batch - (long)st * G) * H;
        const int8_t *src0 = in + (long)st * G * IMG;
        uint8_t *tile0 = lds + cp.tile_off + buf * p.dbuf_stride + cp.C;
        int gi = 0, y = wave;
        while (y >= H) y -= H, ++gi;
        for (int r = wave; r < nrows; r += NWAVE) {
            const int8_t *src = src0 + (long)r * ROWB;
            uint8_t *dst = tile0 + gi * cp.TILE + (y + 1) * cp.ROW;
            for (int o = 0; o < ROWCH; o += 64) {
                const int i = o + lane; // 16-byte group i of the row lands at LDS group i; it must hold source group (x, c ^ swz(x))
                int sidx = i;
                if (mask != 0) {
                    const int x = i >> lgNQ, c = i & nqm;
                    sidx = (x << lgNQ) + (c ^ (((x + 1) >> sh) & mask));
                }
                if (i < ROWCH) dma16(src + sidx * 16, dst + o * 16);
            }
            y += NWAVE;
            while (y >= H) y -= H, ++gi;
        }
    };

    // ---- depthwise phase: tile -> MID (chain_rt's walk: segments of constant (channel group, unit column)) ----
    // RES (compile time): every wave's units lie inside one channel group (the plan's single_q) -- no reload code in the loop, hence no
    // vmcnt wait there (a wait for an operand reload would also wait for the step-ahead staging DMAs: both count on vmcnt)
    auto dw_phase = [&](WzDwW &wd, const v4i &ones, int tile_base) {
        const int S = cp.S, C = cp.C, ROW = cp.ROW, sh = cp.swz_sh, mask = cp.swz_mask;
        const int lgCX = cp.lgCX, lgCY = cp.lgCY, CXv = 1 << lgCX, CYv = 1 << lgCY;
        const int gg = g < 2 ? g : 2; // tap column of this lane group (g == 3 meets zeros in both images: any readable bytes will do)
        const int cx = col & (CXv - 1), cy = (col >> lgCX) & (CYv - 1), cg = col >> (lgCX + lgCY);
        const int xin0 = cx * S + gg;
        const int tb0 = tile_base + cg * cp.TILE + cy * S * ROW + xin0 * C;
        const int mb0 = p.mid_off + (((cg * cp.OH + cy) * cp.OW + cx) << 4) + 4 * g;
        const int UGY = cp.UG * cp.UY, UX = cp.UX;
        const int T_UX = CXv * S * C, XSTEP = CXv * S, M_UX = CXv * 16, PLANE = cp.PLANE;
        typedef int i32x2 __attribute__((ext_vector_type(2)));
        typedef __attribute__((address_space(4))) const i32x2 c_int2;
        c_int2 *rt = (c_int2 *)(uintptr_t)cp.rtab;
        int q = cp.us0, ux = cp.us1, j = cp.us2;
        int n = cp.ucnt;
        const float lo = cp.dw_lo, hi = cp.dw_hi;
        while (n > 0) {
            const int seg = min(n, UGY - j);
            const int xin = xin0 + ux * XSTEP;
            const int a_seg = tb0 + ux * T_UX + ((q ^ ((xin >> sh) & mask)) << 4);
            const int m_seg = mb0 + q * PLANE + ux * M_UX;
            i32x2 e0 = rt[j], e1 = rt[j + (seg > 1 ? 1 : 0)];
            v4i t0 = *(const v4i *)(lds + a_seg + e0[0]), t1 = *(const v4i *)(lds + a_seg + e0[0] + ROW), t2 = *(const v4i *)(lds + a_seg + e0[0] + 2 * ROW);
            for (int k = 0; k < seg; ++k) {
                const i32x2 e2 = rt[j + (k + 2 < seg ? k + 2 : seg - 1)];
                v4i acc = {wd.k.x, wd.k.y, wd.k.z, wd.k.w}, sum = {0, 0, 0, 0};
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(wd.A[0], t0, acc, 0, 0, 0);
                sum = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, t0, sum, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(wd.A[1], t1, acc, 0, 0, 0);
                sum = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, t1, sum, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(wd.A[2], t2, acc, 0, 0, 0);
                sum = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, t2, sum, 0, 0, 0);
                // the next unit's taps (the last unit of a segment prefetches itself: no branch)
                t0 = *(const v4i *)(lds + a_seg + e1[0]), t1 = *(const v4i *)(lds + a_seg + e1[0] + ROW), t2 = *(const v4i *)(lds + a_seg + e1[0] + 2 * ROW);
                acc[0] -= __mul24(wd.z.x, sum[0]), acc[1] -= __mul24(wd.z.y, sum[1]), acc[2] -= __mul24(wd.z.z, sum[2]), acc[3] -= __mul24(wd.z.w, sum[3]);
                *(uint32_t *)(lds + m_seg + e0[1]) = requant_pack4<MG, XR4>(acc[0], acc[1], acc[2], acc[3], wd.a, wd.s, lo, hi);
                e0 = e1, e1 = e2;
            }
            n -= seg, j = 0;
            if (++ux == UX) {
                ux = 0, ++q;
                if constexpr (!RES) {
                    if (n > 0) wd = load_dw(q); // (the wave's range crosses into the next channel group)
                }
            }
        }
    };

    // ---- pointwise phase: MID -> HBM, instantiated per (tiles per block, k steps) as chain_rt's ----
    auto pw_items = [&](const WzPwW<KSC> &wp, const v4i (&pones)[KSC], int step, int gvalid, auto tbc, auto ksc) {
        constexpr int TB = decltype(tbc)::value, KS = decltype(ksc)::value;
        const int NBLK = cp.NBLK, N = cp.N;
        const int lgB = NBLK == 1 ? 0 : (NBLK == 2 ? 1 : (NBLK == 4 ? 2 : 3));
        const int blk = wave & (NBLK - 1), slot = wave >> lgB, SLOTS = NWAVE >> lgB;
        const int P = cp.P, NCH = cp.NCH, PLANE = cp.PLANE, NQ = cp.NQ;
        const float lo = cp.pw_lo, hi = cp.pw_hi;
        int poff[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int pl = 4 * ks + g; // plane = 16-channel group; a k position beyond C meets zeros in the weights AND in the ones tile
            poff[ks] = p.mid_off + (pl < NQ ? pl : NQ - 1) * PLANE;
        }
        const int ch0 = blk * 16 * TB + g * 4 * TB;
        const int plim = gvalid * cp.plimit_img;
        int8_t *obase = out + (size_t)step * G * cp.plimit_img * N;
        const int voff0 = col * N + ch0;
        constexpr bool PF = KSC <= 2; // operand prefetch of the next chunk while the registers allow it
        v4i B[KS], Bn[KS];
        auto fetch = [&](int px, v4i (&d)[KS]) {
            px = px < P ? px : P - 1;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) d[ks] = *(const v4i *)(lds + poff[ks] + px * 16);
        };
        fetch(16 * slot + col, B);
        for (int c = slot; c < NCH; c += SLOTS) {
            const int pix = 16 * c + col;
            if constexpr (PF) fetch(pix + 16 * SLOTS, Bn); // the next chunk's operand (the last chunk re-reads pixel P - 1)
            else if (c != slot) fetch(pix, B);
            v4i acc[TB], rs = {0, 0, 0, 0};
#pragma unroll
            for (int t = 0; t < TB; ++t) acc[t] = v4i{wp.k[t].x, wp.k[t].y, wp.k[t].z, wp.k[t].w};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
                for (int t = 0; t < TB; ++t) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wp.A[t][ks], B[ks], acc[t], 0, 0, 0);
                rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(pones[ks], B[ks], rs, 0, 0, 0); // every row: the pixel's sum over its C bytes
            }
            const int rowsum = rs[0];
#pragma unroll
            for (int t = 0; t < TB; ++t)
                acc[t][0] -= __mul24(wp.z[t].x, rowsum), acc[t][1] -= __mul24(wp.z[t].y, rowsum), acc[t][2] -= __mul24(wp.z[t].z, rowsum), acc[t][3] -= __mul24(wp.z[t].w, rowsum);
            uint32_t packed[TB];
            if constexpr (TB == 2) requant_pack4x2<MG, XR4>(acc[0], wp.a[0], wp.s[0], acc[1], wp.a[1], wp.s[1], lo, hi, packed[0], packed[1]);
            else packed[0] = requant_pack4<MG, XR4>(acc[0][0], acc[0][1], acc[0][2], acc[0][3], wp.a[0], wp.s[0], lo, hi);
            if (pix < plim) {
                int8_t *o = obase + voff0 + c * 16 * N;
                if constexpr (TB == 2) st_out(o, make_uint2(packed[0], packed[1]));
                else st_out(o, packed[0]);
            }
            if constexpr (PF) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) B[ks] = Bn[ks];
            }
        }
    };
    auto pw_phase = [&](const WzPwW<KSC> &wp, const v4i (&pones)[KSC], int step, int gvalid) {
        using std::integral_constant;
        const int TB = cp.TB, KS = cp.KS;
        bool done = false;
        auto go = [&](auto tbc, auto ksc) {
            if (done || TB != decltype(tbc)::value || KS != decltype(ksc)::value) return;
            done = true;
            pw_items(wp, pones, step, gvalid, tbc, ksc);
        };
        auto go_tb = [&](auto ksc) {
            go(integral_constant<int, 1>{}, ksc);
            go(integral_constant<int, 2>{}, ksc);
        };
        go_tb(integral_constant<int, 1>{});
        if constexpr (KSC >= 2) go_tb(integral_constant<int, 2>{});
        if constexpr (KSC >= 4) {
            go_tb(integral_constant<int, 3>{});
            go_tb(integral_constant<int, 4>{});
        }
    };

    wg_sync(); // the halo fill is complete before any DMA lands
    const int nsteps = (batch + G - 1) / G;
    if (dq.step < nsteps) stage(dq.step, 0);
    // the operands stay in registers for the whole launch: the 1x1's, both ones images, and the depthwise's of the wave's first channel group
    const v4i dones = ld16(pa.dw_ones, (uint32_t)(lane * 16));
    v4i pones[KSC];
#pragma unroll
    for (int ks = 0; ks < KSC; ++ks) {
        pones[ks] = v4i{0, 0, 0, 0};
        if (ks < cp.KS) pones[ks] = ld16(pa.pw_ones, (uint32_t)((ks * 64 + lane) * 16));
    }
    WzDwW wd = load_dw(cp.us0);
    const WzPwW<KSC> wp = load_pw();
    const bool dbuf = p.dbuf != 0;
    int cur = 0;
    for (; dq.step < nsteps; dq.advance(tid)) {
        const int step = dq.step;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this step's staging DMAs (and the last step's stores)
        wg_sync(); // this step's images are in the tile; every wave has left the previous step's pointwise phase (MID is free)
        dq.top(tid);
        if (dbuf && dq.nxt < nsteps) stage(dq.nxt, cur ^ 1); // double buffered: the next step's images have this whole step to land
        const int gvalid = min(G, batch - step * G);
        dw_phase(wd, dones, cp.tile_off + cur * p.dbuf_stride);
        wg_sync(); // MID complete; the tile has been read
        if (!dbuf && dq.nxt < nsteps) stage(dq.nxt, 0); // the tile is free: the next step's images fly under the pointwise phase
        if constexpr (!RES) wd = load_dw(cp.us0); // (the wave's first channel group again, under the pointwise phase)
        pw_phase(wp, pones, step, gvalid);
        if (dbuf) cur ^= 1;
    }
    dq.finish(tid);
}

// ------------------------------------------------------------------------
// host: launch
// ------------------------------------------------------------------------
bool pair_wz_instance(int KSC, int magic) {
    // One k step (C <= 64): |acc| <= 64 * 255 * 255 < 2^22 whatever the zero points, so mode 0 appears there only when a switch forces it;
    // from two k steps on (C >= 80) full-range weights against a zero point at the other end of the range reach it.
    return (KSC == 1 && (magic == 1 || magic == 2)) || ((KSC == 2 || KSC == 4) && magic >= 0 && magic <= 2);
}

// chain_plan cuts the depthwise unit list for the workgroup size ITS kernel would use (8 or 16 waves); pair_wz_rt always has 8
void pair_wz_split(ChainPair &c) {
    const int U = c.NQ * c.NU, NW = 8;
    c.single_q = 1;
    for (int w = 0; w < 16; ++w) {
        const int u0 = w < NW ? (int)((long)w * U / NW) : U, u1 = w < NW ? (int)((long)(w + 1) * U / NW) : U;
        const int q = u0 < U ? u0 / c.NU : 0, r = u0 < U ? u0 % c.NU : 0;
        c.ustart[w][0] = q, c.ustart[w][1] = r / (c.UG * c.UY), c.ustart[w][2] = r % (c.UG * c.UY), c.ustart[w][3] = 0;
        c.ucount[w] = u1 - u0;
        if (u1 > u0 && (u1 - 1) / c.NU != q) c.single_q = 0;
    }
}

template <int KSC, bool RES, int MG, uint32_t XR4>
static void launch_pair_wz_t(const int8_t *in, int8_t *out, const PairWzArgs &a, int batch, hipStream_t s) {
    static std::atomic<int> cache[LaunchState::MAX_DEV][161]; // occupancy per (device, LDS size in KiB), as launch_chain_t
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= LaunchState::MAX_DEV) dev = 0;
    std::atomic<int> &slot = cache[dev][(a.c.lds_bytes + 1023) / 1024];
    int per_cu = slot.load(std::memory_order_relaxed);
    if (per_cu <= 0) {
        (void)hipFuncSetAttribute((const void *)pair_wz_rt<KSC, RES, MG, XR4>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pair_wz_rt<KSC, RES, MG, XR4>, 512, (size_t)a.c.lds_bytes) != hipSuccess || per_cu < 1) {
            (void)hipGetLastError();
            per_cu = 1;
        }
        slot.store(per_cu, std::memory_order_relaxed);
    }
    const int nsteps = (batch + a.c.G - 1) / a.c.G;
    const int grid = nsteps < 256 * per_cu ? nsteps : 256 * per_cu;
    PairWzArgs b = a;
    b.c.qcfg = dq_config(nsteps, grid, dq_est_us((double)batch * a.c.hbm_bytes, (double)batch * a.c.requant_bytes));
    b.c.queue = dq_slot(b.c.queue, b.c.qlaunch);
    MF_LAUNCH((pair_wz_rt<KSC, RES, MG, XR4>), dim3(grid), dim3(512), a.c.lds_bytes, s, in, out, b, batch);
}

void launch_pair_wz(const int8_t *in, int8_t *out, const PairWzArgs &a, int batch, hipStream_t s) {
#define MF_PWZ_GO2(KSC, RE, MG)                                                       \
    do {                                                                              \
        if (a.c.xr) launch_pair_wz_t<KSC, RE, MG, 0x80808080u>(in, out, a, batch, s); \
        else launch_pair_wz_t<KSC, RE, MG, 0u>(in, out, a, batch, s);                 \
    } while (0)
#define MF_PWZ_GO(KSC, MG)                         \
    do {                                           \
        if (a.c.resident) MF_PWZ_GO2(KSC, true, MG); \
        else MF_PWZ_GO2(KSC, false, MG);           \
    } while (0)
#define MF_PWZ_MODES(KSC)                        \
    do {                                         \
        if (a.c.magic == 2) MF_PWZ_GO(KSC, 2);   \
        else if (a.c.magic == 1) MF_PWZ_GO(KSC, 1); \
        else MF_PWZ_GO(KSC, 0);                  \
    } while (0)
    if (a.c.KSC == 1) {
        if (a.c.magic == 2) MF_PWZ_GO(1, 2);
        else MF_PWZ_GO(1, 1);
    } else if (a.c.KSC == 2) MF_PWZ_MODES(2);
    else MF_PWZ_MODES(4);
#undef MF_PWZ_MODES
#undef MF_PWZ_GO
#undef MF_PWZ_GO2
}

} // namespace k
} // namespace mf
