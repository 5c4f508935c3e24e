// k_conv1_fc.hip -- a convolution with ONE input channel (DepthwiseConv2D with a depth multiplier, or Conv2D: N filters of KH x KW)
// -> [Reshape] -> FullyConnected over the flattened [OH][OW][N] tensor -> [Softmax] in ONE launch, at any geometry the plan below
// accepts (TensorFlow's keyword-spotting "tiny_conv" family; speech.tflite's own geometry keeps dwc1_fc_softmax, k_dwfc.hip).
// (src/ops/depthwise_conv_2d.rs:27-110 / src/ops/conv_2d.rs:26-110 with one input channel, src/ops/fully_connected.rs:24-82,
//  src/ops/softmax.rs:13-32)
//
// Arithmetic contract, shared device helpers and launch plumbing: k_common.hpp; the Softmax and the output patch: k_fc_layer.hpp.
//
//   columns : 16 IMAGES, in every matrix instruction of the launch.  A step is 16 images, a workgroup walks steps.
//   tiles   : an image is [TROWS][PITCH] bytes in LDS inside a halo of the input zero point (written once per workgroup), so SAME
//             padding is no per-tap test.  The right halo of a row is the left halo of the next one (PITCH = W + the wider of the
//             two, in whole dwords), image column 0 sits on a dword, and staging is 16-byte loads -> dword writes; the next step's
//             first 32 KiB are in registers while this step computes.  PITCH / 4 odd and TILE / 4 = 4 (mod 64): the 64 lanes of an
//             operand read (16 images x 4 filter rows) hit 64 banks.
//   conv    : conv_gemm_rt's C = 1 layout of K: [ky][16 bytes >= KW].  Lane group g of k step ks supplies filter row 4 ks + g of the
//             window: 16 bytes from five ALIGNED dwords + v_alignbyte (a misaligned ds_read_b128 replays: DESIGN 4.10).  Rows are
//             output channels; with N < 16 the idle rows hold the taps of the next PP - 1 pixels along the row, shifted by the
//             stride inside the 16 bytes (KW + (PP - 1) sw <= 16), so one operand read serves PP pixels.  A lane then holds four
//             consecutive channels of one pixel of one image: requant_pack4 in the launch's mode (the bytes of the operator's own
//             launch) and ONE dword into the band buffer.
//   band    : the requantised bytes of BH output rows as [image][k] in NHWC flattening order -- the FullyConnected's operand B.  Two
//             buffers: the waves that are done with band b's products fill band b + 1 while the others still read b (one barrier
//             per band).  Bank phase of the dword writes: BP / 4 = 4 (mod 64).
//   fc      : per band, the 64-byte k steps of the operator's fc_rt image that meet the band's k range [k0, k1), dealt to the waves
//             by absolute k step; accumulators (up to four 16-column tiles + the weight-zero-point row sum as a product with ones)
//             stay in registers across the bands.  A k step that straddles a band edge is visited by both bands, each with the
//             dwords outside its own range zeroed (k0 and k1 are multiples of 4) -- which also covers the last step when
//             K % 64 != 0: stale bytes past K reach neither the weights nor the ones.
//   tail    : the waves' partial sums meet in LDS; wave t finishes tile t (requant_pack4), then fc_chain_softmax and the output patch
//             in aligned 16-byte stores with byte edges.  Nothing past batch x N_fc is written, nothing past batch x H W is read.
#include "k_common.hpp"
#include "k_fc_layer.hpp"

#include <algorithm>

namespace mf {
namespace k {

namespace {
__device__ __forceinline__ uint32_t c1_div(uint32_t d, uint32_t m) { return m ? __umulhi(d, m) : d; } // d / n with m = ceil(2^32 / n) (0: n = 1)
} // namespace

template <int MG, uint32_t XR4>
__global__ __launch_bounds__(256) void conv1_fc_rt(const int8_t *__restrict__ in, int8_t *__restrict__ out, Conv1FcArgs p, long long batch) {
    constexpr int NE = 8; // 16-byte chunks per thread and staging round
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, g = lane >> 4;
    const int H = p.H, W4 = p.W >> 2, HW = p.H * p.W, HW4 = HW >> 2;
    const int N = p.N, OW = p.OW, OH = p.OH, PP = p.PP, NRT = p.NRT, KSC = p.KSC, PITCH = p.PITCH, TILE = p.TILE;
    const int NF = p.fc.N, KS = p.fc.KS, NT = p.fc.NT, BP = p.BP;
    uint8_t *TL = lds + p.toff, *BD = lds + p.boff, *ACT = lds + p.aoff, *PT = lds + p.poff;
    int *part = (int *)(lds + p.qoff), *rsp = part + 4 * NT * 256;
    const uint8_t *WL = lds + p.woff;
    const uint8_t *WG = (const uint8_t *)p.fc.wimg;

    if (p.wres)
        for (int b = wave * 64; b < NT * KS * 64; b += 256) dma16((const int8_t *)WG + (size_t)(b + lane) * 16, lds + p.woff + b * 16);
    for (int i = tid; i < p.tbytes / 16; i += 256) ((uint4 *)TL)[i] = make_uint4(p.izp4, p.izp4, p.izp4, p.izp4);

    // the convolution's operand A and this lane's rows of a tile: (pixel pp, channels cc .. cc + 3)
    v4i Aw[2][4];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) Aw[rt][ks] = ((const v4i *)p.wA)[(rt * 4 + ks) * 64 + lane];
    int pp[2], cc[2];
    bool rowok[2];
    float4 cA[2], cS[2];
    v4i cK[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const int R0 = rt * 16 + 4 * g;
        pp[rt] = PP > 1 ? R0 / N : 0;
        cc[rt] = R0 - pp[rt] * N;
        rowok[rt] = rt < NRT && pp[rt] < PP && cc[rt] < N;
        const int c = rowok[rt] ? cc[rt] : 0;
        cA[rt] = *(const float4 *)(p.A + c), cS[rt] = *(const float4 *)(p.S + c);
        const int4 kc = magic4<MG>(*(const int4 *)(p.Kc + c));
        cK[rt] = v4i{kc.x, kc.y, kc.z, kc.w};
    }

    const long long nblk = (batch + 15) / 16;
    const int NR = (HW + NE * 256 - 1) / (NE * 256); // staging rounds of a step (HW chunks of 16 bytes)
    auto limit_of = [&](long long blk) { // valid bytes of the step's 16 H W (a multiple of 4)
        const long long left = (batch - blk * 16) * (long long)HW;
        return left < 16LL * HW ? (int)left : 16 * HW;
    };
    // every load is issued (a chunk that is not wholly inside the batch reads the batch's first 16 bytes instead and is not used)
    auto load_round = [&](long long blk, int r, u32x4 (&v)[NE]) {
        const int8_t *src = in + blk * 16 * (long long)HW;
        const int limit = limit_of(blk);
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int off = ((r * NE + e) * 256 + tid) * 16;
            v[e] = *(const u32x4 *)(off + 16 <= limit ? src + off : in);
        }
    };
    auto write_round = [&](long long blk, int r, const u32x4 (&v)[NE]) {
        const int8_t *src = in + blk * 16 * (long long)HW;
        const int limit = limit_of(blk);
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int c = (r * NE + e) * 256 + tid, off = c * 16;
            if (off < limit) {
                uint32_t w4[4] = {v[e][0], v[e][1], v[e][2], v[e][3]};
                if (off + 16 > limit) { // the batch ends inside this chunk: its dwords one by one
#pragma unroll
                    for (int q = 0; q < 3; ++q)
                        if (off + 4 * q + 4 <= limit) w4[q] = *(const uint32_t *)(src + off + 4 * q);
                }
                const uint32_t d = 4u * (uint32_t)c;
                int img = (int)c1_div(d, p.m_hw4);
                const uint32_t rr = d - (uint32_t)img * (uint32_t)HW4;
                int row = (int)c1_div(rr, p.m_w4);
                int cw = (int)rr - row * W4;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (off + 4 * q < limit) *(uint32_t *)(TL + img * TILE + (row + p.padt) * PITCH + p.XO + 4 * cw) = w4[q];
                    if (++cw == W4) {
                        cw = 0;
                        if (++row == H) row = 0, ++img;
                    }
                }
            }
        }
    };

    if (blockIdx.x >= nblk) return; // (the launcher starts no such workgroup)
    u32x4 v[NE];
    load_round(blockIdx.x, 0, v);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's DMAs of the weight image have landed ...
    wg_sync();                                       // ... and every other wave's; the halo is written

    const int UPR = (OW + PP - 1) / PP; // units (PP pixels) per output row
    const v4i ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        // ---- the step's 16 images into the tiles (their last readers passed two barriers ago) ----
        write_round(blk, 0, v);
        for (int r = 1; r < NR; ++r) {
            load_round(blk, r, v);
            write_round(blk, r, v);
        }
        if (blk + gridDim.x < nblk) load_round(blk + gridDim.x, 0, v);
        wg_sync();

        v4i facc[4], rs = {0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < 4; ++t) facc[t] = v4i{0, 0, 0, 0};
        for (int b = 0; b < p.NB; ++b) {
            const int oy0 = b * p.BH, bh = min(p.BH, OH - oy0);
            const int k0 = oy0 * OW * N, kb = bh * OW * N; // the band's k range [k0, k0 + kb)
            uint8_t *bd = BD + (b & 1) * 16 * BP + col * BP + CONV1_FC_BAND_FRONT;
            // ---- convolution: units (output row, PP pixels) dealt to the waves ----
            int oyl = 0, oxg = wave;
            while (oxg >= UPR) oxg -= UPR, ++oyl;
            while (oyl < bh) {
                const int ox = oxg * PP;
                const int cb = p.XO - p.padl + ox * p.sw; // byte of a tile row where the unit's windows start
                const uint32_t shb = (uint32_t)cb & 3u;
                const uint8_t *tp = TL + col * TILE + (oy0 + oyl) * p.sh * PITCH + (cb & ~3);
                v4i B[4];
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    if (ks < KSC) {
                        const int ky = min(4 * ks + g, p.KH - 1); // (rows past the filter meet zero weights)
                        const uint32_t *q = (const uint32_t *)(tp + ky * PITCH);
                        const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], d4 = q[4];
                        B[ks] = v4i{(int)__builtin_amdgcn_alignbyte(d1, d0, shb), (int)__builtin_amdgcn_alignbyte(d2, d1, shb),
                                    (int)__builtin_amdgcn_alignbyte(d3, d2, shb), (int)__builtin_amdgcn_alignbyte(d4, d3, shb)};
                    }
                }
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    if (rt < NRT) {
                        v4i acc = cK[rt];
#pragma unroll
                        for (int ks = 0; ks < 4; ++ks)
                            if (ks < KSC) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(Aw[rt][ks], B[ks], acc, 0, 0, 0);
                        if (rowok[rt] && ox + pp[rt] < OW) {
                            const uint32_t d = requant_pack4<MG, XR4>(acc[0], acc[1], acc[2], acc[3], cA[rt], cS[rt], p.lo_f, p.hi_f);
                            *(uint32_t *)(bd + ((oyl * OW + ox + pp[rt]) * N + cc[rt])) = d;
                        }
                    }
                }
                oxg += 4;
                while (oxg >= UPR) oxg -= UPR, ++oyl;
            }
            wg_sync(); // the band is complete
            // ---- FullyConnected: the k steps that meet [k0, k0 + kb), by absolute k step ----
            const int ksa = k0 >> 6, ksb = (k0 + kb + 63) >> 6;
            auto fc_steps = [&](auto resident) { // (two loops, not a selected pointer: that would be a flat load)
                for (int ks = ksa + ((wave - ksa) & 3); ks < ksb; ks += 4) {
                    const int rel = ks * 64 + 16 * g - k0; // this lane's 16 bytes, relative to the band
                    const uint32_t *q = (const uint32_t *)(bd + rel);
                    v4i bv;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const uint32_t dv = q[i];
                        bv[i] = (rel + 4 * i >= 0 && rel + 4 * i < kb) ? (int)dv : 0;
                    }
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        if (t < NT) {
                            const size_t wo = ((size_t)(t * KS + ks) * 64 + lane) * 16;
                            v4i wv;
                            if constexpr (decltype(resident)::value) wv = *(const v4i *)(WL + wo);
                            else wv = *(const v4i *)(WG + wo);
                            facc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wv, bv, facc[t], 0, 0, 0);
                        }
                    }
                    if (p.fc.wzp) rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, bv, rs, 0, 0, 0);
                }
            };
            if (p.wres) fc_steps(std::true_type{});
            else fc_steps(std::false_type{});
        }
        // ---- the waves' sums -> wave t finishes tile t -> Softmax -> patch ----
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < NT) *(v4i *)(part + ((wave * NT + t) * 64 + lane) * 4) = facc[t];
        if (g == 0) rsp[wave * 16 + col] = rs[0];
        wg_sync();
        const long long r0 = blk * 16;
        const int nr = (int)min(16LL, batch - r0);
        const int osh = (int)(((uintptr_t)out + r0 * NF) & 15);
        uint8_t *dst = p.softmax ? ACT : PT + osh;
        if (wave < NT) {
            const int t = wave;
            v4i a = {0, 0, 0, 0};
            int r = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                a += *(const v4i *)(part + ((w * NT + t) * 64 + lane) * 4);
                r += rsp[w * 16 + col];
            }
            const int ch = t * 16 + 4 * g;
            // (mode 0 whatever the convolution's: N_fc bytes per image, and a sum over thousands of k rarely stays below 2^22)
            const int4 kc = *(const int4 *)(p.fc.Kc + ch);
            const int wr = p.fc.wzp * r;
            a[0] += kc.x - wr, a[1] += kc.y - wr, a[2] += kc.z - wr, a[3] += kc.w - wr;
            const float4 A4 = *(const float4 *)(p.fc.A + ch), S4 = {p.fc.S, p.fc.S, p.fc.S, p.fc.S};
            const uint32_t d = requant_pack4<0, XR4>(a[0], a[1], a[2], a[3], A4, S4, p.fc.lo_f, p.fc.hi_f);
            uint8_t *dp = dst + col * NF + ch;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ch + j < NF) dp[j] = (uint8_t)(d >> (8 * j));
        }
        wg_sync();
        if (p.softmax) {
            fc_chain_softmax(p.sm, ACT, PT + osh, nr, NF, tid);
            wg_sync();
        }
        fc_chain_store_patch(out + r0 * NF, PT + osh, (long long)nr * NF, tid);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
namespace {
int up_to_phase(int dwords, int phase) { return dwords + ((phase - dwords) % 64 + 64) % 64; } // the next count = phase (mod 64)
uint32_t div_magic(int n) { return n <= 1 ? 0u : (uint32_t)((0x100000000ull + (uint64_t)n - 1) / (uint64_t)n); }
} // namespace

// Geometry.  Bands: the fewest output rows that give at least 256 bytes of k (four k steps: one per wave), fewer where the LDS needs
// it.  The FullyConnected image stays in LDS where it fits beside the tiles; where it does not (8000 -> 12 beside 49 x 40 tiles), the
// products read it through the L2, 1 KiB per wave and instruction.
bool conv1_fc_plan(Conv1FcArgs &a) {
    if (a.H < 1 || a.W < 4 || a.W % 4 != 0 || a.H * a.W < 16 || a.KH < 1 || a.KH > 16 || a.KW < 1 || a.KW > 16) return false;
    if ((a.sh != 1 && a.sh != 2) || (a.sw != 1 && a.sw != 2)) return false;
    if (a.N % 4 != 0 || a.N < 4 || a.N > 32 || a.wz || !a.finite) return false;
    if (a.pad_same ? (a.OH != (a.H + a.sh - 1) / a.sh || a.OW != (a.W + a.sw - 1) / a.sw)
                   : (a.KH > a.H || a.KW > a.W || a.OH != (a.H - a.KH) / a.sh + 1 || a.OW != (a.W - a.KW) / a.sw + 1))
        return false;
    FcChainLayer &y = a.fc;
    if (y.N < 1 || y.N > 64 || (long long)y.K != (long long)a.OH * a.OW * a.N) return false;
    if (dwfc_supported(a.H, a.W, a.KH, a.KW, a.sh, a.sw, a.OH, a.OW, a.N, y.N)) return false; // dwc1_fc_softmax's own geometry
    y.KS = (y.K + 63) / 64, y.NT = (y.N + 15) / 16, y.TB = 1, y.woff = 0;
    a.padt = a.pad_same ? (a.KH - 1) / 2 : 0, a.padl = a.pad_same ? (a.KW - 1) / 2 : 0;
    const int padb = std::max((a.OH - 1) * a.sh - a.padt + a.KH - a.H, 0), padr = std::max((a.OW - 1) * a.sw - a.padl + a.KW - a.W, 0);
    a.XO = (std::max(a.padl, padr) + 3) & ~3;
    a.PITCH = a.W + a.XO;
    if ((a.PITCH / 4) % 2 == 0) a.PITCH += 4;
    a.TROWS = a.padt + a.H + padb;
    a.TILE = 4 * up_to_phase(a.TROWS * a.PITCH / 4, 4);
    a.PP = 1;
    if (a.N < 16)
        for (int pp = 16 / a.N; pp > 1; pp /= 2)
            if (a.KW + (pp - 1) * a.sw <= 16) {
                a.PP = pp;
                break;
            }
    a.NRT = (a.N * a.PP + 15) / 16, a.KSC = (a.KH + 3) / 4;
    a.m_hw4 = div_magic(a.H * a.W / 4), a.m_w4 = div_magic(a.W / 4);
    a.woff = 0;
    a.tbytes = (16 * a.TILE + 64 + 15) & ~15;
    if (a.tbytes > FC_RT_LDS_MAX) return false;
    const int row_k = a.OW * a.N;
    auto layout = [&](int BH, int wres) {
        a.BH = BH, a.NB = (a.OH + BH - 1) / BH, a.wres = wres;
        a.BP = 4 * up_to_phase((CONV1_FC_BAND_FRONT + BH * row_k + 64) / 4, 4);
        a.toff = wres ? y.NT * y.KS * 1024 : 0;
        a.boff = a.toff + a.tbytes;
        a.qoff = a.boff + 2 * 16 * a.BP;
        a.aoff = a.qoff + 4 * y.NT * 1024 + 256;
        a.poff = a.aoff + ((16 * y.N + 16 + 15) & ~15);
        const long long lds = (long long)a.poff + ((16 * y.N + 32 + 15) & ~15);
        a.lds = (int)std::min<long long>(lds, 1 << 30);
        return lds <= FC_RT_LDS_MAX;
    };
    int BH0 = 1;
    while (BH0 < a.OH && BH0 * row_k < 256) ++BH0;
    for (int wres = 1; wres >= 0; --wres)
        for (int BH = BH0; BH >= 1; --BH)
            if (layout(BH, wres)) return true;
    return false;
}

template <int MG, uint32_t XR4>
static void launch_conv1_fc_t(const int8_t *in, int8_t *out, const Conv1FcArgs &a, long long batch, hipStream_t s) {
    static LaunchState st[FC_RT_LDS_MAX / 1024 + 2]; // occupancy per (device, LDS KiB): asked once, never during a capture
    const int per_cu = prepared(st[(a.lds + 1023) / 1024], conv1_fc_rt<MG, XR4>, 256, a.lds);
    const long long nblk = (batch + 15) / 16;
    const long long grid = std::min(nblk, 256LL * per_cu);
    MF_LAUNCH((conv1_fc_rt<MG, XR4>), dim3((unsigned)grid), dim3(256), a.lds, s, in, out, a, batch);
}
void launch_conv1_fc(const int8_t *in, int8_t *out, const Conv1FcArgs &a, long long batch, hipStream_t s) {
    if (batch <= 0) return;
    if (a.xr) {
        if (a.magic == 2) launch_conv1_fc_t<2, 0x80808080u>(in, out, a, batch, s);
        else if (a.magic) launch_conv1_fc_t<1, 0x80808080u>(in, out, a, batch, s);
        else launch_conv1_fc_t<0, 0x80808080u>(in, out, a, batch, s);
    } else {
        if (a.magic == 2) launch_conv1_fc_t<2, 0u>(in, out, a, batch, s);
        else if (a.magic) launch_conv1_fc_t<1, 0u>(in, out, a, batch, s);
        else launch_conv1_fc_t<0, 0u>(in, out, a, batch, s);
    }
}

} // namespace k
} // namespace mf
