// k_side_concat.hip -- a SqueezeNet fire module's 1x1 expand and its CONCATENATION in one launch: the 1x1 Conv2D on the skip edge
// (strides (1,1) or (2,2)) and the CONCATENATION that reads its result beside the running tensor.  The sibling of
// shortcut_add_rt (k_shortcut_add.hip): the convolution's result S exists in registers only.
//
//   rows    : one output pixel (image n, oy, ox) is one row of the product; its operand bytes are the C bytes of T at
//             (n, oy sh, ox sw), loaded straight from HBM in MFMA layout (lane (col, g): 16 bytes of pixel col, k bytes
//             64 ks + 16 g ..).  A k step that hangs over C meets zero weights: K is padded in the operand, not in memory.
//   product : pw_rt's (k_rt.hip): v_mfma_i32_16x16x64_i8, operand A in REGISTERS for the whole launch, TB <= 4 tiles per wave block,
//             NSPLIT = 1, 2 or 4 waves sharing a 16-row chunk, rows of a tile permuted so that a lane ends with 4 TB consecutive
//             output bytes of its pixel.  requant_pack4<MG, XR4> with the convolution's own constants, clamp and host-chosen mode
//             gives the dword the layer-wise Conv2D stores.
//   join    : concat_dword (k_concat.hpp: the text's form, the identity in converter-written files) on that dword with the join's
//             constants for that input, stored into the convolution's channel slice of the output pixel (pitch N + Cb).  The waves
//             of the chunk also move its 16 pixels' Cb bytes of the running tensor -- one contiguous 16 Cb bytes -- through
//             concat_dword into the other slice, in 16-byte words.
// The output overlaps neither T nor the running tensor.  No LDS, no barrier.  All offsets are 64-bit; the pixel decomposition is
// 32-bit where the row count allows it.
#include "k_concat.hpp"

namespace mf {
namespace k {

template <bool B> __device__ __forceinline__ uint4 side_concat_word(v4i w, const ConcatArgs &p) {
    return make_uint4(concat_dword<B>((uint32_t)w.x, p), concat_dword<B>((uint32_t)w.y, p), concat_dword<B>((uint32_t)w.z, p),
                      concat_dword<B>((uint32_t)w.w, p));
}

template <int KSC, int MG, uint32_t XR4>
__global__ __launch_bounds__(256) void side_concat_rt(const int8_t *__restrict__ t_in, const int8_t *__restrict__ run, int8_t *__restrict__ out, SideConcatArgs p, long long nrows) {
    static_assert(MG != 3, "the join's requantisation reads round-to-nearest bytes: modes 0 to 2 only");
    constexpr int U = 2;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int C = p.pw.K, N = p.pw.N, KS = p.pw.KS, TB = p.pw.TB, NSPLIT = p.pw.NSPLIT;
    const int col = lane & 15, g = lane >> 4;
    const int blk = wave % NSPLIT, slot = wave / NSPLIT, SLOTS = 4 / NSPLIT;
    v4i Aw[4][KSC];
    float4 cA[4], cS[4];
    int4 cK[4];
    const int ch0 = blk * 16 * TB + g * 4 * TB; // this lane's first channel
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int ks = 0; ks < KSC; ++ks) {
            Aw[t][ks] = v4i{0, 0, 0, 0};
            if (t < TB && ks < KS) Aw[t][ks] = ((const v4i *)p.pw.wprep)[(((size_t)blk * TB + t) * KS + ks) * 64 + lane];
        }
        const int ch = ch0 + 4 * t;
        const bool live = t < TB && ch < N;
        cA[t] = live ? *(const float4 *)(p.pw.A + ch) : make_float4(0.f, 0.f, 0.f, 0.f);
        cS[t] = live ? *(const float4 *)(p.pw.S + ch) : make_float4(0.f, 0.f, 0.f, 0.f);
        cK[t] = magic4<MG>(live ? *(const int4 *)(p.pw.Kc + ch) : make_int4(0, 0, 0, 0));
    }
    const int OP = p.OH * p.OW;
    const int CR = p.CR, wpr = CR >> 4;                    // the running slice: bytes and 16-byte words per pixel
    const long long pitch = (long long)N + CR;             // output bytes per pixel
    const int conv_off = p.conv_first ? 0 : CR, run_off = p.conv_first ? N : 0;
    const long long img_bytes = (long long)p.H * p.W * C;
    const bool small = nrows <= 0x7fffffffLL;
    const long long nchunks = (nrows + 15) / 16;
    for (long long cb = ((long long)blockIdx.x * SLOTS + slot) * U; cb < nchunks; cb += (long long)gridDim.x * SLOTS * U) {
        v4i B[U][KSC];
        long long row[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            row[u] = (cb + u) * 16 + col;
            const long long r = row[u] < nrows ? row[u] : nrows - 1; // chunks past the end re-read the last row
            long long img;
            int pix;
            if (small) { // (wave-uniform)
                const uint32_t i32 = (uint32_t)r / (uint32_t)OP;
                img = i32, pix = (int)((uint32_t)r - i32 * (uint32_t)OP);
            } else {
                img = r / OP, pix = (int)(r - img * OP);
            }
            const int oy = pix / p.OW, ox = pix - oy * p.OW;
            const int8_t *src = t_in + img * img_bytes + ((long long)(oy * p.sh) * p.W + ox * p.sw) * C;
#pragma unroll
            for (int ks = 0; ks < KSC; ++ks) {
                const int k0 = ks * 64 + g * 16;                     // a k step hanging over C meets zero weights
                if (ks < KS) B[u][ks] = *(const v4i *)(src + (k0 < C ? k0 : 0));
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            // the running slice of this chunk's pixels: 16 Cb contiguous bytes of `run`, word w of them belongs to pixel w / wpr
            const long long row0 = (cb + u) * 16;
            for (int w = blk * 64 + lane; w < 16 * wpr; w += NSPLIT * 64) {
                const int pr = w / wpr, j = w - pr * wpr;
                if (row0 + pr < nrows) {
                    const v4i v = *(const v4i *)(run + row0 * CR + (long long)w * 16);
                    const uint4 y = p.conv_first ? side_concat_word<true>(v, p.cat) : side_concat_word<false>(v, p.cat);
                    st_out_t<false>(out + (row0 + pr) * pitch + run_off + j * 16, y);
                }
            }
            const long long off = row[u] * pitch + conv_off + ch0;
            // the lane's 4 TB bytes of the convolution's slice: one 16-byte or 8-byte word where TB makes them one aligned word (a lane
            // of a four-tile block holds 16 whole channels or none: N is in sixteens), else dwords
            const bool w16 = TB == 4, w8 = TB == 2;
            // (the matrix instructions stay in wave-uniform control flow: only the stores are per lane)
            const bool live = row[u] < nrows && (!w16 || ch0 + 16 <= N);
            uint32_t res[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t < TB) {
                    v4i acc = {cK[t].x, cK[t].y, cK[t].z, cK[t].w};
#pragma unroll
                    for (int ks = 0; ks < KSC; ++ks)
                        if (ks < KS) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(Aw[t][ks], B[u][ks], acc, 0, 0, 0);
                    const uint32_t ws = requant_pack4<MG, XR4>(acc[0], acc[1], acc[2], acc[3], cA[t], cS[t], p.pw.lo_f, p.pw.hi_f);
                    res[t] = p.conv_first ? concat_dword<false>(ws, p.cat) : concat_dword<true>(ws, p.cat);
                }
            }
            if (!live) {
            } else if (w16) {
                st_out_t<false>(out + off, make_uint4(res[0], res[1], res[2], res[3]));
            } else if (w8) {
                st_out_t<false>(out + off, make_uint2(res[0], res[1]));
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t < TB && ch0 + 4 * t < N) *(uint32_t *)(out + off + 4 * t) = res[t];
            }
        }
    }
}

// the class's channel bounds: shortcut_add_rt's for the convolution (C and N in whole sixteens up to four k steps and four wave blocks
// of four tiles), and the running slice in whole sixteens so that every slice starts on a 16-byte boundary
bool side_concat_supported(int C, int N, int CR) { return shortcut_add_supported(C, N) && CR >= 16 && CR % 16 == 0; }

template <int KSC, int MG, uint32_t XR4>
static void launch_side_concat_t(const int8_t *t_in, const int8_t *run, int8_t *out, const SideConcatArgs &a, long long nrows, hipStream_t s) {
    static LaunchState st;
    const int per_cu = prepared(st, side_concat_rt<KSC, MG, XR4>, 256, 0);
    const int SLOTS = 4 / a.pw.NSPLIT;
    const long long nchunks = (nrows + 15) / 16;
    long long grid = (nchunks + SLOTS * 2 - 1) / (SLOTS * 2);
    // persistent, as pw_rt: a workgroup fetches its operand A once; a few waves of workgroups per CU keep the loads deep
    const long long cap = 256LL * per_cu * 2;
    if (grid > cap) grid = cap;
    if (grid < 1) grid = 1;
    MF_LAUNCH((side_concat_rt<KSC, MG, XR4>), dim3((unsigned)grid), dim3(256), 0, s, t_in, run, out, a, nrows);
}
void launch_side_concat(const int8_t *t_in, const int8_t *run, int8_t *out, const SideConcatArgs &a, long long batch, hipStream_t s) {
    const long long nrows = batch * a.OH * a.OW;
    if (a.pw.KS <= 1) MF_DISPATCH4(a.pw.magic, a.pw.xr, launch_side_concat_t, (t_in, run, out, a, nrows, s), 1)
    else if (a.pw.KS == 2) MF_DISPATCH4(a.pw.magic, a.pw.xr, launch_side_concat_t, (t_in, run, out, a, nrows, s), 2)
    else MF_DISPATCH4(a.pw.magic, a.pw.xr, launch_side_concat_t, (t_in, run, out, a, nrows, s), 4)
}

} // namespace k
} // namespace mf
