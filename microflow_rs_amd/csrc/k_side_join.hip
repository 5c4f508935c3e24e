// k_side_join.hip -- a 1x1 Conv2D on a skip edge (strides (1,1) or (2,2)) and the join that reads its result beside the running tensor,
// in one launch: a ResNet projection shortcut and its ADD (shortcut_add_rt), a SqueezeNet fire module's 1x1 expand and its
// CONCATENATION (side_concat_rt).  ONE kernel body, side_join_rt; the join is a policy.  The convolution's result S exists
// in registers only.
//
//   rows    : one output pixel (image n, oy, ox) is one row of the product; its operand bytes are the C bytes of T at
//             (n, oy sh, ox sw) -- a 1x1 filter has no out-of-bounds tap under SAME or VALID -- loaded straight from HBM in MFMA
//             layout (lane (col, g): 16 bytes of pixel col, k bytes 64 ks + 16 g ..).  A k step that hangs over C meets zero
//             weights: K is padded in the operand (wimage.cpp build_pw_rt_reg_weights), not in memory.
//   product : pw_rt's (k_rt.hip): v_mfma_i32_16x16x64_i8, operand A in REGISTERS for the whole launch, TB <= 4 tiles per wave block,
//             NSPLIT = 1, 2 or 4 waves sharing a 16-row chunk, rows of a tile permuted so that a lane ends with 4 TB consecutive
//             output bytes of its pixel.  The accumulator starts at Kc; requant_pack4<MG, XR4> with the convolution's own constants,
//             clamp and host-chosen mode gives the dword the layer-wise Conv2D stores.
//   join    : what the policy does with that dword and where it goes --
//             AddJoin    : add_dword (k_add.hpp: the text's form) on it and the running tensor's dword at the output position, in the
//                          file's operand order (conv_first), stored at pitch N.  out may be exactly the running tensor (a lane reads
//                          its bytes before it writes them); it must not overlap T.
//             ConcatJoin : concat_dword (k_concat.hpp: the text's form, the identity in converter-written files) with the join's
//                          constants for that input, stored into the convolution's channel slice of the output pixel (pitch N + CR).
//                          The waves of the chunk also move its 16 pixels' CR bytes of the running tensor -- one contiguous 16 CR
//                          bytes -- through concat_dword into the other slice, in 16-byte words.  The output overlaps neither T nor
//                          the running tensor.
// No LDS, no barrier.  All offsets are 64-bit; the pixel decomposition is 32-bit where the row count allows it.
#include "k_add.hpp"
#include "k_concat.hpp"

namespace mf {
namespace k {

// What a lane knows of its chunk when the join's turn comes (wave-uniform but off, ch0, lane and live)
struct SideJoinLane {
    long long row0, nrows; // the chunk's first pixel; pixels in all
    long long off;         // byte offset of the lane's 4 TB output bytes
    int ch0, N, TB;        // the lane's first channel of the convolution's N; tiles per wave block
    int blk, NSPLIT, lane; // the wave's block of the NSPLIT waves that share the chunk
    bool live;             // the lane's pixel exists (and, in a four-tile block, its sixteen channels)
};

// A join policy travels by value in the kernel's argument block and supplies
//   DISJOINT            the launch's contract keeps the three pointers apart: they are __restrict__
//   pitch, conv_off     output bytes per pixel, and where the convolution's channels start in them
//   before              the join's own memory traffic ahead of the product; it returns the lane's four words for combine
//   combine             the convolution's dword (and wr's) -> the stored dword
struct AddJoin {
    AddArgs add;
    static constexpr bool DISJOINT = false; // out may be exactly run (mf_internal.hpp: fused_run2)
    __device__ __forceinline__ long long pitch(int N) const { return N; }
    __device__ __forceinline__ int conv_off(int, int) const { return 0; }
    // the lane's 4 TB bytes of the running tensor: one 16-byte or 8-byte word where TB makes them one aligned word, else dwords
    __device__ __forceinline__ uint4 before(const int8_t *run, int8_t *, const SideJoinLane &l, int) const {
        uint32_t wr[4] = {0u, 0u, 0u, 0u};
        if (!l.live) {
        } else if (l.TB == 4) {
            const v4i v = *(const v4i *)(run + l.off);
            wr[0] = (uint32_t)v.x, wr[1] = (uint32_t)v.y, wr[2] = (uint32_t)v.z, wr[3] = (uint32_t)v.w;
        } else if (l.TB == 2) {
            const uint2 v = *(const uint2 *)(run + l.off);
            wr[0] = v.x, wr[1] = v.y;
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t < l.TB && l.ch0 + 4 * t < l.N) wr[t] = *(const uint32_t *)(run + l.off + 4 * t);
        }
        return make_uint4(wr[0], wr[1], wr[2], wr[3]);
    }
    template <bool CONV_FIRST> __device__ __forceinline__ uint32_t combine(uint32_t ws, uint32_t wr) const {
        return CONV_FIRST ? add_dword<false>(ws, wr, add) : add_dword<false>(wr, ws, add);
    }
};
struct ConcatJoin {
    ConcatArgs cat;
    int CR; // the running tensor's channels (a whole number of sixteens)
    static constexpr bool DISJOINT = true;
    __device__ __forceinline__ long long pitch(int N) const { return (long long)N + CR; }
    __device__ __forceinline__ int conv_off(int conv_first, int) const { return conv_first ? 0 : CR; }
    template <bool B> __device__ __forceinline__ uint4 word(v4i w) const {
        return make_uint4(concat_dword<B>((uint32_t)w.x, cat), concat_dword<B>((uint32_t)w.y, cat), concat_dword<B>((uint32_t)w.z, cat),
                          concat_dword<B>((uint32_t)w.w, cat));
    }
    // the running slice of the chunk's pixels: 16 CR contiguous bytes of `run`, word w of them belongs to pixel w / wpr
    __device__ __forceinline__ uint4 before(const int8_t *run, int8_t *out, const SideJoinLane &l, int conv_first) const {
        const int wpr = CR >> 4, run_off = conv_first ? l.N : 0;
        for (int w = l.blk * 64 + l.lane; w < 16 * wpr; w += l.NSPLIT * 64) {
            const int pr = w / wpr, j = w - pr * wpr;
            if (l.row0 + pr < l.nrows) {
                const v4i v = *(const v4i *)(run + l.row0 * CR + (long long)w * 16);
                const uint4 y = conv_first ? word<true>(v) : word<false>(v);
                st_out_t<false>(out + (l.row0 + pr) * pitch(l.N) + run_off + j * 16, y);
            }
        }
        return make_uint4(0u, 0u, 0u, 0u);
    }
    template <bool CONV_FIRST> __device__ __forceinline__ uint32_t combine(uint32_t ws, uint32_t) const {
        return concat_dword<!CONV_FIRST>(ws, cat);
    }
};
template <bool R, typename T> struct side_join_ptr { typedef T *type; };
template <typename T> struct side_join_ptr<true, T> { typedef T *__restrict__ type; };

template <int KSC, int MG, uint32_t XR4, class Join>
__global__ __launch_bounds__(256) void side_join_rt(typename side_join_ptr<Join::DISJOINT, const int8_t>::type t_in,
                                                    typename side_join_ptr<Join::DISJOINT, const int8_t>::type run,
                                                    typename side_join_ptr<Join::DISJOINT, int8_t>::type out, SideConvArgs p, Join join, long long nrows) {
    static_assert(MG != 3, "the join reads round-to-nearest bytes: no single-fma epilogue here, modes 0 to 2 only");
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
    const long long pitch = join.pitch(N); // output bytes per pixel
    const int conv_off = join.conv_off(p.conv_first, N);
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
            // the lane's 4 TB bytes of the convolution's channels: one 16-byte or 8-byte word where TB makes them one aligned word (a lane
            // of a four-tile block holds 16 whole channels or none: N is in sixteens), else dwords
            const bool w16 = TB == 4, w8 = TB == 2;
            // (the matrix instructions stay in wave-uniform control flow: only the loads and stores are per lane)
            const SideJoinLane l = {(cb + u) * 16, nrows, row[u] * pitch + conv_off + ch0, ch0, N, TB, blk, NSPLIT, lane,
                                    row[u] < nrows && (!w16 || ch0 + 16 <= N)};
            const uint4 rw = join.before(run, out, l, p.conv_first);
            const uint32_t wr[4] = {rw.x, rw.y, rw.z, rw.w};
            uint32_t res[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t < TB) {
                    v4i acc = {cK[t].x, cK[t].y, cK[t].z, cK[t].w};
#pragma unroll
                    for (int ks = 0; ks < KSC; ++ks)
                        if (ks < KS) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(Aw[t][ks], B[u][ks], acc, 0, 0, 0);
                    const uint32_t ws = requant_pack4<MG, XR4>(acc[0], acc[1], acc[2], acc[3], cA[t], cS[t], p.pw.lo_f, p.pw.hi_f);
                    res[t] = p.conv_first ? join.template combine<true>(ws, wr[t]) : join.template combine<false>(ws, wr[t]);
                }
            }
            if (!l.live) {
            } else if (w16) {
                st_out_t<false>(out + l.off, make_uint4(res[0], res[1], res[2], res[3]));
            } else if (w8) {
                st_out_t<false>(out + l.off, make_uint2(res[0], res[1]));
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t < TB && ch0 + 4 * t < N) *(uint32_t *)(out + l.off + 4 * t) = res[t];
            }
        }
    }
}

// the class's channel bounds: C in whole sixteens up to four k steps, N in whole sixteens up to four wave blocks of four tiles; the
// weights of a wave block are then at most 4 x 4 x 16 = 256 bytes per lane (64 registers)
bool shortcut_add_supported(int C, int N) { return C >= 16 && C <= 256 && C % 16 == 0 && N >= 16 && N <= 256 && N % 16 == 0; }
// ... and for a CONCATENATION the running slice in whole sixteens too, so that every slice starts on a 16-byte boundary
bool side_concat_supported(int C, int N, int CR) { return shortcut_add_supported(C, N) && CR >= 16 && CR % 16 == 0; }

template <int KSC, int MG, uint32_t XR4, class Join>
static void launch_side_join_t(const int8_t *t_in, const int8_t *run, int8_t *out, const SideConvArgs &a, const Join &join, long long nrows, hipStream_t s) {
    static LaunchState st; // (one per instantiation)
    const int per_cu = prepared(st, side_join_rt<KSC, MG, XR4, Join>, 256, 0);
    const int SLOTS = 4 / a.pw.NSPLIT;
    const long long nchunks = (nrows + 15) / 16;
    long long grid = (nchunks + SLOTS * 2 - 1) / (SLOTS * 2);
    // persistent, as pw_rt: a workgroup fetches its operand A once; a few waves of workgroups per CU keep the loads deep
    const long long cap = 256LL * per_cu * 2;
    if (grid > cap) grid = cap;
    if (grid < 1) grid = 1;
    MF_LAUNCH((side_join_rt<KSC, MG, XR4, Join>), dim3((unsigned)grid), dim3(256), 0, s, t_in, run, out, a, join, nrows);
}
template <class Join>
static void launch_side_join(const int8_t *t_in, const int8_t *run, int8_t *out, const SideConvArgs &a, const Join &join, long long batch, hipStream_t s) {
    const long long nrows = batch * a.OH * a.OW;
    if (a.pw.KS <= 1) MF_DISPATCH4(a.pw.magic, a.pw.xr, launch_side_join_t, (t_in, run, out, a, join, nrows, s), 1)
    else if (a.pw.KS == 2) MF_DISPATCH4(a.pw.magic, a.pw.xr, launch_side_join_t, (t_in, run, out, a, join, nrows, s), 2)
    else MF_DISPATCH4(a.pw.magic, a.pw.xr, launch_side_join_t, (t_in, run, out, a, join, nrows, s), 4)
}
void launch_shortcut_add(const int8_t *t_in, const int8_t *run, int8_t *out, const ShortcutAddArgs &a, long long batch, hipStream_t s) {
    launch_side_join(t_in, run, out, a.conv, AddJoin{a.add}, batch, s);
}
void launch_side_concat(const int8_t *t_in, const int8_t *run, int8_t *out, const SideConcatArgs &a, long long batch, hipStream_t s) {
    launch_side_join(t_in, run, out, a.conv, ConcatJoin{a.cat, a.CR}, batch, s);
}

} // namespace k
} // namespace mf
