// k_pool_fc.hip -- the usual classifier head in one launch: AveragePool2D over the whole [H][W][C] image (microflow::ops::
// average_pool_2d, src/ops/average_pool_2d.rs:29-66) -> [Reshape] -> 1 .. FC_CHAIN_MAX FullyConnected layers -> [Softmax].
// Only the image and the last operator's output touch HBM.
//
// A step is R images (a multiple of 16), in two phases:
//
//   pool   : the sum over the pixels is a product with a constant 0/1 operand.  Operand B of v_mfma_i32_16x16x64_i8 comes straight
//            from HBM in MFMA layout, as pw_mfma's does: a lane's 16 bytes are 16 channels of one pixel, the four lane groups are
//            four pixels, and column j of the product is (channel group pass 16 + j % CGW, pixel subset j / CGW) of ONE image, so
//            that a wave's load instruction covers 4 NS consecutive pixels x CGW 16 = up to 1 KiB of contiguous bytes.  Operand
//            A holds a 1 at k = 16 g + i for row i, so D[i][j] accumulates channel i of the column's channel group over all its
//            pixels.  C / 16 that neither divides nor is a multiple of 16 (C = 48, 96, 320, 576 ...) leaves columns idle (their
//            lanes supply zeros); so does a pixel past the image (H W not a multiple of 4 NS).  Such a lane reads the batch's first
//            16 bytes instead, so nothing is read past batch x H W C.  A wave walks (image, pass, load) with the next four loads issued before the current four are
//            consumed, across images: 4 .. 8 loads in flight per lane whatever the image size.  No LDS staging: every input byte is
//            loaded once, into registers.  After the last pixel the NS columns of a channel group are added across lanes, and a
//            lane holds 4 consecutive channels of one image: avgpool_generic's arithmetic (k_generic.hip), value by value, and one
//            dword into the int8 [R][C] tile in LDS.
//   layers : fc_chain's step (k_fc_layer.hpp) with that tile as layer 0's operand: per layer products, weight-zero-point row sums
//            and requant_pack4 -- the bytes of the layers' own launches; softmax_table's arithmetic; the output patch in aligned
//            16-byte stores with byte edges.  Nothing past batch x N_last is written.
//
// The layers' weight images (their fc_rt images) arrive once per workgroup by LDS-DMA.  The plan keeps a workgroup's LDS small
// enough for two or more per CU where the weights allow: one workgroup's pool phase (HBM) runs under another's layer phase.
#include "k_common.hpp"
#include "k_fc_layer.hpp"

#include <algorithm>

#include "k_pool_fc_body.hpp"

namespace mf {
namespace k {

template <int MG, uint32_t XR4>
__global__ __launch_bounds__(256) void pool_fc_chain(const int8_t *__restrict__ in, int8_t *__restrict__ out, PoolFcArgs p, long long rows) {
    pool_fc_body<MG, XR4, false>(in, out, p, rows, F32Edge{});
}

// ---- host side ----------------------------------------------------------------------------------------------------
// Geometry: R aims at ~64 KiB of image bytes per step (16 loads per wave: small images need many per step to keep loads in flight
// across them), 16 .. 128 images and at most 32 KiB per activation tile; then as few images as it takes to leave room for two
// workgroups per CU (half the LDS), or, where the weights alone are past that, to fit the budget at all.
bool pool_fc_plan(PoolFcArgs &a) {
    FcChainArgs &c = a.c;
    if (c.L < 1 || c.L > FC_CHAIN_MAX || a.P < 1 || a.C < 16 || a.C % 16 != 0 || (long long)a.P * a.C > (1 << 28)) return false;
    if (c.l[0].K != a.C) return false;
    long long W = 0;
    int nmax = 0;                                    // widest tensor kept in an activation buffer
    for (int l = 0; l < c.L; ++l) {
        FcChainLayer &y = c.l[l];
        if (y.K < 1 || y.N < 1 || (l > 0 && y.K != c.l[l - 1].N)) return false;
        y.KS = (y.K + 63) / 64, y.NT = (y.N + 15) / 16;
        y.woff = (int)W;
        W += (long long)y.NT * y.KS * 1024;
        if (l < c.L - 1 || c.softmax) nmax = std::max(nmax, y.N);
    }
    const int NL = c.l[c.L - 1].N, CG = a.C / 16;
    a.CGW = std::min(CG, 16), a.NS = 16 / a.CGW, a.NPASS = (CG + 15) / 16, a.NIT = (a.P + 4 * a.NS - 1) / (4 * a.NS);
    auto rb = [](long long bytes) { return (long long)((bytes + 112 + 15) & ~15ll); }; // (+ the over-read of a 16-byte operand piece)
    auto total = [&](int R) { return W + rb((long long)R * a.C) + 2 * rb((long long)R * nmax) + (((long long)R * NL + 32 + 15) & ~15ll); };
    int R = (int)std::min<long long>(std::max<long long>(65536 / ((long long)a.P * a.C) / 16 * 16, 16), 128);
    while (R > 16 && (long long)R * std::max(nmax, NL) > 32768) R -= 16;
    if ((long long)R * std::max(nmax, NL) > 32768) return false;
    const long long half = 80 * 1024 - 512;          // two workgroups per CU
    const long long budget = total(16) <= half ? half : FC_RT_LDS_MAX;
    while (R > 16 && total(R) > budget) R -= 16;
    if (total(R) > budget) return false;
    c.R = R, c.NBUF = 1;
    c.xoff = (int)W, c.xbytes = (int)rb((long long)R * a.C);
    c.aoff = c.xoff + c.xbytes, c.abytes = (int)rb((long long)R * nmax);
    c.poff = c.aoff + 2 * c.abytes, c.lds = (int)total(R);
    pool_fc_tb(c, R);
    volatile float inv = 1.0f / (float)a.P;          // 1. / view.len as f32 (average_pool_2d.rs:52)
    a.inv = inv;
    return true;
}

template <int MG, uint32_t XR4>
static void launch_pool_fc_t(const int8_t *in, int8_t *out, const PoolFcArgs &a, long long rows, hipStream_t s) {
    static LaunchState st[FC_RT_LDS_MAX / 1024 + 2]; // occupancy per (device, LDS KiB): asked once, never during a capture
    const int per_cu = prepared(st[(a.c.lds + 1023) / 1024], pool_fc_chain<MG, XR4>, 256, a.c.lds);
    // fewer images per step than planned when the batch would otherwise give fewer than ~1024 steps (as launch_fc_rt_t); the
    // planned LDS layout holds any smaller step
    PoolFcArgs b = a;
    b.c.R = (int)std::min<long long>(a.c.R, std::max<long long>(16, rows / 1024 / 16 * 16));
    pool_fc_tb(b.c, b.c.R);
    const long long ntiles = (rows + b.c.R - 1) / b.c.R;
    const long long grid = std::min(ntiles, 256LL * per_cu);
    MF_LAUNCH((pool_fc_chain<MG, XR4>), dim3((unsigned)grid), dim3(256), a.c.lds, s, in, out, b, rows);
}
void launch_pool_fc(const int8_t *in, int8_t *out, const PoolFcArgs &a, long long batch, hipStream_t s) {
    if (batch <= 0) return;
    if (a.c.xr) {
        if (a.c.magic == 2) launch_pool_fc_t<2, 0x80808080u>(in, out, a, batch, s);
        else if (a.c.magic) launch_pool_fc_t<1, 0x80808080u>(in, out, a, batch, s);
        else launch_pool_fc_t<0, 0x80808080u>(in, out, a, batch, s);
    } else {
        if (a.c.magic == 2) launch_pool_fc_t<2, 0u>(in, out, a, batch, s);
        else if (a.c.magic) launch_pool_fc_t<1, 0u>(in, out, a, batch, s);
        else launch_pool_fc_t<0, 0u>(in, out, a, batch, s);
    }
}

} // namespace k
} // namespace mf
