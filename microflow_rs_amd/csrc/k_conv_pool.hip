// k_conv_pool.hip -- a Conv2D and the AveragePool2D behind it in one launch (microflow::ops::conv_2d, src/ops/conv_2d.rs:28-108;
// microflow::ops::average_pool_2d, src/ops/average_pool_2d.rs:29-66): the stages of LeNet-style CNNs.  The convolution's output, the
// widest tensor of such a network, is written by one launch and read back by the next only to be averaged; here it lives in LDS.
//
//   step    : G whole images, or one band of PB pooled rows of one image (kernels.hpp conv_pool_band: the convolution rows the band's
//             windows read; overlapping windows recompute the shared rows at a band edge).  Persistent workgroups walk the steps.
//   phase A : conv_gemm_rt's staging and product (k_conv_gemm.hip) with the whole weight image resident: the input tile inside its
//             input-zero-point halo, K' = [ky][pad16(KW C)], the [KS][4] tap table, the operand from aligned reads (AL = 16 / 4 / 1),
//             the ones-tile MFMA and the mask table for filter zero points, requant_pack4 with the convolution's own constants.  Each
//             lane's packed dword -- the bytes the convolution's own launch would store -- goes to Y[g][row][ox][NP] in LDS.
//   phase B : one work item is (image, pooled pixel, channel quad): one dword of Y per in-range tap, summed per byte with masked
//             v_dot4 as avgpool_c4 does, then avgpool_generic's arithmetic (k_generic.hip) value by value with the pool's own
//             constants.  The pooled bytes of a step are one contiguous range of the output: dwords where N % 4 == 0, else one byte
//             per real channel.
//
// Three barriers per step: top of the step (the previous step's reads of the tile and of Y are done), tile staged, Y complete.
#include "k_common.hpp"

#include <algorithm>
#include <map>
#include <mutex>

namespace mf {
namespace k {

#define MF_CONV_POOL_KERNEL conv_pool_rt
#define MF_CONV_POOL_MAX 0
#define MF_CONV_POOL_LAUNCH launch_conv_pool
#define MF_CONV_POOL_LAUNCH_T launch_conv_pool_t
#define MF_CONV_POOL_LAUNCH_W launch_conv_pool_w
#include "k_conv_pool_body.inc" // the kernel and its launcher: shared with k_conv_maxpool.hip

// ---- host side ----------------------------------------------------------------------------------------------------
// The whole weight image, then per step G tiles and G images of Y (at most 16 images and 48 KiB of tiles, as conv_gemm_plan): inside
// 80 KiB where that holds one whole image (two workgroups per CU), else the widest that fits, else bands of PB pooled rows -- PB as
// large as fits, the bands evened out.
bool conv_pool_plan(ConvPoolArgs &a, std::vector<int> &tap, std::vector<uint32_t> &mask, int H, int W, int C, int N, int KH, int KW, int sh, int sw,
                    int OH, int OW, bool pad_same, bool wz, int PFH, int PFW, int psh, int psw, int POH, int POW, bool pool_same) {
    if (H < 1 || W < 1 || C < 1 || N < 1 || KH < 1 || KW < 1 || sh < 1 || sw < 1 || OH < 1 || OW < 1) return false;
    if (PFH < 1 || PFW < 1 || psh < 1 || psw < 1 || POH < 1 || POW < 1) return false;
    if (POH * POW < 2) return false;                     // (a global pool belongs to the tail and pool_fc_chain groups)
    if ((W * C) % 4 != 0) return false;                  // whole-dword image rows
    const int pshy = pool_same ? (PFH - 1) / 2 : 0, pshx = pool_same ? (PFW - 1) / 2 : 0;
    if (!pool_same && ((POH - 1) * psh + PFH > OH || (POW - 1) * psw + PFW > OW)) return false; // a VALID window leaves the tensor
    if ((POH - 1) * psh - pshy >= OH || (POW - 1) * psw - pshx >= OW) return false;              // a window with no tap at all
    const int KWC = KW * C, KWCP = (KWC + 15) & ~15, KS = (KH * KWCP + 63) / 64, NT = (N + 15) / 16;
    if (KS > CONV_GEMM_KS_MAX) return false;
    const int padl = pad_same ? (KW - 1) / 2 : 0, padt = pad_same ? (KH - 1) / 2 : 0;
    const int LP = (padl * C + 15) & ~15;
    // bytes read right of the image row: the last window's padded filter row (+ the 4 bytes of the aligned reads)
    const int over = std::max(0, ((OW - 1) * sw - padl) * C + KWCP + 4 - W * C);
    const int ROW = ((LP + W * C + over + 15) & ~15) + 16;
    const int tabb = KS * 16 + (wz ? KS * 64 : 0) + NT * 256; // tap table, masks, the constants [Kc | A | S | wzp][NT 16]
    const int NP4 = (N + 3) / 4, NP = 4 * (NP4 % 2 == 0 ? NP4 + 1 : NP4); // an odd number of dwords per pixel: 16 pixels, 16 banks
    const long long wbytes = (long long)NT * KS * 1024;
    a.H = H, a.W = W, a.C = C, a.N = N, a.KH = KH, a.KW = KW, a.sh = sh, a.sw = sw, a.OH = OH, a.OW = OW;
    a.padl = padl, a.padt = padt, a.KWCP = KWCP, a.KS = KS, a.NT = NT, a.TB = std::min(4, NT), a.LP = LP, a.ROW = ROW;
    a.PFH = PFH, a.PFW = PFW, a.psh = psh, a.psw = psw, a.POH = POH, a.POW = POW, a.pshy = pshy, a.pshx = pshx, a.NP = NP;
    auto rows_for = [&](int cb) { return (cb - 1) * sh + KH; };
    auto ybytes = [&](int cb) { return ((long long)cb * OW * NP + 15) & ~15LL; };
    // the most convolution rows a band of `pb` pooled rows reads
    auto conv_rows = [&](int pb) {
        int cb = 0;
        for (int b = 0; b * pb < POH; ++b) {
            int py0, py1, c0, c1;
            conv_pool_band(OH, POH, pb, psh, pshy, PFH, b, py0, py1, c0, c1);
            cb = std::max(cb, c1 - c0);
        }
        return cb;
    };
    auto finish = [&](int G, int PB, int CB) {
        a.G = G, a.PB = PB, a.NB = (POH + PB - 1) / PB, a.CB = CB, a.RB = rows_for(CB), a.TILE = a.RB * ROW, a.YIMG = (int)ybytes(CB);
        a.xoff = (int)wbytes, a.yoff = a.xoff + G * a.TILE + 256, a.toff = a.yoff + G * a.YIMG, a.moff = a.toff + KS * 16;
        a.coff = a.moff + (wz ? KS * 64 : 0), a.lds = a.toff + tabb;
        tap.assign((size_t)KS * 4, 0);
        mask.assign((size_t)KS * 16, 0);
        for (int ks = 0; ks < KS; ++ks)
            for (int gg = 0; gg < 4; ++gg) {
                const int k0 = ks * 64 + gg * 16, ky = k0 / KWCP, j = k0 % KWCP;
                if (ky >= KH) continue;                  // beyond K': zero weights, offset 0, no window bytes
                tap[(size_t)ks * 4 + gg] = ky * ROW + j;
                for (int i = 0; i < 16; ++i)
                    if (j + i < KWC) mask[(size_t)(ks * 4 + gg) * 4 + i / 4] |= 0xffu << (8 * (i & 3));
            }
        return true;
    };
    const int cb_all = conv_rows(POH);
    const long long tile_all = (long long)rows_for(cb_all) * ROW, per_img = tile_all + ybytes(cb_all);
    for (int pass = 0; pass < 2; ++pass) {
        const long long avail = (pass == 0 ? 80 * 1024 : CONV_GEMM_LDS_MAX) - wbytes - tabb - 256;
        if (tile_all > 48 * 1024 || avail < per_img) continue;
        const int G = (int)std::min<long long>(std::min<long long>(16, 48 * 1024 / tile_all), avail / per_img);
        return finish(G, POH, cb_all);
    }
    const long long avail = CONV_GEMM_LDS_MAX - wbytes - tabb - 256;
    auto fits = [&](int pb) {
        const int cb = conv_rows(pb);
        const long long tile = (long long)rows_for(cb) * ROW;
        return tile <= 48 * 1024 && tile + ybytes(cb) <= avail;
    };
    int pb = POH;
    while (pb > 1 && !fits(pb)) --pb;
    if (!fits(pb)) return false;                         // the weights do not fit whole beside a band of one pooled row
    const int nb = (POH + pb - 1) / pb;
    pb = (POH + nb - 1) / nb;                            // evened out (not larger than the one that fits)
    while (pb > 1 && !fits(pb)) --pb;                    // (an evened band may read one more convolution row at another phase of the stride)
    return finish(1, pb, conv_rows(pb));
}

} // namespace k
} // namespace mf
