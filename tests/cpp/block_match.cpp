// The block test of block_band_rt (fused_impl.hpp: match_expand_block) and its plan (k_block_band.hip: k::block_band_plan, from the built
// library) without a GPU: three operators filled by hand, no device call.  One line per case:
//   "<case> no"   or   "<case> noplan"   or
//   "<case> ok CI=.. E=.. N=.. S=.. H=.. W=.. izp=.. RB=.. NB=.. ... band=<lo_r>:<hi_r>:<first staged byte of the image>:<bytes> ..."
// The band fields come from k::block_band_rows, the arithmetic the kernel's staging and expand phase use for their ranges.
#include <cmath>
#include <cstdio>
#include <functional>

#include "fused_impl.hpp"

using mf::OpImpl;

struct Block {
    OpImpl ex, dw, pw;
};

// Conv2D 1x1 C -> E on H x W, DepthwiseConv2D 3x3 SAME at stride S on E, Conv2D 1x1 E -> N: zero filter zero points, izp 4
static void fill(Block &b, int H, int W, int C, int E, int S, int N) {
    mf::OpSpec &e = b.ex.s, &d = b.dw.s, &q = b.pw.s;
    e = mf::OpSpec{}, d = mf::OpSpec{}, q = mf::OpSpec{};
    e.kind = MF_OP_CONV_2D, e.H = H, e.W = W, e.C = C, e.N = E, e.KH = 1, e.KW = 1, e.sh = 1, e.sw = 1, e.pad = MF_PAD_SAME, e.OH = H, e.OW = W;
    d.kind = MF_OP_DEPTHWISE_CONV_2D, d.H = H, d.W = W, d.C = E, d.N = E, d.KH = 3, d.KW = 3, d.sh = S, d.sw = S, d.pad = MF_PAD_SAME;
    d.OH = (H + S - 1) / S, d.OW = (W + S - 1) / S;
    q.kind = MF_OP_CONV_2D, q.H = d.OH, q.W = d.OW, q.C = E, q.N = N, q.KH = 1, q.KW = 1, q.sh = 1, q.sw = 1, q.pad = MF_PAD_SAME, q.OH = q.H, q.OW = q.W;
    b.ex.h_wzp.assign((size_t)E, 0), b.dw.h_wzp.assign((size_t)E, 0), b.pw.h_wzp.assign((size_t)N, 0);
    b.dw.conv.izp = 4;
}

static void run(const char *name, int H, int W, int C, int E, int S, int N, const std::function<void(Block &)> &change) {
    Block b;
    fill(b, H, W, C, E, S, N);
    change(b);
    const mf::BlockMatch m = mf::match_expand_block(&b.ex, &b.dw, &b.pw);
    if (!m) {
        printf("%s no\n", name);
        return;
    }
    mf::k::BlockBandArgs bb{};
    if (!mf::k::block_band_plan(m.pair.geom, m.CI, bb)) {
        printf("%s noplan\n", name);
        return;
    }
    const mf::k::PairBandArgs &a = bb.b;
    printf("%s ok CI=%d E=%d N=%d S=%d H=%d W=%d izp=%u RB=%d NB=%d TR=%d ROW=%d TILE=%d in_off=%d in_bytes=%d tile_off=%d mid_off=%d mid_bytes=%d q_off=%d lds=%d wgs=%d CX=%d CY=%d "
           "UX=%d UY=%d NCH=%d KSC=%d KSI=%d TB=%d NBLK=%d SLOTS=%d NWB=%d nfull=%d",
           name, bb.CI, a.C, a.N, a.S, a.H, a.W, a.izp4 & 0xffu, a.RB, a.NB, a.TR, a.ROW, a.TILE, bb.in_off, bb.in_bytes, a.tile_off, a.mid_off, a.mid_bytes, a.q_off, a.lds_bytes, a.wgs,
           1 << a.lgCX, 1 << a.lgCY, a.UX, a.UY, a.NCH, a.KSC, bb.KSI, a.TB, a.NBLK, a.SLOTS, a.NWB, bb.nfull);
    for (int band = 0; band < a.NB; ++band) {
        int lo_r = 0, hi_r = 0;
        mf::k::block_band_rows(a.H, a.S, a.RB, a.TR, band, lo_r, hi_r);
        const long long start = (long long)(a.S * band * a.RB - 1 + lo_r) * a.W * bb.CI, len = (long long)(hi_r - lo_r) * a.W * bb.CI;
        printf(" band=%d:%d:%lld:%lld", lo_r, hi_r, start, len);
    }
    printf("\n");
}

int main() {
    const auto none = [](Block &) {};
    // the six blocks of tests/test_gpu_expand_block.py
    run("6x6x8-32-8", 6, 6, 8, 32, 1, 8, none);
    run("9x7x16-64-24", 9, 7, 16, 64, 1, 24, none);
    run("13x11x12-48-20", 13, 11, 12, 48, 1, 20, none);
    run("10x10x24-144s2-32", 10, 10, 24, 144, 2, 32, none);
    run("40x40x16-96-16", 40, 40, 16, 96, 1, 16, none);
    run("34x30x32-256s2-64", 34, 30, 32, 256, 2, 64, none);
    // one refusal per condition, each the 12x12x16 -> 64 -> 16 block but for that condition
    run("base", 12, 12, 16, 64, 1, 16, none);
    run("E_le_N", 12, 12, 16, 64, 1, 64, none);
    run("E_le_C", 12, 12, 64, 64, 1, 16, none);
    run("E_mod16", 12, 12, 12, 36, 1, 12, none);
    run("E_272", 12, 12, 16, 272, 1, 16, none);
    run("expand3x3", 12, 12, 16, 64, 1, 16, [](Block &b) { b.ex.s.KH = 3, b.ex.s.KW = 3; });
    run("expand_stride2", 12, 12, 16, 64, 1, 16, [](Block &b) { b.ex.s.sh = 2, b.ex.s.sw = 2; });
    run("expand_other_HW", 12, 12, 16, 64, 1, 16, [](Block &b) { b.ex.s.H = 24, b.ex.s.W = 24, b.ex.s.OH = 24, b.ex.s.OW = 24; });
    run("wzp_expand", 12, 12, 16, 64, 1, 16, [](Block &b) { b.ex.h_wzp[3] = 5; });
    run("wzp_depthwise", 12, 12, 16, 64, 1, 16, [](Block &b) { b.dw.h_wzp[3] = -2; });
    run("wzp_project", 12, 12, 16, 64, 1, 16, [](Block &b) { b.pw.h_wzp[3] = 1; });
    run("element_type", 12, 12, 16, 64, 1, 16, [](Block &b) { b.ex.s.u8 = true; });
    run("element_type_pair", 12, 12, 16, 64, 1, 16, [](Block &b) { b.pw.s.u8 = true; });
    run("expand_not_finite", 12, 12, 16, 64, 1, 16, [](Block &b) { b.ex.finite_consts = false; });
    run("depthwise_not_finite", 12, 12, 16, 64, 1, 16, [](Block &b) { b.dw.finite_consts = false; });
    run("project_not_finite", 12, 12, 16, 64, 1, 16, [](Block &b) { b.pw.finite_consts = false; });
    run("odd_width_stride2", 9, 9, 16, 64, 2, 16, none);
    run("generic_expand", 12, 12, 16, 64, 1, 16, [](Block &b) { b.ex.force_generic = true; });
    run("generic_depthwise", 12, 12, 16, 64, 1, 16, [](Block &b) { b.dw.force_generic = true; });
    run("generic_project", 12, 12, 16, 64, 1, 16, [](Block &b) { b.pw.force_generic = true; });
    run("device", 12, 12, 16, 64, 1, 16, [](Block &b) { b.ex.device = 1; });
    run("dw5x5", 12, 12, 16, 64, 1, 16, [](Block &b) { b.dw.s.KH = 5, b.dw.s.KW = 5; });
    return 0;
}
