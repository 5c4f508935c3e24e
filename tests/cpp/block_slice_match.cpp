// The block test of block_slice_rt (fused_impl.hpp: match_expand_block_deep) and its plan (k_block_slice.hip: k::block_slice_plan, from
// the built library) without a GPU: three operators filled by hand, no device call.  One line per case:
//   "<case> no"   or   "<case> noplan"   or   "<case> ok CI=.. E=.. N=.. ... lds=.."
#include <cstdio>
#include <functional>

#include "fused_impl.hpp"

struct Block {
    mf::OpImpl ex, dw, pw;
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
    const mf::BlockMatch m = mf::match_expand_block_deep(&b.ex, &b.dw, &b.pw);
    if (!m) {
        printf("%s no\n", name);
        return;
    }
    mf::k::BlockSliceArgs bs{};
    if (!mf::k::block_slice_plan(m.pair.geom, m.CI, bs)) {
        printf("%s noplan\n", name);
        return;
    }
    const mf::k::PairBandArgs &a = bs.b;
    printf("%s ok CI=%d E=%d N=%d S=%d H=%d W=%d izp=%u NS=%d NT=%d KSI=%d UPW=%d PC=%d PT=%d WC=%d WT=%d RB=%d NB=%d TR=%d ROW=%d TILE=%d NCH=%d CY=%d in_off=%d in_bytes=%d tile_off=%d "
           "mid_off=%d mid_bytes=%d q_off=%d lds=%d wgs=%d\n",
           name, bs.CI, bs.E, a.N, a.S, a.H, a.W, a.izp4 & 0xffu, bs.NS, bs.NT, bs.KSI, bs.UPW, mf::k::block_slice_pc(bs.UPW), mf::k::block_slice_pt(bs.UPW), 1 << bs.lgWC, 8 >> bs.lgWC, a.RB,
           a.NB, a.TR, a.ROW, a.TILE, a.NCH, 1 << a.lgCY, bs.in_off, bs.in_bytes, a.tile_off, a.mid_off, a.mid_bytes, a.q_off, a.lds_bytes, a.wgs);
}

int main() {
    const auto none = [](Block &) {};
    // the blocks of tests/test_gpu_block_slice.py
    run("6x6x8-320-8", 6, 6, 8, 320, 1, 8, none);
    run("9x7x16-384-24", 9, 7, 16, 384, 1, 24, none);
    run("10x10x24-320s2-32", 10, 10, 24, 320, 2, 32, none);
    run("14x14x96-576-96", 14, 14, 96, 576, 1, 96, none);
    run("7x7x160-960-320", 7, 7, 160, 960, 1, 320, none);
    run("40x40x16-320-16", 40, 40, 16, 320, 1, 16, none);
    run("10x10x8-320s2-8", 10, 10, 8, 320, 2, 8, none);
    run("9x7x96-384-24", 9, 7, 96, 384, 1, 24, none);
    run("9x7x96-384-40", 9, 7, 96, 384, 1, 40, none);
    // one refusal per condition
    run("E_272", 12, 12, 16, 272, 1, 16, none);
    run("E_256", 12, 12, 16, 256, 1, 16, none);
    run("E_le_N", 7, 7, 160, 320, 1, 320, none);
    run("C_196", 7, 7, 196, 960, 1, 160, none);
    run("N_324", 7, 7, 160, 960, 1, 324, none);
    run("wzp_project", 12, 12, 16, 320, 1, 16, [](Block &b) { b.pw.h_wzp[3] = 1; });
    run("odd_width_stride2", 9, 9, 16, 320, 2, 16, none);
    return 0;
}
