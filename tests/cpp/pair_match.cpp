// The fused units' one pair test (fused_impl.hpp: match_dw3x3_pw1x1) without a GPU: two operators filled by hand, no device call.
//   pair_match   ->   one line per case: "<case> ok {H, W, C, S, OH, OW, N, izp4} f=<0|1>"  or  "<case> no"
#include <cmath>
#include <cstdio>
#include <functional>

#include "fused_impl.hpp"

using mf::OpImpl;

// a DepthwiseConv2D 3x3 SAME on 6x6x16 at stride S (dw3x3_rt) and the Conv2D 1x1 to N channels behind it (pw_rt)
static void fill(OpImpl &dw, OpImpl &pw, int S, int N) {
    mf::OpSpec &d = dw.s, &q = pw.s;
    d = mf::OpSpec{}, q = mf::OpSpec{};
    d.kind = MF_OP_DEPTHWISE_CONV_2D, d.H = 6, d.W = 6, d.C = 16, d.N = 16, d.KH = 3, d.KW = 3, d.sh = S, d.sw = S, d.pad = MF_PAD_SAME;
    d.OH = (6 + S - 1) / S, d.OW = (6 + S - 1) / S;
    q.kind = MF_OP_CONV_2D, q.H = d.OH, q.W = d.OW, q.C = 16, q.N = N, q.KH = 1, q.KW = 1, q.sh = 1, q.sw = 1, q.pad = MF_PAD_SAME;
    q.OH = q.H, q.OW = q.W;
    dw.fast = OpImpl::DW_RT, pw.fast = OpImpl::PW_RT;
    dw.dwrt.dw.izp4 = 0x04040404u;
}

static void run(const char *name, int S, int N, const std::function<void(OpImpl &, OpImpl &)> &change) {
    OpImpl dw, pw;
    fill(dw, pw, S, N);
    change(dw, pw);
    const mf::PairMatch m = mf::match_dw3x3_pw1x1(&dw, &pw);
    if (!m) {
        printf("%s no\n", name);
        return;
    }
    const mf::k::ChainGeom &g = m.geom;
    printf("%s ok {%d, %d, %d, %d, %d, %d, %d, izp%u} f=%d\n", name, g.H, g.W, g.C, g.S, g.OH, g.OW, g.N, g.izp4 & 0xffu, m.f == &dw.dwrt.dw ? 1 : 0);
}

int main() {
    const auto none = [](OpImpl &, OpImpl &) {};
    run("stride1", 1, 16, none);
    run("stride2", 2, 32, none);
    // one refusal per condition, each the stride-1 pair but for that condition
    run("filter5x5", 1, 16, [](OpImpl &dw, OpImpl &) { dw.s.KH = 5, dw.s.KW = 5; });
    run("valid", 1, 16, [](OpImpl &dw, OpImpl &) { dw.s.pad = MF_PAD_VALID; });
    run("sh_ne_sw", 1, 16, [](OpImpl &dw, OpImpl &) { dw.s.sw = 2; });
    run("stride3", 1, 16, [](OpImpl &dw, OpImpl &) { dw.s.sh = 3, dw.s.sw = 3; });
    run("multiplier2", 1, 16, [](OpImpl &dw, OpImpl &pw) { dw.s.N = 32, pw.s.C = 32; }); // (the 1x1 still reads exactly the depthwise output)
    run("second3x3", 1, 16, [](OpImpl &, OpImpl &pw) { pw.s.KH = 3, pw.s.KW = 3; });
    run("second_stride2", 1, 16, [](OpImpl &, OpImpl &pw) { pw.s.sh = 2, pw.s.sw = 2; });
    run("second_H", 1, 16, [](OpImpl &, OpImpl &pw) { pw.s.H = 5, pw.s.OH = 5; });
    run("second_C", 1, 16, [](OpImpl &, OpImpl &pw) { pw.s.C = 32; });
    run("element_type", 1, 16, [](OpImpl &, OpImpl &pw) { pw.s.u8 = true; });
    run("device", 1, 16, [](OpImpl &, OpImpl &pw) { pw.device = 1; });
    run("dw_not_finite", 1, 16, [](OpImpl &dw, OpImpl &) { dw.finite_consts = false; });
    run("pw_not_finite", 1, 16, [](OpImpl &, OpImpl &pw) { pw.finite_consts = false; });
    // what is NOT shared stays with the callers: the matcher takes these
    run("other_kernels", 1, 16, [](OpImpl &dw, OpImpl &pw) { dw.fast = OpImpl::NONE, pw.fast = OpImpl::NONE; });
    run("force_generic", 1, 16, [](OpImpl &dw, OpImpl &) { dw.force_generic = true; });
    run("odd_width_stride2", 2, 16, [](OpImpl &dw, OpImpl &pw) { dw.s.W = 7, dw.s.OW = 4, pw.s.W = 4, pw.s.OW = 4; });
    return 0;
}
