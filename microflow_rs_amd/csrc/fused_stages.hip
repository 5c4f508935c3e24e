// fused_stages.hip -- second-level groups: pair groups that already exist (fused_pairs.hip) joined with their neighbours into one
// launch -- the stage, the quads, the stem in front of a quad, the pair (and the pair before it) in front of the tail.  The groups
// inside stay available for mf_model_run_until.  Host code only; the kernels are in k_*.hip.
#include <cstring>

#include "fused_impl.hpp"

namespace mf {

// A run of `npairs` identical DepthwiseConv2D 3x3 (stride 1) + Conv2D 1x1 pairs on one small tensor as one persistent
// kernel (k_stage.hip: five pairs on 6x6x128 = person_detect ops 13..22).  `pairs` are the already created pair
// groups; returns nullptr when no stage kernel exists for them.
FusedImpl *fused_stage_create(FusedImpl *const *pairs, int npairs) {
    const bool off = switches().no_stage;
    if (off || npairs < 2 || !pairs[0] || pairs[0]->kind != FusedImpl::DWPW) return nullptr;
    const OpSpec &d0 = pairs[0]->a->s;
    const char *nm = k::stage_name(d0.H, d0.W, d0.C, npairs);
    if (!nm) return nullptr;
    for (int i = 0; i < npairs; ++i) {
        const FusedImpl *f = pairs[i];
        if (!f || f->kind != FusedImpl::DWPW) return nullptr;
        const OpSpec &d = f->a->s, &q = f->b->s;
        if (d.H != d0.H || d.W != d0.W || d.C != d0.C || d.sh != 1 || q.N != d0.C) return nullptr; // same tensor in and out
        if (d.u8 != d0.u8 || q.u8 != d0.u8 || !f->dwpw.dw.magic || !f->dwpw.pw.magic || !f->dwpw.dw.wmm) return nullptr; // bit-pattern epilogues
        if (f->dwpw.dw.izp4 != pairs[0]->dwpw.dw.izp4 || f->a->device != pairs[0]->a->device) return nullptr;
    }
    bool all_fma = true; // the single-fma form needs it of every operator of the run
    for (int i = 0; i < npairs; ++i) all_fma = all_fma && pairs[i]->a->fma_ok && pairs[i]->b->fma_ok;
    // ... and their patched accumulators as the kernel's table: [pair][depthwise, pointwise][wave = aligned 16-channel group][2]
    std::vector<k::EpiPatchRec> ptab((size_t)npairs * 32, k::EpiPatchRec{0, 0});
    for (int i = 0; i < npairs && all_fma; ++i)
        for (int ph = 0; ph < 2 && all_fma; ++ph) {
            const k::EpiPatch &pl = (ph ? pairs[i]->b : pairs[i]->a)->fma_patch;
            for (int e = 0; e < pl.n && all_fma; ++e) {
                const int ch = pl.ch[e];
                if (ch < 0 || ch >= 128) { // (the table has the eight 16-channel groups of this kernel's 128 channels)
                    all_fma = false;
                    break;
                }
                k::EpiPatchRec *slot = &ptab[(((size_t)i * 2 + ph) * 8 + (size_t)(ch >> 4)) * 2];
                if (slot[0].P != 0) ++slot;
                if (slot->P != 0) all_fma = false; // (three in one group: the kernel's table holds two)
                else *slot = k::epi_patch_rec(pl.P[e], pl.R[e], ch & 3, (ch >> 2) & 3);
                if (all_fma && slot != &ptab[(((size_t)i * 2 + ph) * 8 + (size_t)(ch >> 4)) * 2]) slot[-1].meta |= 32; // "a second record follows"
            }
        }
    std::unique_ptr<FusedImpl> s = make_group(FusedImpl::STAGE, pairs[0]->a, pairs[npairs - 1]->b, nullptr, nm);
    s->stage.pairs = npairs;
    std::vector<k::StagePair> table((size_t)npairs);
    for (int i = 0; i < npairs; ++i) {
        const OpImpl *dw = pairs[i]->a, *pw = pairs[i]->b;
        const k::DwPwArgs pa = pair_args(dw, pw, all_fma ? 2 : 0);
        k::StagePair &sp = table[(size_t)i];
        set_pair_consts(sp, pa.dw, pa.pw);
        // (this kernel takes Kc with the bit-pattern offset already added)
        sp.dw_wmm = pa.dw.wmm, sp.dwK = kc_with_magic(*s, host_kc(dw, pa.dw.Kc));
        sp.pw_w = plain_pw_image(*s, pw);
        sp.pwK = kc_with_magic(*s, host_kc(pw, pa.pw.Kc));
    }
    k::StageArgs &a = s->stage.args;
    a.patch_tab = nullptr;
    if (all_fma) { // (also when nothing is patched: the kernel fetches its records with the operands, unconditionally)
        a.patch_tab = (const k::EpiPatchRec *)keep(*s, ptab.data(), ptab.size() * sizeof(k::EpiPatchRec));
    }
    a.pairs = (const k::StagePair *)keep(*s, table.data(), table.size() * sizeof(k::StagePair));
    a.izp4 = pairs[0]->dwpw.dw.izp4;
    a.xr4 = d0.u8 ? 0x80808080u : 0u;
    a.queue = pairs[0]->dwpw.dw.queue, a.qlaunch = pairs[0]->dwpw.dw.qlaunch;
    a.mode = all_fma ? 3 : 2; // the saturating-pack epilogue needs it of every operator of the run
    for (int i = 0; i < npairs && !all_fma; ++i)
        if (pairs[i]->a->magic_mode != 2 || pairs[i]->b->magic_mode != 2) a.mode = 1;
    s->epi_mode = a.mode;
    return s.release();
}

// The pair's operand images and constants as the pair + tail kernels take them (PairTailArgs / PairFrontArgs share the names): Kc with
// the bit-pattern offset added where the launch runs the bit-pattern epilogue
template <typename T> static void pair_tail_operands(FusedImpl &f, T &a, const OpImpl *dw, const OpImpl *pw, const k::DwFastArgs &df, int magic) {
    set_pair_consts(a, df, pw->conv);
    a.dw_wmm = df.wmm, a.izp4 = df.izp4;
    if (magic) a.dwK = kc_with_magic(f, dw->h_Kc);
    a.pw_w = plain_pw_image(f, pw);
    if (magic) a.pwK = kc_with_magic(f, pw->h_Kc);
}

// The last pair group (DepthwiseConv2D 3x3 stride 1 + Conv2D 1x1 on 3x3x256) followed by the tail group
// (AveragePool2D over the whole tensor -> head Conv2D -> Softmax) as one kernel (k_tail3.hip).  nullptr when the shapes are not the
// compiled instance.
FusedImpl *fused_pair_tail_create(FusedImpl *pair, FusedImpl *tail) {
    const bool off = switches().no_pairtail;
    if (off || !pair || !tail || tail->kind != FusedImpl::TAIL) return nullptr;
    // the pair: a table group (dwpw_mm) or a single-pair run-time-geometry chain group
    OpImpl *dw = nullptr, *pw = nullptr;
    if (pair->kind == FusedImpl::DWPW) dw = pair->a, pw = pair->b;
    else if (fused_is_chain_single(pair)) dw = pair->chain.members[0].first, pw = pair->chain.members[0].second;
    const PairMatch m = match_dw3x3_pw1x1(dw, pw);
    // the kernel multiplies the taps' matrix-pipe image (a table kernel's or dw3x3_rt's) and has no filter zero point term
    if (!m || !m.f || !m.f->wmm || (dw->fast == OpImpl::DW_RT && dw->rt_wz)) return nullptr;
    if ((pw->fast != OpImpl::PW_MFMA && pw->fast != OpImpl::PW_RT) || (pw->fast == OpImpl::PW_RT && pw->rt_wz)) return nullptr;
    const OpSpec &d = *m.d, &q = *m.q;
    const k::TailArgs &t = tail->tail;
    if (!k::pair_tail_supported(d.H, d.W, d.C, q.N, t.N, t.ntaps) || d.sh != 1) return nullptr; // the compiled instances: stride 1
    if ((d.u8 ? 0x80 : 0) != t.xr) return nullptr;
    if (t.H != d.OH || t.W != d.OW || t.C != q.N || dw->device != tail->a->device) return nullptr; // the tail consumes the pair's output
    const int magic = (dw->magic_mode >= 1 && pw->magic_mode >= 1) ? 1 : 0; // bit-pattern epilogues, or the v_cvt form for both
    std::unique_ptr<FusedImpl> f = make_group(FusedImpl::PAIRTAIL, dw, tail->b, tail->c, k::pair_tail_name(d.H, d.C));
    k::PairTailArgs &a = f->pairtail.args;
    a.H = d.H, a.C = d.C, a.magic = magic;
    f->epi_mode = magic;
    pair_tail_operands(*f, a, dw, pw, *m.f, magic);
    a.tail = t;
    return f.release();
}

// The pair group in front of a pair + tail launch joins it (person_detect ops 23..30 in one launch; k_tail3.hip FRONT).  Borrows the
// pair + tail stage's device arrays (destroy it first); the front pair's own arrays are the group's.
FusedImpl *fused_front_pair_tail_create(FusedImpl *front, FusedImpl *pairtail) {
    if (switches().no_pair_front || !front || !pairtail || pairtail->kind != FusedImpl::PAIRTAIL || pairtail->pairtail.has_front) return nullptr;
    if (front->kind != FusedImpl::DWPW) return nullptr;
    OpImpl *dw = front->a, *pw = front->b;
    const PairMatch m = match_dw3x3_pw1x1(dw, pw);
    if (!m || dw->fast != OpImpl::DW_NHWC || pw->fast != OpImpl::PW_MFMA) return nullptr; // a table pair (its taps' matrix-pipe image: below)
    const OpSpec &d = *m.d, &q = *m.q;
    const k::PairTailArgs &t = pairtail->pairtail.args;
    if (!k::pair_front_supported(d.H, d.W, d.C, d.sh, q.N, t.H, t.C)) return nullptr;
    if (q.OH != t.H || q.OW != t.H || (d.u8 ? 0x80u : 0u) != (uint32_t)t.tail.xr || dw->device != pairtail->a->device) return nullptr;
    if (!m.f->wmm) return nullptr;
    // one epilogue form for the launch's four convolutions: the bit-pattern one needs it of all four
    const int magic = (dw->magic_mode >= 1 && pw->magic_mode >= 1) ? 1 : 0;
    if (magic != t.magic) return nullptr;
    std::unique_ptr<FusedImpl> f = make_group(FusedImpl::PAIRTAIL, dw, pairtail->b, pairtail->c, "pair_front_tail<6,6,128,2,256|3,3,256,2>");
    f->pairtail.args = t, f->pairtail.has_front = true, f->epi_mode = magic;
    pair_tail_operands(*f, f->pairtail.front, dw, pw, *m.f, magic);
    return f.release();
}

static std::unique_ptr<FusedImpl> quad_group(FusedImpl *p1, FusedImpl *p2, const k::DwPwArgs &a, const k::DwPwArgs &b, const char *name, bool mm) {
    const OpSpec &d1 = p1->a->s, &q1 = p1->b->s, &d2 = p2->a->s, &q2 = p2->b->s;
    std::unique_ptr<FusedImpl> f = make_group(FusedImpl::QUAD, p1->a, p2->b, nullptr, name);
    f->quad.args.a = a, f->quad.args.b = b, f->quad.mm = mm;
    f->epi_mode = std::min(pair_mode(a), pair_mode(b));
    f->quad.ops[0] = p1->a, f->quad.ops[1] = p1->b, f->quad.ops[2] = p2->a, f->quad.ops[3] = p2->b;
    const int shp[10] = {d1.H, d1.W, d1.C, d1.sh, q1.N, d2.H, d2.W, d2.C, d2.sh, q2.N};
    for (int i = 0; i < 10; ++i) f->quad.shape[i] = shp[i];
    return f;
}
// Two consecutive DepthwiseConv2D 3x3 + Conv2D 1x1 pair groups as one kernel (k_quad.hip), when a quad kernel exists for the two
// shapes.
FusedImpl *fused_quad_create(FusedImpl *p1, FusedImpl *p2) {
    const bool off = switches().no_quad;
    if (off || !p1 || !p2 || p1->kind != FusedImpl::DWPW || p2->kind != FusedImpl::DWPW) return nullptr;
    const OpSpec &d1 = p1->a->s, &q1 = p1->b->s, &d2 = p2->a->s, &q2 = p2->b->s;
    if (p1->a->device != p2->a->device || d1.u8 != d2.u8) return nullptr;
    if (d2.H != q1.H || d2.W != q1.W || d2.C != q1.N) return nullptr; // the second pair consumes the first pair's output
    if (k::quad_mm_shape(d1.H, d1.W, d1.C, d1.sh, q1.N, d2.H, d2.W, d2.C, d2.sh, q2.N)) {
        if (switches().no_quad_mm) return nullptr;
        // the pairs' own blocks (dwpw_mm's: matrix-pipe depthwise weights, pw_mfma-layout pointwise weights, patch tables); one
        // epilogue mode for the launch: the single-fma form if both pairs run it, else the two-rounding forms for both
        k::DwPwArgs a = p1->dwpw, b = p2->dwpw;
        if (pair_mode(a) != 3 || pair_mode(b) != 3) a = pair_args(p1->a, p1->b, 0), b = pair_args(p2->a, p2->b, 0);
        if (!a.dw.wmm || !a.pw.wprep || !b.dw.wmm || !b.pw.wprep) return nullptr;
        if (!a.dw.magic || !a.pw.magic || !b.dw.magic || !b.pw.magic) return nullptr; // bit-pattern epilogues
        return quad_group(p1, p2, a, b, "quad_mm<12,12,64,1,64|12,12,64,2,128>", true).release();
    }
    const char *nm = k::quad_name(d1.H, d1.W, d1.C, d1.sh, q1.N, d2.H, d2.W, d2.C, d2.sh, q2.N);
    if (!nm) return nullptr;
    // (the single-fma form needs it of all four operators)
    const bool fma = p1->a->fma_strict() && p1->b->fma_strict() && p2->a->fma_strict() && p2->b->fma_strict();
    const k::DwPwArgs a = pair_args(p1->a, p1->b, fma ? 1 : 0), b = pair_args(p2->a, p2->b, fma ? 1 : 0);
    if (!a.dw.wmm || !a.pw.wrr || !b.dw.wmm || !b.pw.wrr) return nullptr;
    if (!a.dw.magic || !a.pw.magic || !b.dw.magic || !b.pw.magic) return nullptr; // bit-pattern epilogues
    return quad_group(p1, p2, a, b, nm, false).release();
}

// The network's one-input-channel stem in front of a quad: five operators in one launch (k_quad.hip, STEM instance).  The quad
// itself stays (mf_model_run_until, and the f32 entry point, whose boundary quantisation is fused into the stem kernel).
FusedImpl *fused_quad_stem_create(OpImpl *stem, FusedImpl *quad) {
    const bool off = switches().no_penta;
    if (off || !stem || !quad || quad->kind != FusedImpl::QUAD || quad->quad.args.stem || stem->fast != OpImpl::DW_STEM) return nullptr;
    const OpSpec &t = stem->s, &d1 = quad->a->s;
    if (stem->device != quad->a->device || t.u8 != d1.u8 || stem->force_generic) return nullptr;
    if (t.OH != d1.H || t.OW != d1.W || t.N != d1.C || t.sh != 2 || t.sw != 2 || t.C != 1) return nullptr; // pair A consumes the stem's output
    const int *q = quad->quad.shape;
    const char *nm = k::quad_stem_name(t.H, t.W, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9]);
    if (!nm || !stem->stem.magic) return nullptr;
    std::unique_ptr<FusedImpl> f = make_group(FusedImpl::QUAD, stem, quad->b, nullptr, nm);
    k::QuadArgs &a = f->quad.args;
    a = quad->quad.args;
    for (int i = 0; i < 10; ++i) f->quad.shape[i] = q[i];
    // five operators, one epilogue mode: the single-fma form if all five have it, else everyone's two-rounding constants
    OpImpl *const *qo = quad->quad.ops;
    const bool fma = stem->fma_strict() && qo[0]->fma_strict() && qo[1]->fma_strict() && qo[2]->fma_strict() && qo[3]->fma_strict();
    a.a = pair_args(qo[0], qo[1], fma ? 1 : 0), a.b = pair_args(qo[2], qo[3], fma ? 1 : 0);
    k::DwStemArgs sa = stem->stem;
    if (fma) sa.use_fma();
    std::vector<uint32_t> tab(152);
    for (int l = 0; l < 64; ++l) tab[(size_t)2 * l] = sa.wmm[l][0], tab[(size_t)2 * l + 1] = sa.wmm[l][1];
    for (int c = 0; c < 8; ++c) {
        memcpy(&tab[(size_t)128 + c], &sa.A[c], 4);
        memcpy(&tab[(size_t)136 + c], &sa.S[c], 4);
        memcpy(&tab[(size_t)144 + c], &sa.Kc[c], 4);
    }
    a.stem = (const uint32_t *)keep(*f, tab.data(), tab.size() * 4);
    a.stem_izp4 = sa.izp4, a.stem_lo = sa.lo_f, a.stem_hi = sa.hi_f, a.stem_magic = sa.magic;
    // the f32 entry (model_groups.cpp sets the stem's input quantisation before the groups are built): same launch, f32 image in
    a.in_scale = sa.in_scale, a.in_zp_f = sa.in_zp_f, a.in_sat_lo = sa.in_sat_lo, a.in_sat_hi = sa.in_sat_hi;
    a.in_rcp = sa.in_rcp, a.in_xr4 = sa.in_xr4, a.in_fast = sa.in_fast, a.f32_ok = stem->accepts_f32 ? 1 : 0;
    f->epi_mode = std::min(std::min(pair_mode(a.a), pair_mode(a.b)), sa.magic);
    return f.release();
}

} // namespace mf
