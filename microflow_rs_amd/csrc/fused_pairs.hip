// fused_pairs.hip -- one DepthwiseConv2D 3x3 + Conv2D 1x1 pair (or a run of them: chain_rt) as one launch.  fused_create at the end
// of the file states the order in which a pair is offered to the four builders.  Host code only; the kernels are in k_*.hip.
#include <cstdio>

#include "fused_impl.hpp"

namespace mf {

// ---- a table pair (kernels.hpp: dwpw_name; k_fused_mm.hip) ----
static std::unique_ptr<FusedImpl> table_pair_create(OpImpl *dw, OpImpl *pw) {
    if (!dw || !pw || dw->fast != OpImpl::DW_NHWC || pw->fast != OpImpl::PW_MFMA) return nullptr;
    const OpSpec &d = dw->s, &q = pw->s;
    // the pointwise conv must consume exactly the depthwise output tensor
    if (q.H != d.OH || q.W != d.OW || q.C != d.N || dw->device != pw->device) return nullptr;
    const char *nm = k::dwpw_name(d.H, d.W, d.C, d.sh, q.N);
    if (!nm) return nullptr;
    std::unique_ptr<FusedImpl> f = make_group(FusedImpl::DWPW, dw, pw, nullptr, nm);
    f->dwpw = pair_args(dw, pw, 2);
    if (pair_mode(f->dwpw) == 3 && (dw->fma_patch.n || pw->fma_patch.n)) {
        // patched accumulators: dwpw_mm applies them (launch_dwpw routes there), from one record per tile.  Its depthwise tiles are the
        // aligned 16-channel groups; pointwise tile (blk, tt) holds channels blk NB + pg NB / 4 + 4 tt + i in lane group pg (k_fused_mm.hip)
        const int NB = q.N < 64 ? q.N : 64, TB = NB / 16, NQ = d.C / 16;
        std::vector<k::EpiPatchRec> tab((size_t)NQ + (size_t)(q.N / NB) * TB, k::EpiPatchRec{0, 0});
        bool ok = d.C >= 16 && patch_table(dw->fma_patch, tab, 0, [&](int ch, int &reg, int &grp) { return reg = ch & 3, grp = (ch >> 2) & 3, ch >> 4; });
        ok = ok && patch_table(pw->fma_patch, tab, (size_t)NQ, [&](int ch, int &reg, int &grp) {
                 const int rel = ch % NB, within = rel % (NB / 4);
                 return reg = within & 3, grp = rel / (NB / 4), (ch / NB) * TB + within / 4;
             });
        if (ok) {
            const k::EpiPatchRec *t = (const k::EpiPatchRec *)keep(*f, tab.data(), tab.size() * sizeof(k::EpiPatchRec));
            if (dw->fma_patch.n) f->dwpw.dw.patch = t;
            if (pw->fma_patch.n) f->dwpw.pw.patch = t + NQ;
            f->name = k::dwpw_mm_name(d.H, d.W, d.C, d.sh, q.N);
        } else {
            f->dwpw = pair_args(dw, pw, 1); // (both strict, or the two-rounding forms)
        }
    }
    f->epi_mode = pair_mode(f->dwpw);
    return f;
}

// ---- run-time-geometry chains (k_chain.hip) ----
static bool chain_enabled() {
    const bool off = switches().no_chain;
    return !off;
}
// a DepthwiseConv2D 3x3 + Conv2D 1x1 pair the chain kernel can run: any H / W, C % 16 == 0, N % 16 == 0
static int chain_superpixel(int C) {
    const bool no_sp = switches().chain_no_sp; // A/B: only C == 8 stride 1 (round 4's first form) below 16 channels
    if (C % 16 == 0) return 1;
    if (C == 8 || (!no_sp && (C == 4 || C == 2))) return 16 / C;
    return 0;
}
static bool chain_pair_ok(const OpImpl *dw, const OpImpl *pw) {
    const PairMatch m = match_dw3x3_pw1x1(dw, pw);
    if (!m || dw->force_generic || pw->force_generic) return false; // (an operator sent to the generic kernels stays a launch of its own)
    const OpSpec &d = *m.d, &q = *m.q;
    // the depthwise's taps in matrix-pipe form come from dw3x3_rt's or a table kernel's image; none exists with filter zero points
    if (!m.f) return false;
    const int P = chain_superpixel(d.C);  // pixels per 16-channel "superpixel" (1: C % 16 == 0; 0: no such form)
    if ((P == 1 && !m.f->wmm) || (dw->fast == OpImpl::DW_RT && dw->rt_wz)) return false;
    if (P == 0 || d.W % (P * d.sh) != 0) return false; // (C < 16: whole superpixels in and out, see chain_geom)
    if (P > 1 && d.sh == 2 && switches().chain_no_sp) return false;
    if ((P * q.N) % 16 != 0) return false; // whole output tiles
    // the 1x1 alone on pw_rt or pw_mfma (anything else is a shape class of its own), and no filter zero points: the kernel has no such term
    if (pw->fast != OpImpl::PW_RT && pw->fast != OpImpl::PW_MFMA) return false;
    if (pw->fast == OpImpl::PW_RT && pw->rt_wz) return false;
    if ((dw->magic_mode < 1 || pw->magic_mode < 1) && q.C < 256) return false; // (the v_cvt epilogue exists for four k steps only: launch_chain)
    return true;
}
// The geometry the planner sees.  C < 16 (the first pairs of a MobileNet-v1-shaped network: C = 8, or 4 and 8 at width 0.5): P = 16 / C
// adjacent pixels form one 16-channel "superpixel" -- the depthwise taps are build_dw_mm_weights_sp (MFMA rows = (pixel of the
// superpixel, channel), filter-row blocks = neighbouring superpixels, either stride), the 1x1 convolution is block diagonal over the P
// pixels -- so the pair IS a 16-channel pair of 1/P the width with P times the outputs.  Such a pair only ever runs alone (its output
// tensor is not in the next pair's units).
k::ChainGeom chain_geom(const OpImpl *dw, const OpImpl *pw) {
    const OpSpec &d = dw->s;
    const int P = chain_superpixel(d.C);
    if (P > 1) return k::ChainGeom{d.H, d.W / P, 16, d.sh, d.OH, d.OW / P, P * pw->s.N, dw_fast(dw)->izp4};
    return k::ChainGeom{d.H, d.W, d.C, d.sh, d.OH, d.OW, pw->s.N, dw_fast(dw)->izp4};
}
std::unique_ptr<FusedImpl> chain_create(const std::pair<OpImpl *, OpImpl *> *mem, int n, int force_G, int force_dbuf) {
    if (!chain_enabled() || n < 1 || n > k::CHAIN_MAX) return nullptr;
    std::vector<k::ChainGeom> geo((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (!chain_pair_ok(mem[i].first, mem[i].second)) {
            if (n == 1 && switches().chain_verbose)
                fprintf(stderr, "[microflow_amd] not a chain pair: %dx%dx%d s%d (kernels %s, %s; epilogue modes %d, %d)\n", mem[i].first->s.H, mem[i].first->s.W,
                        mem[i].first->s.C, mem[i].first->s.sh, mem[i].first->fast_name.c_str(), mem[i].second->fast_name.c_str(), mem[i].first->magic_mode, mem[i].second->magic_mode);
            return nullptr;
        }
        if (mem[i].first->device != mem[0].first->device || mem[i].first->s.u8 != mem[0].first->s.u8) return nullptr;
        if (mem[i].first->s.C < 16 && n != 1) return nullptr;
        geo[(size_t)i] = chain_geom(mem[i].first, mem[i].second);
    }
    std::vector<k::ChainPair> tab((size_t)n);
    std::unique_ptr<FusedImpl> c = make_group(FusedImpl::CHAIN, mem[0].first, mem[n - 1].second, nullptr, "");
    k::ChainArgs &a = c->chain.args;
    if (!k::chain_plan(geo.data(), n, tab.data(), a, 150 * 1024, force_G, force_dbuf)) {
        if (n == 1 && force_G == 0 && switches().chain_verbose)
            fprintf(stderr, "[microflow_amd] no chain plan for %dx%dx%d s%d -> %d\n", geo[0].H, geo[0].W, geo[0].C, geo[0].S, geo[0].N);
        return nullptr;
    }
    int magic = 2;
    std::string name = "chain_rt<";
    for (int i = 0; i < n; ++i) {
        OpImpl *dw = mem[i].first, *pw = mem[i].second;
        k::ChainPair &t = tab[(size_t)i];
        t.dw_wmm = dw_fast(dw)->wmm;
        set_pair_consts(t, *dw_fast(dw), pw->conv);
        const OpSpec &q = pw->s;
        const int group = chain_superpixel(dw->s.C); // pixels per MFMA column / product row
        const std::vector<int8_t> prep = wimage::build_pw_rt_reg_weights(pw->h_w.data(), q.C, q.N, group, t.TB, t.NBLK); // [N][1][1][C], i8 domain
        t.pw_w = keep(*c, prep.data(), prep.size());
        if (group > 1) {
            // the taps in superpixel form (from the depthwise weights as uploaded: [3][3][C], i8 domain)
            const std::vector<int8_t> sp = wimage::build_dw_mm_weights_sp(dw->h_w.data(), dw->s.C, dw->s.sh);
            t.dw_wmm = keep(*c, sp.data(), sp.size());
            // the constants of MFMA row (pixel of the superpixel, channel) are the channel's: `group` copies of the arrays
            auto copies = [&](const auto &src) { // (a vector of 4-byte constants, one per channel)
                auto h = src;
                h.resize((size_t)group * src.size());
                for (size_t e = src.size(); e < h.size(); ++e) h[e] = h[e % src.size()];
                return keep(*c, h.data(), h.size() * 4);
            };
            t.dwA = (const float *)copies(dw->h_A), t.dwS = (const float *)copies(dw->h_S), t.dwK = (const int *)copies(dw->h_Kc);
            t.pwA = (const float *)copies(pw->h_A), t.pwS = (const float *)copies(pw->h_S), t.pwK = (const int *)copies(pw->h_Kc);
        }
        upload_rtab(*c, t);
        magic = std::min(magic, std::min(dw->magic_mode, pw->magic_mode));
        name += (i ? "|" : "") + pair_label(dw->s, q);
        c->chain.members.push_back(mem[i]);
    }
    name += ";G" + std::to_string(a.G) + ">";
    c->name = name;
    if (switches().chain_verbose) fprintf(stderr, "[microflow_amd] %s est %.4f us/image/CU lds %d nwave %d dbuf %d\n", name.c_str(), a.est_us_per_image, a.lds_bytes, a.nwave, a.dbuf);
    a.pairs = (const k::ChainPair *)keep(*c, tab.data(), tab.size() * sizeof(k::ChainPair));
    if (magic == 0 && a.KSC != 4) return nullptr;
    a.magic = magic, a.xr = mem[0].first->s.u8 ? 0x80 : 0;
    c->epi_mode = magic;
    a.queue = (int *)mem[0].first->d_queue.p, a.qlaunch = &mem[0].first->q_launches;
    return c;
}
// second level: `n` consecutive single-pair chain groups as ONE chain (nullptr: no plan fits)
FusedImpl *fused_chain_create(FusedImpl *const *groups, int n, int force_G) {
    std::vector<std::pair<OpImpl *, OpImpl *>> mem;
    for (int i = 0; i < n; ++i) {
        if (!fused_is_chain_single(groups[i])) return nullptr;
        mem.push_back(groups[i]->chain.members[0]);
    }
    return chain_create(mem.data(), n, force_G).release();
}
bool fused_is_chain_single(const FusedImpl *f) { return f && f->kind == FusedImpl::CHAIN && f->chain.members.size() == 1; }

// the table pairs, then chain_rt (MF_CHAIN_ALL, tests / A-B: the chain kernel on table shapes too)
static std::unique_ptr<FusedImpl> table_or_chain_create(OpImpl *dw, OpImpl *pw) {
    if (dw && pw && (switches().chain_all || dw->fast != OpImpl::DW_NHWC || pw->fast != OpImpl::PW_MFMA ||
                     !k::dwpw_name(dw->s.H, dw->s.W, dw->s.C, dw->s.sh, pw->s.N))) {
        const std::pair<OpImpl *, OpImpl *> one(dw, pw);
        if (std::unique_ptr<FusedImpl> c = chain_create(&one, 1)) return c;
    }
    return table_pair_create(dw, pw);
}

// ---- one pair of any image size in row bands (k_pair_band.hip; 256 < C <= 512: k_pair_band_deep.hip): fused_create's last resort ----
// Takes a pair only when the table kernels and chain_create have both declined AND the pair is too large for chain_rt at one image
// per step (pair_band_plan's size condition): chain_rt keeps every pair it takes, and a small pair chain_plan refuses for another
// reason (12x12x48 -> 48: three output tiles) stays two operators.  Does not depend on which kernel the 1x1 runs on its own: the
// operand image is built here from its host weights.
// Above 256 input channels there is no size condition (chain_rt never takes such a pair): pair_band_deep_plan takes whatever fits.
static std::unique_ptr<FusedImpl> pair_band_create(OpImpl *dw, OpImpl *pw) {
    const PairMatch m = match_dw3x3_pw1x1(dw, pw);
    if (switches().no_pair_band || !m || dw->force_generic || pw->force_generic) return nullptr; // (generic operators stay launches of their own)
    const OpSpec &d = *m.d, &q = *m.q;
    if (d.sh == 2 && d.W % 2 != 0) return nullptr; // (the plans' stride-2 column units: pair_band_plan)
    if (d.C % 16 != 0 || d.C < 16 || d.C > 512 || q.N % 16 != 0 || q.N < 16 || q.N > 1024) return nullptr; // the two plans' channel ranges
    // the depthwise member: dw3x3_rt or a table kernel with its taps in matrix-pipe form (none with filter zero points)
    if (!m.f || !m.f->wmm || (dw->fast == OpImpl::DW_RT && dw->rt_wz)) return nullptr;
    // the 1x1: whatever it runs alone, its filter zero points must be zero in the i8 domain
    if (pw->h_w.size() != (size_t)q.N * q.C || pw->h_A.size() != (size_t)q.N) return nullptr;
    for (int32_t z : pw->h_wzp)
        if (z != 0) return nullptr;
    std::unique_ptr<FusedImpl> c = make_group(FusedImpl::PAIRBAND, dw, pw, nullptr, "");
    k::PairBandArgs &a = c->pairband;
    const bool deep = d.C > 256; // 256 < C <= 512: pair_band_deep_rt's plan (k_pair_band_deep.hip: eight k steps, no lower size bound)
    if (!(deep ? k::pair_band_deep_plan(m.geom, a) : k::pair_band_plan(m.geom, a))) return nullptr;
    // Classes measured NOT faster than the operators' own launches (profiles/r07/time_pair_band.txt) stay layer-wise:
    //   C < 64 -- 112x112x32 -> 64 ran x1.01, 96x96x32 -> 64 x1.13 inside a spread of 0.16 - 0.28;
    //   a plan that needs more than half a CU's LDS with fewer than four k steps -- eight waves alone on a CU that the same kernel
    //   fills with sixteen elsewhere: 56x56x128 s2 -> 256 ran x1.04 inside a spread of 0.09;
    //   four k steps (one workgroup per CU: 180 registers) up to 256 outputs, where the 1x1 alone runs a weights-in-registers kernel --
    //   28x28x256 -> 256 ran x1.00 with 4-row bands, x1.09 with 8-row bands inside a spread of 0.11 (-> 512 runs x1.88).
    //   eight k steps (pair_band_deep_rt; profiles/r08/time_pair_band_deep.txt) up to 256 outputs, the same class: 14x14x512 -> 256
    //   ran 0.496 ms against 0.555 (dw3x3_rt + pw_rt<512,256>), x1.12 with spreads of 0.104 and 0.106 -- a margin a rerun can eat.  Every
    //   other class measured there (N >= 320, where the 1x1 alone runs conv_gemm_rt) ran x1.61 - x2.78 and stays.
    if (d.C < 64 || (a.wgs == 1 && a.KSC < 4) || (a.KSC >= 4 && q.N <= 256)) return nullptr;
    const int magic = std::min(dw->magic_mode, pw->magic_mode);
    if (!deep && !k::pair_band_instance(a.KSC, magic)) return nullptr; // (no compiled instance: the pair stays layer-wise)
    a.dw_wmm = m.f->wmm;
    set_pair_consts(a, *m.f, pw->conv);
    const std::vector<int8_t> prep = wimage::build_pw_rt_reg_weights(pw->h_w.data(), q.C, q.N, 1, a.TB, a.NBLK); // [N][1][1][C], i8 domain
    a.pw_w = keep(*c, prep.data(), prep.size());
    a.magic = magic, a.xr = d.u8 ? 0x80 : 0;
    a.queue = (int *)dw->d_queue.p, a.qlaunch = &dw->q_launches;
    c->epi_mode = magic;
    c->name = std::string(deep ? "pair_band_deep_rt<" : "pair_band_rt<") + pair_label(d, q) + ";RB" + std::to_string(a.RB) + ";NB" + std::to_string(a.NB) + ">";
    if (switches().chain_verbose)
        fprintf(stderr, "[microflow_amd] band group %s: tile %d rows x %d B%s, MID %d B, lds %d B, %d workgroup%s per CU, %d x %d output tiles, mode %d\n", c->name.c_str(), a.TR,
                a.ROW, a.dbuf ? " (two)" : "", a.mid_bytes, a.lds_bytes, a.wgs, a.wgs == 1 ? "" : "s", a.NBLK, a.TB, magic);
    return c;
}

// ---- one pair whose filters carry zero points (k_pair_wz.hip): after the table pairs, chain_rt and the band kernels have all declined ----
// Every other fused launch refuses a filter zero point away from zero in the i8 domain -- every classic asymmetric-uint8 model, and
// per-channel zero points on i8 -- so such a pair used to run dw3x3_rt<S,wzp> + pw_rt<K,N,wzp> with its intermediate tensor through
// HBM.  This group takes exactly those pairs (at least one member with a non-zero zero point: a pair without keeps the group it has
// today), on chain_plan's single-pair plan.  A kind of its own: the stage, quad, tail and chain-partition code all answer "no" to it.
static std::unique_ptr<FusedImpl> pair_wz_create(OpImpl *dw, OpImpl *pw) {
    const PairMatch m = match_dw3x3_pw1x1(dw, pw);
    if (switches().no_pair_wz || !m || dw->force_generic || pw->force_generic) return nullptr; // (generic operators stay launches of their own)
    const OpSpec &d = *m.d, &q = *m.q;
    if (d.W % d.sh != 0) return nullptr; // (chain_plan's stride-2 column units)
    if (d.C % 16 != 0 || d.C < 16 || d.C > 256 || q.N % 16 != 0 || q.N < 16) return nullptr; // chain_rt's channel range, whole tiles
    // the members' own launches: dw3x3_rt or a table kernel, pw_rt or pw_mfma (anything else is a shape class of its own)
    if (!m.f) return nullptr;
    if (pw->fast != OpImpl::PW_RT && pw->fast != OpImpl::PW_MFMA) return nullptr;
    if (dw->h_w.size() != (size_t)9 * d.C || pw->h_w.size() != (size_t)q.N * q.C || dw->h_wzp.size() != (size_t)d.C || pw->h_wzp.size() != (size_t)q.N) return nullptr;
    const bool wz = !std::all_of(dw->h_wzp.begin(), dw->h_wzp.end(), [](int32_t z) { return z == 0; }) ||
                    !std::all_of(pw->h_wzp.begin(), pw->h_wzp.end(), [](int32_t z) { return z == 0; });
    if (!wz) return nullptr; // (zero filter zero points: the pair keeps exactly the group -- or the two launches -- it has today)
    std::unique_ptr<FusedImpl> c = make_group(FusedImpl::PAIRWZ, dw, pw, nullptr, "");
    k::ChainArgs &a = c->pairwz.c;
    k::ChainPair t{};
    if (!k::chain_plan(&m.geom, 1, &t, a, 150 * 1024)) {
        if (switches().chain_verbose) fprintf(stderr, "[microflow_amd] no chain plan for the zero-point pair %dx%dx%d s%d -> %d\n", d.H, d.W, d.C, d.sh, q.N);
        return nullptr;
    }
    // chain_plan weighs a step's fixed cost against TWO workgroups per CU while the LDS allows them.  From two k steps on pair_wz_rt's
    // registers (134 - 179) allow one, which then has the whole LDS: twice the images per step where the plan still fits
    // (profiles/r09/time_pair_wz.txt: 6x6x128 -> 128 0.106 -> 0.093 ms).  One k step keeps the plan's choice: its resident instances
    // hold 116 registers, two workgroups per CU (24x24x32 s2 -> 64 ran 0.127 ms so, 0.155 ms with twice the images in one workgroup).
    for (int gm = a.KSC >= 2 ? switches().pair_wz_gmul : 1; gm > 1; gm /= 2) {
        k::ChainPair t2{};
        k::ChainArgs a2{};
        if (!k::chain_plan(&m.geom, 1, &t2, a2, 150 * 1024, a.G * gm)) continue;
        t = t2, a = a2;
        break;
    }
    const int magic = std::min(dw->magic_mode, pw->magic_mode);
    if (!k::pair_wz_instance(a.KSC, magic)) return nullptr; // (no compiled instance: the pair stays layer-wise)
    k::pair_wz_split(t); // (the plan's unit ranges are for chain_rt's 8 or 16 waves; pair_wz_rt has 8)
    a.nwave = 8, a.resident = (t.single_q && !switches().chain_no_res) ? 1 : 0; // (MF_CHAIN_NO_RES: A/B, as chain_rt's)
    // the depthwise taps in matrix-pipe form, from the weights as uploaded ([3][3][C], i8 domain): route_dw_rt builds no such image
    // for an operator with filter zero points
    const std::vector<int8_t> taps = wimage::build_dw_mm_weights(dw->h_w.data(), d.C);
    t.dw_wmm = keep(*c, taps.data(), taps.size());
    const std::vector<int8_t> prep = wimage::build_pw_rt_reg_weights(pw->h_w.data(), q.C, q.N, 1, t.TB, t.NBLK); // [N][1][1][C], i8 domain
    t.pw_w = keep(*c, prep.data(), prep.size());
    set_pair_consts(t, dw->conv, pw->conv);
    upload_rtab(*c, t);
    // the two ones images (wimage.cpp): the all-ones filter's tap image -- its three filter rows are the same 1 KiB, the kernel keeps
    // one -- and the 1x1's tile of ones, zero beyond C
    const std::vector<int8_t> dones = wimage::build_dw_ones_image();
    c->pairwz.dw_ones = keep(*c, dones.data(), 1024);
    const std::vector<int8_t> pones = wimage::build_pw_ones_tile(q.C);
    c->pairwz.pw_ones = keep(*c, pones.data(), pones.size());
    c->pairwz.dw_wzp = dw->conv.wzp, c->pairwz.pw_wzp = pw->conv.wzp;
    a.pairs = (const k::ChainPair *)keep(*c, &t, sizeof(t));
    a.magic = magic, a.xr = d.u8 ? 0x80 : 0;
    a.queue = (int *)dw->d_queue.p, a.qlaunch = &dw->q_launches;
    c->epi_mode = magic;
    c->name = "pair_wz_rt<" + pair_label(d, q) + ";G" + std::to_string(a.G) + ">";
    if (switches().chain_verbose)
        fprintf(stderr, "[microflow_amd] zero-point group %s: lds %d B, dbuf %d, %d x %d output tiles, %d k step%s, mode %d\n", c->name.c_str(), a.lds_bytes, a.dbuf, t.NBLK, t.TB, t.KS,
                t.KS == 1 ? "" : "s", magic);
    return c;
}

// ---- a 1x1 expand + depthwise 3x3 + 1x1 project block in row bands (k_block_band.hip): the model's second level, over the pair's group ----
// Every operand image is built here from the members' host copies and every constant array is the member's own (the project's padded
// to whole 16-channel tiles where N % 16 != 0), so the block does not depend on which kernels the members run alone.
static constexpr int BLOCK_LIMIT_STEPS = 512;
FusedImpl *fused_block_create(OpImpl *ex, OpImpl *dw, OpImpl *pw, bool pair_grouped) {
    if (switches().no_expand_block) return nullptr;
    const BlockMatch m = match_expand_block(ex, dw, pw);
    if (!m) return nullptr;
    const OpSpec &e = ex->s, &d = *m.pair.d, &q = *m.pair.q;
    const int CI = m.CI, E = d.C, N = q.N;
    if (ex->h_w.size() != (size_t)E * CI || dw->h_w.size() != (size_t)9 * E || pw->h_w.size() != (size_t)N * E) return nullptr;
    if (ex->h_A.size() != (size_t)E || dw->h_A.size() != (size_t)E || pw->h_A.size() != (size_t)N || pw->h_S.size() != (size_t)N || pw->h_Kc.size() != (size_t)N) return nullptr;
    std::unique_ptr<FusedImpl> c = make_group(FusedImpl::BLOCK, ex, dw, pw, "");
    k::BlockBandArgs &bb = c->block;
    k::PairBandArgs &a = bb.b;
    if (!k::block_band_plan(m.pair.geom, CI, bb)) return nullptr;
    // Classes measured NOT faster than the launches they replace by more than the spread of the repeats (profiles/r13/time_expand_block.txt,
    // DESIGN 4.16) keep those launches:
    //   four k steps of E at stride 1 on a plan that needs more than half a CU's LDS -- eight waves alone on a CU, 6-row bands that
    //   compute the expand of 8 rows: 56x56x24 -> 144 -> 24 ran 0.624 ms against 0.590 (x0.95);
    //   four k steps of E and less than one 16-pixel chunk of output per image -- a step is three barriers and a DMA for 36 pixels:
    //   6x6x32 -> 192 s2 -> 64 ran 0.173 ms against 0.112 (x0.64).
    if (a.KSC == 4 && ((d.sh == 1 && a.wgs == 1) || d.OH * d.OW < 16)) return nullptr;
    const int magic = std::min(ex->magic_mode, std::min(dw->magic_mode, pw->magic_mode));
    if (!k::block_band_instance(a.KSC, bb.KSI, magic)) return nullptr; // (no compiled instance: the block keeps its launches)
    const std::vector<int8_t> exw = wimage::build_pw_rt_reg_weights(ex->h_w.data(), CI, E, 1, 1, E / 16); // [E][1][1][CI], i8 domain
    bb.ex_w = keep(*c, exw.data(), exw.size());
    bb.exA = ex->conv.A, bb.exS = ex->conv.S, bb.exK = ex->conv.Kc, bb.ex_lo = ex->conv.lo_f, bb.ex_hi = ex->conv.hi_f;
    const std::vector<int8_t> taps = wimage::build_dw_mm_weights(dw->h_w.data(), E); // [3][3][E], i8 domain
    a.dw_wmm = keep(*c, taps.data(), taps.size());
    const std::vector<int8_t> prep = wimage::build_pw_rt_reg_weights(pw->h_w.data(), E, N, 1, a.TB, a.NBLK); // [N][1][1][E]; rows past N are zero
    a.pw_w = keep(*c, prep.data(), prep.size());
    set_pair_consts(a, dw->conv, pw->conv);
    if (N % 16 != 0) { // a lane fetches the constants of its four channels whether or not they are below N
        const size_t np = (size_t)a.TB * a.NBLK * 16;
        auto padded = [&](const auto &src) {
            auto h = src;
            h.resize(np, 0);
            return keep(*c, h.data(), np * 4);
        };
        a.pwA = (const float *)padded(pw->h_A), a.pwS = (const float *)padded(pw->h_S), a.pwK = (const int *)padded(pw->h_Kc);
    }
    // Classes in which the one launch wins only while the launches it replaces cannot fill the chip (profiles/r13/time_expand_block.txt,
    // the sweep) run it up to a batch limit and the launches they had above it (fused_batch_ok, as conv1_fc_rt's limit):
    //   one k step of E (E <= 64), and four k steps at stride 2 with N <= 32: up to one round of the 512 resident workgroups, 512 / NB images;
    //   a quarter of that where the depthwise + project pair has a launch of its own (pw_rt + chain_rt / pair_band_rt: two launches
    //   are replaced, not three).
    if (a.KSC == 1 || (a.KSC == 4 && d.sh == 2 && N <= 32)) c->block_max_batch = (size_t)std::max(1, (pair_grouped ? BLOCK_LIMIT_STEPS / 4 : BLOCK_LIMIT_STEPS) / a.NB);
    a.magic = magic, a.xr = d.u8 ? 0x80 : 0;
    a.queue = (int *)ex->d_queue.p, a.qlaunch = &ex->q_launches;
    c->epi_mode = magic;
    c->name = "block_band_rt<" + std::to_string(e.H) + "x" + std::to_string(e.W) + "x" + std::to_string(CI) + "-" + std::to_string(E) + (d.sh == 2 ? "s2" : "") + "-" + std::to_string(N) +
              ";RB" + std::to_string(a.RB) + ";NB" + std::to_string(a.NB) + ">";
    if (switches().chain_verbose)
        fprintf(stderr, "[microflow_amd] block group %s: input band %d B, tile %d rows x %d B, MID %d B, lds %d B, %d workgroup%s per CU, %d x %d output tiles, k steps %d / %d, mode %d, batch limit %zu\n",
                c->name.c_str(), bb.in_bytes, a.TR, a.ROW, a.mid_bytes, a.lds_bytes, a.wgs, a.wgs == 1 ? "" : "s", a.NBLK, a.TB, bb.KSI, a.KSC, magic, c->block_max_batch);
    return c.release();
}

// A pair as one launch.  THE ORDER: a table pair or chain_rt (chain_rt first where no table kernel exists or under MF_CHAIN_ALL), then
// the band kernels, then -- only ever for a pair with filter zero points, which the others refuse -- pair_wz_rt.
FusedImpl *fused_create(OpImpl *dw, OpImpl *pw) {
    std::unique_ptr<FusedImpl> f = table_or_chain_create(dw, pw);
    if (!f) f = pair_band_create(dw, pw);
    if (!f) f = pair_wz_create(dw, pw);
    return f.release();
}

} // namespace mf
