// fused.hip -- fused groups: consecutive prepared operators (ops.hip) as one launch.  A group borrows its operators' device
// arrays and builds the operand images its kernel needs beyond them from the operators' host copies (ops_impl.hpp).  At the
// end of the file: the planner that cuts a run of run-time-geometry pairs into chain launches, by cost model or by measurement.
// Host code only; the kernels are in k_*.hip.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>

#include "ops_impl.hpp"
#include "wimage.hpp"

namespace mf {

struct FusedImpl {
    enum Kind { DWPW, TAIL, FCSM, STAGE, DWFC, PAIRTAIL, QUAD, CHAIN, FCCHAIN, POOLFC, PAIRBAND, PAIRWZ, CONV1FC } kind;
    OpImpl *a, *b, *c;
    k::DwPwArgs dwpw;
    k::TailArgs tail;
    std::string name;
    // STAGE: the whole late stage in one kernel
    k::StageArgs stage{};
    int stage_pairs = 0;
    std::vector<std::unique_ptr<DevBuf>> stage_w; // the stage kernel's own operand arrays and its pair table
    // DWFC: one-input-channel depthwise -> FullyConnected -> Softmax in one kernel (operand tables in stage_w)
    k::DwFcArgs dwfc{};
    // PAIRTAIL: the last pair + the tail in one kernel (operand arrays in stage_w)
    k::PairTailArgs pairtail{};
    k::PairFrontArgs pairfront{}; // ... with the pair in front of it in the same launch (has_front; k_tail3.hip FRONT)
    bool has_front = false;
    // QUAD: two consecutive pairs in one kernel (k_quad.hip); a = the first pair's depthwise, b = the second pair's conv
    k::QuadArgs quad{};
    bool quad_mm = false; // the C = 64 quad (k_quad_mm.hip): intermediate tensors through LDS, the pairs' dwpw_mm argument blocks
    int quad_shape[10] = {0};
    OpImpl *quad_ops[4] = {nullptr, nullptr, nullptr, nullptr}; // the two pairs' operators (the stem variant rebuilds the blocks from them)
    // CHAIN: 1 .. CHAIN_MAX consecutive pairs of any geometry in one launch (k_chain.hip); table and weights in stage_w
    k::ChainArgs chain{};
    std::vector<std::pair<OpImpl *, OpImpl *>> chain_members;
    // FCCHAIN: consecutive FullyConnected layers (+ Softmax) in one launch (k_fc_rt.hip fc_chain); the layers' fc_rt images
    k::FcChainArgs fcchain{};
    long long fcchain_M = 1; // rows per inference
    // POOLFC: the global AveragePool2D + FullyConnected layers (+ Softmax) in one launch (k_pool_fc.hip pool_fc_chain); a = the pool
    k::PoolFcArgs poolfc{};
    // PAIRBAND: one pair too large for chain_rt's LDS plan, walked in row bands (k_pair_band.hip); a = the depthwise, b = the conv
    k::PairBandArgs pairband{};
    // PAIRWZ: one pair with filter zero points, whole images in LDS (k_pair_wz.hip); a = the depthwise, b = the conv; table and images in stage_w
    k::PairWzArgs pairwz{};
    // CONV1FC: a one-input-channel convolution + FullyConnected (+ Softmax) in one launch (k_conv1_fc.hip); a = the convolution, b = the
    // FullyConnected, c = the Softmax or nullptr; the convolution's operand A in stage_w
    k::Conv1FcArgs conv1fc{};
    size_t conv1fc_max_batch = 0; // 0: any batch; else the largest batch at which the launch beat the operators' own (fused_batch_ok)
    // the model's f32 boundary inside this group's launch (fused_set_input_quant / fused_set_output_dequant): FCCHAIN and DWFC both
    // ends, POOLFC and PAIRTAIL the exit
    k::F32Edge edge{};
    bool edge_in = false, edge_out = false;
    int epi_mode = -1; // epilogue mode (k_common.hpp) of the launch's requantising operators; -1: not recorded (the operators' minimum)
};
// the pair's argument blocks as the operators hold them (two-rounding constants), and switched to the single-fma form when
// both operators have it
// fma: 0 = the two-rounding constants; 1 = the single-fma form if both operators have it WITHOUT patched accumulators (quads,
// register-resident pairs); 2 = ... with or without (dwpw_mm, the stage: kernels that apply the patch list)
static k::DwPwArgs pair_args(const OpImpl *dw, const OpImpl *pw, int fma) {
    k::DwPwArgs a;
    a.dw = dw->dwf, a.pw = pw->pw;
    if ((fma == 1 && dw->fma_strict() && pw->fma_strict()) || (fma == 2 && dw->fma_ok && pw->fma_ok)) a.dw.use_fma(true), a.pw.use_fma(true);
    return a;
}
static int pair_mode(const k::DwPwArgs &a) { return std::min(a.dw.magic, a.pw.magic); }
// An operator's patch list as the table a kernel reads: one EpiPatchRec per tile, `tile_of(channel, reg, lane_group)` = the tile
// index of the channel in that kernel (and which of a lane's four accumulators / which 16-lane group hold it).  false: two patched
// channels share a tile -- the kernel's record holds one -- so this launch cannot use the single-fma form.
template <typename F> static bool patch_table(const k::EpiPatch &pl, std::vector<k::EpiPatchRec> &tab, size_t base, F tile_of) {
    for (int e = 0; e < pl.n; ++e) {
        int reg = 0, grp = 0;
        const int t = tile_of(pl.ch[e], reg, grp);
        if (t < 0 || base + (size_t)t >= tab.size() || tab[base + (size_t)t].P != 0) return false;
        tab[base + (size_t)t] = k::epi_patch_rec(pl.P[e], pl.R[e], reg, grp);
    }
    return true;
}

// a device array the group owns: uploaded now, freed with the group
static const void *keep(FusedImpl &f, const void *src, size_t bytes) {
    f.stage_w.emplace_back(new DevBuf);
    f.stage_w.back()->upload(src, bytes);
    return f.stage_w.back()->p;
}
// the host copy of the Kc array an operator's argument block points at: its two-rounding constants or its single-fma ones
static const std::vector<int32_t> &host_kc(const OpImpl *op, const int *d_kc) { return d_kc == op->d_Kc3.as<int>() ? op->h_Kc3 : op->h_Kc; }
// Kc + the bit-pattern offset of requant_t<true> (k_common.hpp), as an array of the group's own
static const int *kc_with_magic(FusedImpl &owner, const std::vector<int32_t> &h_Kc) {
    std::vector<int32_t> h = h_Kc;
    for (int32_t &v : h) v = wrap_add(v, 0x4B400000);
    return (const int *)keep(owner, h.data(), h.size() * 4);
}
// a 1x1 convolution's weights ([N][1][1][C], i8 domain, as uploaded) as the stage and tail kernels' operand A
static const void *plain_pw_image(FusedImpl &owner, const OpImpl *pw) {
    const std::vector<int8_t> prep = wimage::build_pw_plain_weights(pw->h_w.data(), pw->s.C, pw->s.N);
    return keep(owner, prep.data(), prep.size());
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
    if (!dw || !pw || dw->device != pw->device || dw->force_generic || pw->force_generic) return false;
    const OpSpec &d = dw->s, &q = pw->s;
    if (d.kind != MF_OP_DEPTHWISE_CONV_2D || q.kind != MF_OP_CONV_2D || d.u8 != q.u8) return false;
    if (dw->fast != OpImpl::DW_RT && dw->fast != OpImpl::DW_NHWC) return false;
    const k::DwFastArgs &f = dw->fast == OpImpl::DW_NHWC ? dw->dwf : dw->dwrt.dw;
    const int P = chain_superpixel(d.C);  // pixels per 16-channel "superpixel" (1: C % 16 == 0; 0: no such form)
    if ((P == 1 && !f.wmm) || (dw->fast == OpImpl::DW_RT && dw->rt_wz)) return false;
    if (d.KH != 3 || d.KW != 3 || d.pad != MF_PAD_SAME || d.sh != d.sw || (d.sh != 1 && d.sh != 2) || d.C != d.N) return false;
    if (P == 0 || d.W % (P * d.sh) != 0) return false; // (C < 16: whole superpixels in and out, see chain_geom)
    if (P > 1 && d.sh == 2 && switches().chain_no_sp) return false;
    if (q.KH != 1 || q.KW != 1 || q.sh != 1 || q.sw != 1 || q.OH != q.H || q.OW != q.W || (P * q.N) % 16 != 0) return false;
    if (q.H != d.OH || q.W != d.OW || q.C != d.N) return false;
    if (pw->fast != OpImpl::PW_RT && pw->fast != OpImpl::PW_MFMA) return false;
    if (pw->fast == OpImpl::PW_RT && pw->rt_wz) return false;
    if (!dw->finite_consts || !pw->finite_consts) return false;
    if ((dw->magic_mode < 1 || pw->magic_mode < 1) && q.C < 256) return false; // (the v_cvt epilogue exists for four k steps only: launch_chain)
    return true;
}
// The geometry the planner sees.  C < 16 (the first pairs of a MobileNet-v1-shaped network: C = 8, or 4 and 8 at width 0.5): P = 16 / C
// adjacent pixels form one 16-channel "superpixel" -- the depthwise taps are build_dw_mm_weights_sp (MFMA rows = (pixel of the
// superpixel, channel), filter-row blocks = neighbouring superpixels, either stride), the 1x1 convolution is block diagonal over the P
// pixels -- so the pair IS a 16-channel pair of 1/P the width with P times the outputs.  Such a pair only ever runs alone (its output
// tensor is not in the next pair's units).
static k::ChainGeom chain_geom(const OpImpl *dw, const OpImpl *pw) {
    const OpSpec &d = dw->s;
    const k::DwFastArgs &f = dw->fast == OpImpl::DW_NHWC ? dw->dwf : dw->dwrt.dw;
    const int P = chain_superpixel(d.C);
    if (P > 1) return k::ChainGeom{d.H, d.W / P, 16, d.sh, d.OH, d.OW / P, P * pw->s.N, f.izp4};
    return k::ChainGeom{d.H, d.W, d.C, d.sh, d.OH, d.OW, pw->s.N, f.izp4};
}
static FusedImpl *chain_create(const std::pair<OpImpl *, OpImpl *> *mem, int n, int force_G = 0, int force_dbuf = -1) {
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
    std::unique_ptr<FusedImpl> c(new FusedImpl{FusedImpl::CHAIN, mem[0].first, mem[n - 1].second, nullptr, {}, {}, ""});
    if (!k::chain_plan(geo.data(), n, tab.data(), c->chain, 150 * 1024, force_G, force_dbuf)) {
        if (n == 1 && force_G == 0 && switches().chain_verbose)
            fprintf(stderr, "[microflow_amd] no chain plan for %dx%dx%d s%d -> %d\n", geo[0].H, geo[0].W, geo[0].C, geo[0].S, geo[0].N);
        return nullptr;
    }
    int magic = 2;
    std::string name = "chain_rt<";
    for (int i = 0; i < n; ++i) {
        OpImpl *dw = mem[i].first, *pw = mem[i].second;
        const k::DwFastArgs &f = dw->fast == OpImpl::DW_NHWC ? dw->dwf : dw->dwrt.dw;
        k::ChainPair &t = tab[(size_t)i];
        t.dw_wmm = f.wmm, t.dwA = f.A, t.dwS = f.S, t.dwK = f.Kc, t.dw_lo = f.lo_f, t.dw_hi = f.hi_f;
        const OpSpec &q = pw->s;
        const int group = chain_superpixel(dw->s.C); // pixels per MFMA column / product row
        const std::vector<int8_t> prep = wimage::build_pw_rt_reg_weights(pw->h_w.data(), q.C, q.N, group, t.TB, t.NBLK); // [N][1][1][C], i8 domain
        t.pw_w = keep(*c, prep.data(), prep.size());
        t.pwA = pw->conv.A, t.pwS = pw->conv.S, t.pwK = pw->conv.Kc, t.pw_lo = pw->conv.lo_f, t.pw_hi = pw->conv.hi_f;
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
        {
            std::vector<int> rt;
            k::chain_rtab(t, rt);
            t.rtab = (const int *)keep(*c, rt.data(), rt.size() * sizeof(int));
        }
        magic = std::min(magic, std::min(dw->magic_mode, pw->magic_mode));
        name += (i ? "|" : "") + std::to_string(dw->s.H) + "x" + std::to_string(dw->s.W) + "x" + std::to_string(dw->s.C) +
                (dw->s.sh == 2 ? "s2" : "") + "-" + std::to_string(q.N);
        c->chain_members.push_back(mem[i]);
    }
    name += ";G" + std::to_string(c->chain.G) + ">";
    c->name = name;
    if (switches().chain_verbose) fprintf(stderr, "[microflow_amd] %s est %.4f us/image/CU lds %d nwave %d dbuf %d\n", name.c_str(), c->chain.est_us_per_image, c->chain.lds_bytes, c->chain.nwave, c->chain.dbuf);
    c->chain.pairs = (const k::ChainPair *)keep(*c, tab.data(), tab.size() * sizeof(k::ChainPair));
    if (magic == 0 && c->chain.KSC != 4) return nullptr;
    c->chain.magic = magic, c->chain.xr = mem[0].first->s.u8 ? 0x80 : 0;
    c->epi_mode = magic;
    c->chain.queue = (int *)mem[0].first->d_queue.p, c->chain.qlaunch = &mem[0].first->q_launches;
    return c.release();
}
// second level: `n` consecutive single-pair chain groups as ONE chain (nullptr: no plan fits)
FusedImpl *fused_chain_create(FusedImpl *const *groups, int n, int force_G) {
    std::vector<std::pair<OpImpl *, OpImpl *>> mem;
    for (int i = 0; i < n; ++i) {
        if (!groups[i] || groups[i]->kind != FusedImpl::CHAIN || groups[i]->chain_members.size() != 1) return nullptr;
        mem.push_back(groups[i]->chain_members[0]);
    }
    return chain_create(mem.data(), n, force_G);
}
bool fused_is_chain_single(const FusedImpl *f) { return f && f->kind == FusedImpl::CHAIN && f->chain_members.size() == 1; }

// ---- one pair of any image size in row bands (k_pair_band.hip; 256 < C <= 512: k_pair_band_deep.hip): fused_create's last resort ----
// Takes a pair only when the table kernels and chain_create have both declined AND the pair is too large for chain_rt at one image
// per step (pair_band_plan's size condition): chain_rt keeps every pair it takes, and a small pair chain_plan refuses for another
// reason (12x12x48 -> 48: three output tiles) stays two operators.  Does not depend on which kernel the 1x1 runs on its own: the
// operand image is built here from its host weights.
// Above 256 input channels there is no size condition (chain_rt never takes such a pair): pair_band_deep_plan takes whatever fits.
static FusedImpl *pair_band_create(OpImpl *dw, OpImpl *pw) {
    if (switches().no_pair_band || !dw || !pw || dw->device != pw->device || dw->force_generic || pw->force_generic) return nullptr;
    const OpSpec &d = dw->s, &q = pw->s;
    if (d.kind != MF_OP_DEPTHWISE_CONV_2D || q.kind != MF_OP_CONV_2D || d.u8 != q.u8) return nullptr;
    // geometry as chain_pair_ok: 3x3 SAME, equal strides 1 or 2, one output per channel, the 1x1 at stride 1 on the depthwise output
    if (d.KH != 3 || d.KW != 3 || d.pad != MF_PAD_SAME || d.sh != d.sw || (d.sh != 1 && d.sh != 2) || d.C != d.N) return nullptr;
    if (d.sh == 2 && d.W % 2 != 0) return nullptr;
    if (q.KH != 1 || q.KW != 1 || q.sh != 1 || q.sw != 1 || q.OH != q.H || q.OW != q.W) return nullptr;
    if (q.H != d.OH || q.W != d.OW || q.C != d.N) return nullptr;
    if (d.C % 16 != 0 || d.C < 16 || d.C > 512 || q.N % 16 != 0 || q.N < 16 || q.N > 1024) return nullptr;
    // the depthwise member: dw3x3_rt or a table kernel with its taps in matrix-pipe form (none with filter zero points)
    if (dw->fast != OpImpl::DW_RT && dw->fast != OpImpl::DW_NHWC) return nullptr;
    const k::DwFastArgs &f = dw->fast == OpImpl::DW_NHWC ? dw->dwf : dw->dwrt.dw;
    if (!f.wmm || (dw->fast == OpImpl::DW_RT && dw->rt_wz)) return nullptr;
    // the 1x1: whatever it runs alone, its filter zero points must be zero in the i8 domain
    if (pw->h_w.size() != (size_t)q.N * q.C || pw->h_A.size() != (size_t)q.N) return nullptr;
    for (int32_t z : pw->h_wzp)
        if (z != 0) return nullptr;
    if (!dw->finite_consts || !pw->finite_consts) return nullptr;
    std::unique_ptr<FusedImpl> c(new FusedImpl{FusedImpl::PAIRBAND, dw, pw, nullptr, {}, {}, ""});
    k::PairBandArgs &a = c->pairband;
    const bool deep = d.C > 256; // 256 < C <= 512: pair_band_deep_rt's plan (k_pair_band_deep.hip: eight k steps, no lower size bound)
    const k::ChainGeom geom{d.H, d.W, d.C, d.sh, d.OH, d.OW, q.N, f.izp4};
    if (!(deep ? k::pair_band_deep_plan(geom, a) : k::pair_band_plan(geom, a))) return nullptr;
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
    a.dw_wmm = f.wmm, a.dwA = f.A, a.dwS = f.S, a.dwK = f.Kc, a.dw_lo = f.lo_f, a.dw_hi = f.hi_f;
    const std::vector<int8_t> prep = wimage::build_pw_rt_reg_weights(pw->h_w.data(), q.C, q.N, 1, a.TB, a.NBLK); // [N][1][1][C], i8 domain
    a.pw_w = keep(*c, prep.data(), prep.size());
    a.pwA = pw->conv.A, a.pwS = pw->conv.S, a.pwK = pw->conv.Kc, a.pw_lo = pw->conv.lo_f, a.pw_hi = pw->conv.hi_f;
    a.magic = magic, a.xr = d.u8 ? 0x80 : 0;
    a.queue = (int *)dw->d_queue.p, a.qlaunch = &dw->q_launches;
    c->epi_mode = magic;
    c->name = std::string(deep ? "pair_band_deep_rt<" : "pair_band_rt<") + std::to_string(d.H) + "x" + std::to_string(d.W) + "x" + std::to_string(d.C) + (d.sh == 2 ? "s2" : "") + "-" + std::to_string(q.N) +
              ";RB" + std::to_string(a.RB) + ";NB" + std::to_string(a.NB) + ">";
    if (switches().chain_verbose)
        fprintf(stderr, "[microflow_amd] band group %s: tile %d rows x %d B%s, MID %d B, lds %d B, %d workgroup%s per CU, %d x %d output tiles, mode %d\n", c->name.c_str(), a.TR,
                a.ROW, a.dbuf ? " (two)" : "", a.mid_bytes, a.lds_bytes, a.wgs, a.wgs == 1 ? "" : "s", a.NBLK, a.TB, magic);
    return c.release();
}

// ---- one pair whose filters carry zero points (k_pair_wz.hip): after the table pairs, chain_rt and the band kernels have all declined ----
// Every other fused launch refuses a filter zero point away from zero in the i8 domain -- every classic asymmetric-uint8 model, and
// per-channel zero points on i8 -- so such a pair used to run dw3x3_rt<S,wzp> + pw_rt<K,N,wzp> with its intermediate tensor through
// HBM.  This group takes exactly those pairs (at least one member with a non-zero zero point: a pair without keeps the group it has
// today), on chain_plan's single-pair plan.  A kind of its own: the stage, quad, tail and chain-partition code all answer "no" to it.
static FusedImpl *pair_wz_create(OpImpl *dw, OpImpl *pw) {
    if (switches().no_pair_wz || !dw || !pw || dw->device != pw->device || dw->force_generic || pw->force_generic) return nullptr;
    const OpSpec &d = dw->s, &q = pw->s;
    if (d.kind != MF_OP_DEPTHWISE_CONV_2D || q.kind != MF_OP_CONV_2D || d.u8 != q.u8) return nullptr;
    // geometry as chain_pair_ok: 3x3 SAME, equal strides 1 or 2, one output per channel, the 1x1 at stride 1 on the depthwise output
    if (d.KH != 3 || d.KW != 3 || d.pad != MF_PAD_SAME || d.sh != d.sw || (d.sh != 1 && d.sh != 2) || d.C != d.N) return nullptr;
    if (d.W % d.sh != 0) return nullptr;
    if (q.KH != 1 || q.KW != 1 || q.sh != 1 || q.sw != 1 || q.OH != q.H || q.OW != q.W) return nullptr;
    if (q.H != d.OH || q.W != d.OW || q.C != d.N) return nullptr;
    if (d.C % 16 != 0 || d.C < 16 || d.C > 256 || q.N % 16 != 0 || q.N < 16) return nullptr;
    // the members' own launches: dw3x3_rt or a table kernel, pw_rt or pw_mfma (anything else is a shape class of its own)
    if (dw->fast != OpImpl::DW_RT && dw->fast != OpImpl::DW_NHWC) return nullptr;
    if (pw->fast != OpImpl::PW_RT && pw->fast != OpImpl::PW_MFMA) return nullptr;
    if (dw->h_w.size() != (size_t)9 * d.C || pw->h_w.size() != (size_t)q.N * q.C || dw->h_wzp.size() != (size_t)d.C || pw->h_wzp.size() != (size_t)q.N) return nullptr;
    if (!dw->finite_consts || !pw->finite_consts) return nullptr;
    const bool wz = !std::all_of(dw->h_wzp.begin(), dw->h_wzp.end(), [](int32_t z) { return z == 0; }) ||
                    !std::all_of(pw->h_wzp.begin(), pw->h_wzp.end(), [](int32_t z) { return z == 0; });
    if (!wz) return nullptr; // (zero filter zero points: the pair keeps exactly the group -- or the two launches -- it has today)
    const k::DwFastArgs &f = dw->fast == OpImpl::DW_NHWC ? dw->dwf : dw->dwrt.dw;
    const k::ChainGeom geom{d.H, d.W, d.C, d.sh, d.OH, d.OW, q.N, f.izp4};
    std::unique_ptr<FusedImpl> c(new FusedImpl{FusedImpl::PAIRWZ, dw, pw, nullptr, {}, {}, ""});
    k::ChainArgs &a = c->pairwz.c;
    k::ChainPair t{};
    if (!k::chain_plan(&geom, 1, &t, a, 150 * 1024)) {
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
        if (!k::chain_plan(&geom, 1, &t2, a2, 150 * 1024, a.G * gm)) continue;
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
    t.dwA = dw->conv.A, t.dwS = dw->conv.S, t.dwK = dw->conv.Kc, t.dw_lo = dw->conv.lo_f, t.dw_hi = dw->conv.hi_f;
    const std::vector<int8_t> prep = wimage::build_pw_rt_reg_weights(pw->h_w.data(), q.C, q.N, 1, t.TB, t.NBLK); // [N][1][1][C], i8 domain
    t.pw_w = keep(*c, prep.data(), prep.size());
    t.pwA = pw->conv.A, t.pwS = pw->conv.S, t.pwK = pw->conv.Kc, t.pw_lo = pw->conv.lo_f, t.pw_hi = pw->conv.hi_f;
    {
        std::vector<int> rt;
        k::chain_rtab(t, rt);
        t.rtab = (const int *)keep(*c, rt.data(), rt.size() * sizeof(int));
    }
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
    c->name = "pair_wz_rt<" + std::to_string(d.H) + "x" + std::to_string(d.W) + "x" + std::to_string(d.C) + (d.sh == 2 ? "s2" : "") + "-" + std::to_string(q.N) + ";G" + std::to_string(a.G) + ">";
    if (switches().chain_verbose)
        fprintf(stderr, "[microflow_amd] zero-point group %s: lds %d B, dbuf %d, %d x %d output tiles, %d k step%s, mode %d\n", c->name.c_str(), a.lds_bytes, a.dbuf, t.NBLK, t.TB, t.KS,
                t.KS == 1 ? "" : "s", magic);
    return c.release();
}

static FusedImpl *pair_create(OpImpl *dw, OpImpl *pw);
FusedImpl *fused_create(OpImpl *dw, OpImpl *pw) {
    if (FusedImpl *f = pair_create(dw, pw)) return f; // the table pairs, then chain_rt
    if (FusedImpl *f = pair_band_create(dw, pw)) return f;
    return pair_wz_create(dw, pw); // (only ever a pair with filter zero points, which the two above refuse)
}
static FusedImpl *pair_create(OpImpl *dw, OpImpl *pw) {
    const bool chain_all = switches().chain_all; // tests / A-B: the chain kernel on table shapes too
    if (dw && pw && (chain_all || dw->fast != OpImpl::DW_NHWC || pw->fast != OpImpl::PW_MFMA ||
                     !k::dwpw_name(dw->s.H, dw->s.W, dw->s.C, dw->s.sh, pw->s.N))) {
        const std::pair<OpImpl *, OpImpl *> one(dw, pw);
        if (FusedImpl *c = chain_create(&one, 1)) return c;
    }
    if (!dw || !pw || dw->fast != OpImpl::DW_NHWC || pw->fast != OpImpl::PW_MFMA) return nullptr;
    const OpSpec &d = dw->s, &q = pw->s;
    // the pointwise conv must consume exactly the depthwise output tensor
    if (q.H != d.OH || q.W != d.OW || q.C != d.N || dw->device != pw->device) return nullptr;
    const char *nm = k::dwpw_name(d.H, d.W, d.C, d.sh, q.N);
    if (!nm) return nullptr;
    FusedImpl *f = new FusedImpl{FusedImpl::DWPW, dw, pw, nullptr, {}, {}, nm};
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

FusedImpl *fused_tail_create(OpImpl *pool, OpImpl *conv, OpImpl *sm) {
    if (!pool || !conv || !sm) return nullptr;
    const OpSpec &p = pool->s, &c = conv->s, &m = sm->s;
    if (p.u8 != c.u8 || c.u8 != m.u8) return nullptr;
    if (!conv->finite_consts || !std::isfinite(p.pool_c0) || !std::isfinite(p.pool_c1)) return nullptr;
    if (p.kind != MF_OP_AVERAGE_POOL_2D || c.kind != MF_OP_CONV_2D || m.kind != MF_OP_SOFTMAX) return nullptr;
    if (p.OH != 1 || p.OW != 1) return nullptr;                       // one pooling window
    if (c.KH != 1 || c.KW != 1 || c.H != 1 || c.W != 1 || c.OH != 1 || c.OW != 1 || c.C != p.C) return nullptr;
    if (m.M != 1 || m.N != c.N) return nullptr;                       // softmax over the head's N values
    // the in-range taps of the single window (focus (0,0); src/tensor.rs:180-228)
    const int shy = p.pad == MF_PAD_SAME ? (p.KH - 1) / 2 : 0, shx = p.pad == MF_PAD_SAME ? (p.KW - 1) / 2 : 0;
    std::vector<int> taps;
    for (int ky = 0; ky < p.KH; ++ky)
        for (int kx = 0; kx < p.KW; ++kx) {
            const int iy = ky - shy, ix = kx - shx;
            if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) taps.push_back((iy * p.W + ix) * p.C);
        }
    if (!k::tail_supported(p.C, c.N, (int)taps.size())) return nullptr;
    FusedImpl *f = new FusedImpl{FusedImpl::TAIL, pool, conv, sm, {}, {}, "tail_pool_head_softmax<" + std::to_string(c.N) + ">"};
    k::TailArgs &t = f->tail;
    t.H = p.H, t.W = p.W, t.C = p.C, t.N = c.N;
    t.ntaps = (int)taps.size();
    for (int i = 0; i < t.ntaps; ++i) t.tap_off[i] = taps[(size_t)i];
    volatile float inv = 1.0f / (float)t.ntaps; // 1. / view.len as f32 (average_pool_2d.rs:52)
    t.inv_len = inv;
    t.pool_c0 = pool->pool.c0, t.pool_c1 = pool->pool.c1, t.pool_lo = pool->pool.lo, t.pool_hi = pool->pool.hi;
    t.w = conv->conv.w, t.wzp = conv->conv.wzp, t.A = conv->conv.A, t.S = conv->conv.S, t.Kc = conv->conv.Kc;
    t.lo_f = conv->conv.lo_f, t.hi_f = conv->conv.hi_f;
    t.exp_table = sm->sm.exp_table, t.sm_oscale = sm->sm.oscale, t.sm_ozp_f = sm->sm.ozp_f;
    t.pool_bias = pool->pool.bias, t.pool_sat_lo = pool->pool.sat_lo, t.pool_sat_hi = pool->pool.sat_hi;
    t.sm_sat_lo = sm->sm.sat_lo, t.sm_sat_hi = sm->sm.sat_hi, t.xr = pool->pool.xr;
    return f;
}

// FullyConnected (one row per inference, the few-outputs row-wave kernel) -> [Reshape] -> Softmax
// over exactly those outputs
FusedImpl *fused_fc_softmax_create(OpImpl *fc, OpImpl *sm) {
    if (!fc || !sm || fc->fast != OpImpl::FC_ROWWAVE || sm->s.kind != MF_OP_SOFTMAX) return nullptr;
    if (fc->s.M != 1 || sm->s.M != 1 || sm->s.N != fc->s.N || fc->s.N < 2 || fc->device != sm->device) return nullptr;
    if (fc->s.u8 != sm->s.u8) return nullptr;
    return new FusedImpl{FusedImpl::FCSM, fc, sm, nullptr, {}, {}, "fc_rowwave_softmax<" + std::to_string(fc->s.N) + ">"};
}

// Consecutive FullyConnected operators (each reading the previous one's [M][N] output) + optionally a Softmax over one row, as
// one fc_chain launch; nullptr when a member has no fc_rt image or the layers' images and tiles do not fit the LDS budget
static bool fc_chain_args(OpImpl *const *fcs, int n, OpImpl *sm, k::FcChainArgs &a) {
    if (switches().no_fc_chain || n < 2 || n > k::FC_CHAIN_MAX) return false;
    a = k::FcChainArgs{};
    a.L = n;
    int mode = 3;
    for (int l = 0; l < n; ++l) {
        const OpImpl *o = fcs[l];
        if (!o || o->s.kind != MF_OP_FULLY_CONNECTED || !o->fcrt_ok || o->fast == OpImpl::FC_ROWWAVE || o->s.M != fcs[0]->s.M ||
            o->s.u8 != fcs[0]->s.u8 || o->device != fcs[0]->device)
            return false;
        const k::FcRtArgs &f = o->fcrt;
        k::FcChainLayer &y = a.l[l];
        y.wimg = f.wimg, y.A = f.A, y.Kc = f.Kc, y.S = f.S, y.lo_f = f.lo_f, y.hi_f = f.hi_f, y.K = f.K, y.N = f.N, y.wzp = f.wzp;
        mode = std::min(mode, f.magic);
    }
    if (sm) {
        if (sm->s.kind != MF_OP_SOFTMAX || fcs[0]->s.M != 1 || sm->s.M != 1 || sm->s.N != fcs[n - 1]->s.N || sm->s.u8 != fcs[0]->s.u8 ||
            sm->device != fcs[0]->device)
            return false;
        a.softmax = 1, a.sm = sm->sm;
    }
    a.magic = mode, a.xr = fcs[0]->fcrt.xr;
    return k::fc_chain_plan(a);
}
bool fused_fc_chain_fits(OpImpl *const *fcs, int n, OpImpl *sm) {
    k::FcChainArgs a;
    return fc_chain_args(fcs, n, sm, a);
}
FusedImpl *fused_fc_chain_create(OpImpl *const *fcs, int n, OpImpl *sm) {
    k::FcChainArgs a;
    if (!fc_chain_args(fcs, n, sm, a)) return nullptr;
    FusedImpl *f = new FusedImpl{FusedImpl::FCCHAIN, fcs[0], fcs[n - 1], sm, {}, {}, "fc_chain<" + std::to_string(n) + (sm ? ">+sm" : ">")};
    f->fcchain = a, f->fcchain_M = fcs[0]->s.M, f->epi_mode = a.magic;
    return f;
}

// AveragePool2D over the whole image (one output pixel whose in-range taps are every pixel) -> [Reshape] -> FullyConnected layers
// with one row per inference, the first reading the C pooled values -> [Softmax over the last layer's outputs], as one pool_fc_chain
// launch; false when the pool is not the global one, C % 16 != 0, a constant is not finite, a layer has no fc_rt image, or the images
// and tiles do not fit the LDS budget (k::pool_fc_plan)
static bool pool_fc_args(OpImpl *pool, OpImpl *const *fcs, int n, OpImpl *sm, k::PoolFcArgs &a) {
    if (switches().no_pool_fc || !pool || n < 1 || n > k::FC_CHAIN_MAX) return false;
    const OpSpec &p = pool->s;
    if (p.kind != MF_OP_AVERAGE_POOL_2D || p.OH != 1 || p.OW != 1 || p.C % 16 != 0) return false;
    if (!std::isfinite(p.pool_c0) || !std::isfinite(p.pool_c1)) return false;
    // the in-range taps of the single window (focus (0,0); src/tensor.rs:180-228) must be the whole image
    const int shy = p.pad == MF_PAD_SAME ? (p.KH - 1) / 2 : 0, shx = p.pad == MF_PAD_SAME ? (p.KW - 1) / 2 : 0;
    if (p.KH - 1 - shy < p.H - 1 || p.KW - 1 - shx < p.W - 1) return false;
    a = k::PoolFcArgs{};
    k::FcChainArgs &c = a.c;
    c.L = n;
    int mode = 3;
    for (int l = 0; l < n; ++l) {
        const OpImpl *o = fcs[l];
        if (!o || o->s.kind != MF_OP_FULLY_CONNECTED || !o->fcrt_ok || o->s.M != 1 || o->s.u8 != p.u8 || o->device != pool->device) return false;
        const k::FcRtArgs &f = o->fcrt;
        k::FcChainLayer &y = c.l[l];
        y.wimg = f.wimg, y.A = f.A, y.Kc = f.Kc, y.S = f.S, y.lo_f = f.lo_f, y.hi_f = f.hi_f, y.K = f.K, y.N = f.N, y.wzp = f.wzp;
        mode = std::min(mode, f.magic);
    }
    if (fcs[0]->s.K != p.C) return false;
    if (sm) {
        if (sm->s.kind != MF_OP_SOFTMAX || sm->s.M != 1 || sm->s.N != fcs[n - 1]->s.N || sm->s.u8 != p.u8 || sm->device != pool->device) return false;
        c.softmax = 1, c.sm = sm->sm;
    }
    c.magic = mode, c.xr = fcs[0]->fcrt.xr;
    a.P = p.H * p.W, a.C = p.C;
    a.c0 = pool->pool.c0, a.c1 = pool->pool.c1, a.lo = pool->pool.lo, a.hi = pool->pool.hi, a.bias = pool->pool.bias;
    a.sat_lo = pool->pool.sat_lo, a.sat_hi = pool->pool.sat_hi;
    if (pool->pool.xr != c.xr) return false;
    return k::pool_fc_plan(a);
}
bool fused_pool_fc_fits(OpImpl *pool, OpImpl *const *fcs, int n, OpImpl *sm) {
    k::PoolFcArgs a;
    return pool_fc_args(pool, fcs, n, sm, a);
}
FusedImpl *fused_pool_fc_create(OpImpl *pool, OpImpl *const *fcs, int n, OpImpl *sm) {
    k::PoolFcArgs a;
    if (!pool_fc_args(pool, fcs, n, sm, a)) return nullptr;
    FusedImpl *f = new FusedImpl{FusedImpl::POOLFC, pool, fcs[n - 1], sm, {}, {}, "pool_fc_chain<" + std::to_string(n) + (sm ? ">+sm" : ">")};
    f->poolfc = a, f->epi_mode = a.c.magic;
    return f;
}
bool fused_input_ok(const FusedImpl *f, const int8_t *d_in) {
    return (f->kind != FusedImpl::POOLFC && f->kind != FusedImpl::PAIRBAND && f->kind != FusedImpl::PAIRWZ && f->kind != FusedImpl::CONV1FC) || ((uintptr_t)d_in & 15) == 0; // (these read 16-byte words at the pointer)
}

// A DepthwiseConv2D or Conv2D with one input channel -> [Reshape] -> FullyConnected (one row per inference, reading the flattened
// output) -> [Softmax over its outputs], as one conv1_fc_rt launch (k_conv1_fc.hip); false for what k::conv1_fc_plan refuses (filter
// zero points, non-finite constants, the geometry limits, dwc1_fc_softmax's own geometry, the LDS budget).  The FullyConnected's fc_rt
// image and padded constants are the operator's where it has them; where the operator alone is past fc_rt's own budget (8000 -> 12
// runs fc_generic) the group builds them from the host copies
static bool conv1_fc_args(OpImpl *cv, OpImpl *fc, OpImpl *sm, k::Conv1FcArgs &a) {
    if (switches().no_conv1_fc || !cv || !fc || cv->force_generic || fc->force_generic) return false;
    const OpSpec &d = cv->s, &q = fc->s;
    if ((d.kind != MF_OP_DEPTHWISE_CONV_2D && d.kind != MF_OP_CONV_2D) || d.C != 1 || q.kind != MF_OP_FULLY_CONNECTED) return false;
    if (q.M != 1 || q.u8 != d.u8 || fc->device != cv->device || cv->h_w.empty() || fc->h_w.empty()) return false;
    const k::FcArgs &g = fc->fc;
    if ((int)fc->h_A.size() != g.N || (int)fc->h_Kc.size() != g.N || !std::isfinite(g.S) ||
        !std::all_of(fc->h_A.begin(), fc->h_A.end(), [](float v) { return std::isfinite(v); }))
        return false;
    a = k::Conv1FcArgs{};
    a.H = d.H, a.W = d.W, a.N = d.N, a.KH = d.KH, a.KW = d.KW, a.sh = d.sh, a.sw = d.sw, a.OH = d.OH, a.OW = d.OW;
    a.pad_same = d.pad == MF_PAD_SAME;
    a.wz = std::any_of(cv->h_wzp.begin(), cv->h_wzp.end(), [](int32_t z) { return z != 0; }), a.finite = cv->finite_consts;
    k::FcChainLayer &y = a.fc;
    y.S = g.S, y.lo_f = g.lo_f, y.hi_f = g.hi_f, y.K = g.K, y.N = g.N, y.wzp = g.wzp;
    if (fc->fcrt_ok) y.wimg = fc->fcrt.wimg, y.A = fc->fcrt.A, y.Kc = fc->fcrt.Kc; // (else: fused_conv1_fc_create builds them)
    if (sm) {
        if (sm->s.kind != MF_OP_SOFTMAX || sm->s.M != 1 || sm->s.N != q.N || sm->s.u8 != d.u8 || sm->device != cv->device) return false;
        a.softmax = 1, a.sm = sm->sm;
    }
    a.A = cv->conv.A, a.S = cv->conv.S, a.Kc = cv->conv.Kc, a.lo_f = cv->conv.lo_f, a.hi_f = cv->conv.hi_f;
    a.izp4 = 0x01010101u * (uint32_t)(uint8_t)(int8_t)d.izp;
    a.magic = std::min(cv->magic_mode, 2), a.xr = g.xr; // (the convolution's mode; the FullyConnected's few bytes take mode 0)
    if (cv->conv.xr != g.xr) return false;
    return k::conv1_fc_plan(a);
}
// The routing rule of DESIGN 4.2d, by measurement (profiles/r10/time_conv1_fc.txt): where the FullyConnected has its own fc_rt launch,
// conv1_fc_rt beat the three launches at batch 4096 (one step per workgroup: 1.13 - 1.55x) and lost at 65 536 (0.82 - 1.01x), so such
// a group takes batches up to 4096 only; where the FullyConnected alone runs fc_generic it won at both (2.3 - 3.1x) and takes any
bool fused_batch_ok(const FusedImpl *f, size_t batch) {
    return f->kind != FusedImpl::CONV1FC || f->conv1fc_max_batch == 0 || batch <= f->conv1fc_max_batch;
}
bool fused_conv1_fc_fits(OpImpl *conv, OpImpl *fc, OpImpl *sm) {
    k::Conv1FcArgs a;
    return conv1_fc_args(conv, fc, sm, a);
}
FusedImpl *fused_conv1_fc_create(OpImpl *conv, OpImpl *fc, OpImpl *sm) {
    k::Conv1FcArgs a;
    if (!conv1_fc_args(conv, fc, sm, a)) return nullptr;
    const OpSpec &d = conv->s;
    const bool dw = d.kind == MF_OP_DEPTHWISE_CONV_2D;
    std::unique_ptr<FusedImpl> f(new FusedImpl{FusedImpl::CONV1FC, conv, fc, sm, {}, {},
                                               std::string("conv1_fc_rt<") + (dw ? "dw," : "conv,") + std::to_string(d.KH) + "x" + std::to_string(d.KW) +
                                                   "," + std::to_string(d.N) + (sm ? ">+sm" : ">")});
    // the taps as uploaded (i8 domain): depthwise [KH][KW][N], Conv2D [N][KH][KW][1]
    auto w = [&](int ky, int kx, int c) { return dw ? conv->h_w[((size_t)ky * d.KW + kx) * d.N + c] : conv->h_w[((size_t)c * d.KH + ky) * d.KW + kx]; };
    // operand A: row R = 16 rt + r is (pixel R / N, channel R % N) where a tile holds PP pixels, channel R otherwise; lane group g of k
    // step ks holds filter row 4 ks + g at bytes pixel * sw .. + KW - 1
    std::vector<int8_t> wa((size_t)2 * 4 * 64 * 16, 0);
    for (int rt = 0; rt < a.NRT; ++rt)
        for (int ks = 0; ks < a.KSC; ++ks)
            for (int lane = 0; lane < 64; ++lane) {
                const int R = rt * 16 + (lane & 15), ky = 4 * ks + (lane >> 4);
                const int px = a.PP > 1 ? R / d.N : 0, c = R - px * d.N;
                if (px >= a.PP || c >= d.N || ky >= d.KH) continue;
                for (int kx = 0; kx < d.KW; ++kx) wa[(((size_t)rt * 4 + ks) * 64 + lane) * 16 + (size_t)(px * d.sw + kx)] = w(ky, kx, c);
            }
    a.wA = keep(*f, wa.data(), wa.size());
    if (!fc->fcrt_ok) {
        const std::vector<int8_t> img = k::fc_rt_weight_image(fc->h_w.data(), a.fc.K, a.fc.N);
        std::vector<float> pA((size_t)a.fc.NT * 16, 0.0f);
        std::vector<int32_t> pK((size_t)a.fc.NT * 16, 0);
        std::copy(fc->h_A.begin(), fc->h_A.end(), pA.begin()), std::copy(fc->h_Kc.begin(), fc->h_Kc.end(), pK.begin());
        a.fc.wimg = keep(*f, img.data(), img.size());
        a.fc.A = (const float *)keep(*f, pA.data(), pA.size() * 4), a.fc.Kc = (const int *)keep(*f, pK.data(), pK.size() * 4);
    }
    f->conv1fc = a, f->epi_mode = a.magic;
    f->conv1fc_max_batch = fc->fcrt_ok ? 4096 : 0;
    return f.release();
}

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
    std::unique_ptr<FusedImpl> s(new FusedImpl{FusedImpl::STAGE, pairs[0]->a, pairs[npairs - 1]->b, nullptr, {}, {}, nm});
    s->stage_pairs = npairs;
    std::vector<k::StagePair> table((size_t)npairs);
    for (int i = 0; i < npairs; ++i) {
        const FusedImpl *fp = pairs[i];
        FusedImpl tmp{FusedImpl::DWPW, fp->a, fp->b, nullptr, {}, {}, ""};
        tmp.dwpw = pair_args(fp->a, fp->b, all_fma ? 2 : 0);
        const FusedImpl *f = &tmp;
        k::StagePair &sp = table[(size_t)i];
        // (this kernel takes Kc with the bit-pattern offset already added)
        sp.dw_wmm = f->dwpw.dw.wmm, sp.dwA = f->dwpw.dw.A, sp.dwS = f->dwpw.dw.S, sp.dwK = kc_with_magic(*s, host_kc(f->a, f->dwpw.dw.Kc));
        sp.dw_lo = f->dwpw.dw.lo_f, sp.dw_hi = f->dwpw.dw.hi_f;
        sp.pw_w = plain_pw_image(*s, f->b);
        sp.pwA = f->dwpw.pw.A, sp.pwS = f->dwpw.pw.S, sp.pwK = kc_with_magic(*s, host_kc(f->b, f->dwpw.pw.Kc));
        sp.pw_lo = f->dwpw.pw.lo_f, sp.pw_hi = f->dwpw.pw.hi_f;
    }
    s->stage.patch_tab = nullptr;
    if (all_fma) { // (also when nothing is patched: the kernel fetches its records with the operands, unconditionally)
        s->stage.patch_tab = (const k::EpiPatchRec *)keep(*s, ptab.data(), ptab.size() * sizeof(k::EpiPatchRec));
    }
    s->stage.pairs = (const k::StagePair *)keep(*s, table.data(), table.size() * sizeof(k::StagePair));
    s->stage.izp4 = pairs[0]->dwpw.dw.izp4;
    s->stage.xr4 = d0.u8 ? 0x80808080u : 0u;
    s->stage.queue = pairs[0]->dwpw.dw.queue, s->stage.qlaunch = pairs[0]->dwpw.dw.qlaunch;
    s->stage.mode = all_fma ? 3 : 2; // the saturating-pack epilogue needs it of every operator of the run
    for (int i = 0; i < npairs && !all_fma; ++i)
        if (pairs[i]->a->magic_mode != 2 || pairs[i]->b->magic_mode != 2) s->stage.mode = 1;
    s->epi_mode = s->stage.mode;
    return s.release();
}

// DepthwiseConv2D with one input channel (the dw_c1_lds operator) -> [Reshape] -> FullyConnected + Softmax group, as
// one kernel (k_dwfc.hip; speech.tflite ops 1..3).  Second level like the stage: the operator and the group inside
// stay available for mf_model_run_until.  nullptr when the shapes are not the compiled instance.
FusedImpl *fused_dwfc_create(OpImpl *dw, FusedImpl *fcsm) {
    const bool off = switches().no_dwfc;
    if (off || !dw || !fcsm || dw->fast != OpImpl::DW_C1 || fcsm->kind != FusedImpl::FCSM) return nullptr;
    OpImpl *fc = fcsm->a, *sm = fcsm->b;
    const OpSpec &d = dw->s, &q = fc->s;
    using Gm = k::DwFcGeom;
    if (!k::dwfc_supported(d.H, d.W, d.KH, d.KW, d.sh, d.sw, d.OH, d.OW, d.N, q.N)) return nullptr;
    if (d.pad != MF_PAD_SAME || d.C != 1 || q.M != 1 || q.K != d.OH * d.OW * d.N || dw->device != fc->device) return nullptr;
    if (d.u8 != q.u8) return nullptr;
    std::unique_ptr<FusedImpl> f(new FusedImpl{FusedImpl::DWFC, dw, fc, sm, {}, {}, k::dwfc_name()});
    // both operators' weights as they were uploaded (i8 domain): the depthwise taps from dw_c1_lds's packed form
    // [ky][4-tap group][8 channels] dwords, the FullyConnected matrix [N][K]
    const k::DwC1Args &c1 = dw->dwc1;
    const std::vector<uint32_t> &wp = dw->h_wpack;
    auto dw_w = [&](int ky, int kx, int c) { return (int8_t)(wp[((size_t)ky * c1.KG + kx / 4) * 8 + c] >> (8 * (kx & 3))); };
    const std::vector<int8_t> &fc_w = fc->h_w;
    // operand A: taps of filter row ky = (4k + g) - 2p at byte b = kx + 2s + E0 of the 16-byte window, for row
    // r = (p, c) of the accumulator tile; zero elsewhere
    std::vector<int8_t> wa((size_t)4 * 3 * 64 * 16, 0);
    for (int sft = 0; sft < 4; ++sft)
        for (int kk = 0; kk < 3; ++kk)
            for (int lane = 0; lane < 64; ++lane) {
                const int r = lane & 15, g = lane >> 4, p = r >> 3, c = r & 7;
                const int ky = 4 * kk + g - Gm::S * p;
                if (ky < 0 || ky >= Gm::KH) continue;
                for (int kx = 0; kx < Gm::KW; ++kx)
                    wa[(((size_t)sft * 3 + kk) * 64 + lane) * 16 + (size_t)(kx + Gm::S * sft + Gm::E0)] =
                        dw_w(ky, kx, c);
            }
    // FullyConnected as operand A of one more MFMA per unit (t, m): lane group g = (p, channel half) holds, for row
    // n < 4, the weights of the 16 activations it packs -- pixels (2t + p, 4m + s), s = 0..3, channels 4 (g & 1) .. + 3
    // of the NHWC flattening -- and for row 4 ones (the row sum); nothing for pixel rows beyond the image
    std::vector<int8_t> wf((size_t)Gm::FCW_BYTES, 0);
    for (int u = 0; u < Gm::NU; ++u)
        for (int g = 0; g < 4; ++g) {
            const int t = u / Gm::NM, m = u % Gm::NM, oy = 2 * t + (g >> 1);
            if (oy >= Gm::OH) continue;
            for (int sft = 0; sft < 4; ++sft) {
                const size_t k0 = ((size_t)oy * Gm::OW + 4 * m + sft) * 8 + 4 * (size_t)(g & 1);
                for (int b = 0; b < 4; ++b) {
                    for (int n = 0; n < 4; ++n) wf[(((size_t)u * 4 + g) * 5 + n) * 16 + 4 * sft + b] = fc_w[(size_t)n * q.K + k0 + b];
                    wf[(((size_t)u * 4 + g) * 5 + 4) * 16 + 4 * sft + b] = 1;
                }
            }
        }
    f->dwfc.wA = keep(*f, wa.data(), wa.size());
    f->dwfc.wfc = keep(*f, wf.data(), wf.size());
    f->dwfc.dwA = c1.A, f->dwfc.dwS = c1.S, f->dwfc.dwKc = c1.Kc, f->dwfc.dw_lo = c1.lo_f, f->dwfc.dw_hi = c1.hi_f;
    f->dwfc.izp4 = 0x01010101u * (uint32_t)(uint8_t)(int8_t)c1.izp;
    f->dwfc.magic = c1.magic, f->dwfc.xr = c1.xr;
    f->epi_mode = c1.magic;
    f->dwfc.fc = fc->fc, f->dwfc.sm = sm->sm;
    return f.release();
}

// The last pair group (DepthwiseConv2D 3x3 stride 1 + Conv2D 1x1 on 3x3x256) followed by the tail group
// (AveragePool2D over the whole tensor -> head Conv2D -> Softmax) as one kernel (k_tail3.hip).  Second level like the
// stage; nullptr when the shapes are not the compiled instance.
FusedImpl *fused_pair_tail_create(FusedImpl *pair, FusedImpl *tail) {
    const bool off = switches().no_pairtail;
    if (off || !pair || !tail || tail->kind != FusedImpl::TAIL) return nullptr;
    // the pair: a table group (dwpw_mm) or a single-pair run-time-geometry chain group
    OpImpl *dw = nullptr, *pw = nullptr;
    if (pair->kind == FusedImpl::DWPW) dw = pair->a, pw = pair->b;
    else if (pair->kind == FusedImpl::CHAIN && pair->chain_members.size() == 1) dw = pair->chain_members[0].first, pw = pair->chain_members[0].second;
    if (!dw || !pw || (dw->fast != OpImpl::DW_NHWC && dw->fast != OpImpl::DW_RT) || (dw->fast == OpImpl::DW_RT && dw->rt_wz)) return nullptr;
    if ((pw->fast != OpImpl::PW_MFMA && pw->fast != OpImpl::PW_RT) || (pw->fast == OpImpl::PW_RT && pw->rt_wz)) return nullptr;
    const OpSpec &d = dw->s, &q = pw->s;
    const k::TailArgs &t = tail->tail;
    if (!k::pair_tail_supported(d.H, d.W, d.C, q.N, t.N, t.ntaps) || d.sh != 1 || d.sw != 1 || d.u8 != q.u8) return nullptr;
    if (d.KH != 3 || d.KW != 3 || d.pad != MF_PAD_SAME || d.C != d.N || q.KH != 1 || q.KW != 1 || q.C != d.N) return nullptr;
    if ((d.u8 ? 0x80 : 0) != t.xr) return nullptr;
    if (t.H != d.OH || t.W != d.OW || t.C != q.N || dw->device != tail->a->device) return nullptr;
    const k::DwFastArgs &df = dw->fast == OpImpl::DW_NHWC ? dw->dwf : dw->dwrt.dw;
    if (!df.wmm || !dw->finite_consts || !pw->finite_consts) return nullptr;
    const int magic = (dw->magic_mode >= 1 && pw->magic_mode >= 1) ? 1 : 0; // bit-pattern epilogues, or the v_cvt form for both
    std::unique_ptr<FusedImpl> f(new FusedImpl{FusedImpl::PAIRTAIL, dw, tail->b, tail->c, {}, {}, k::pair_tail_name(d.H, d.C)});
    k::PairTailArgs &a = f->pairtail;
    a.H = d.H, a.C = d.C, a.magic = magic;
    f->epi_mode = magic;
    a.dw_wmm = df.wmm, a.dwA = df.A, a.dwS = df.S, a.dwK = magic ? kc_with_magic(*f, dw->h_Kc) : df.Kc;
    a.dw_lo = df.lo_f, a.dw_hi = df.hi_f, a.izp4 = df.izp4;
    a.pw_w = plain_pw_image(*f, pw);
    a.pwA = pw->conv.A, a.pwS = pw->conv.S, a.pwK = magic ? kc_with_magic(*f, pw->h_Kc) : pw->conv.Kc;
    a.pw_lo = pw->conv.lo_f, a.pw_hi = pw->conv.hi_f;
    a.tail = t;
    return f.release();
}

// The pair group in front of a pair + tail launch joins it (person_detect ops 23..30 in one launch; k_tail3.hip FRONT): second
// level like the others -- the pair group and the pair + tail stage stay for mf_model_run_until.  Borrows the pair + tail stage's
// device arrays (destroy it first); the front pair's own arrays are in stage_w.
FusedImpl *fused_front_pair_tail_create(FusedImpl *front, FusedImpl *pairtail) {
    if (switches().no_pair_front || !front || !pairtail || pairtail->kind != FusedImpl::PAIRTAIL || pairtail->has_front) return nullptr;
    if (front->kind != FusedImpl::DWPW) return nullptr;
    OpImpl *dw = front->a, *pw = front->b;
    if (!dw || !pw || dw->fast != OpImpl::DW_NHWC || pw->fast != OpImpl::PW_MFMA) return nullptr;
    const OpSpec &d = dw->s, &q = pw->s;
    const k::PairTailArgs &t = pairtail->pairtail;
    if (d.sh != d.sw || !k::pair_front_supported(d.H, d.W, d.C, d.sh, q.N, t.H, t.C)) return nullptr;
    if (d.KH != 3 || d.KW != 3 || d.pad != MF_PAD_SAME || d.C != d.N || q.KH != 1 || q.KW != 1 || q.C != d.N) return nullptr;
    if (q.OH != t.H || q.OW != t.H || d.u8 != q.u8 || (d.u8 ? 0x80u : 0u) != (uint32_t)t.tail.xr || dw->device != pairtail->a->device) return nullptr;
    const k::DwFastArgs &df = dw->dwf;
    if (!df.wmm || !dw->finite_consts || !pw->finite_consts) return nullptr;
    // one epilogue form for the launch's four convolutions: the bit-pattern one needs it of all four
    const int magic = (dw->magic_mode >= 1 && pw->magic_mode >= 1) ? 1 : 0;
    if (magic != t.magic) return nullptr;
    std::unique_ptr<FusedImpl> f(new FusedImpl{FusedImpl::PAIRTAIL, dw, pairtail->b, pairtail->c, {}, {}, "pair_front_tail<6,6,128,2,256|3,3,256,2>"});
    f->pairtail = t, f->has_front = true, f->epi_mode = magic;
    k::PairFrontArgs &a = f->pairfront;
    a.dw_wmm = df.wmm, a.dwA = df.A, a.dwS = df.S, a.dwK = magic ? kc_with_magic(*f, dw->h_Kc) : df.Kc;
    a.dw_lo = df.lo_f, a.dw_hi = df.hi_f, a.izp4 = df.izp4;
    a.pw_w = plain_pw_image(*f, pw);
    a.pwA = pw->conv.A, a.pwS = pw->conv.S, a.pwK = magic ? kc_with_magic(*f, pw->h_Kc) : pw->conv.Kc;
    a.pw_lo = pw->conv.lo_f, a.pw_hi = pw->conv.hi_f;
    return f.release();
}

static FusedImpl *quad_group(FusedImpl *p1, FusedImpl *p2, const k::DwPwArgs &a, const k::DwPwArgs &b, const char *name, bool mm) {
    const OpSpec &d1 = p1->a->s, &q1 = p1->b->s, &d2 = p2->a->s, &q2 = p2->b->s;
    FusedImpl *f = new FusedImpl{FusedImpl::QUAD, p1->a, p2->b, nullptr, {}, {}, name};
    f->quad.a = a, f->quad.b = b, f->quad_mm = mm;
    f->epi_mode = std::min(pair_mode(a), pair_mode(b));
    f->quad_ops[0] = p1->a, f->quad_ops[1] = p1->b, f->quad_ops[2] = p2->a, f->quad_ops[3] = p2->b;
    const int shp[10] = {d1.H, d1.W, d1.C, d1.sh, q1.N, d2.H, d2.W, d2.C, d2.sh, q2.N};
    for (int i = 0; i < 10; ++i) f->quad_shape[i] = shp[i];
    return f;
}
// Two consecutive DepthwiseConv2D 3x3 + Conv2D 1x1 pair groups as one kernel (k_quad.hip), when a quad kernel exists for the two
// shapes.  Second level like the stage: the pairs inside stay available for mf_model_run_until.
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
        return quad_group(p1, p2, a, b, "quad_mm<12,12,64,1,64|12,12,64,2,128>", true);
    }
    const char *nm = k::quad_name(d1.H, d1.W, d1.C, d1.sh, q1.N, d2.H, d2.W, d2.C, d2.sh, q2.N);
    if (!nm) return nullptr;
    // (the single-fma form needs it of all four operators)
    const bool fma = p1->a->fma_strict() && p1->b->fma_strict() && p2->a->fma_strict() && p2->b->fma_strict();
    const k::DwPwArgs a = pair_args(p1->a, p1->b, fma ? 1 : 0), b = pair_args(p2->a, p2->b, fma ? 1 : 0);
    if (!a.dw.wmm || !a.pw.wrr || !b.dw.wmm || !b.pw.wrr) return nullptr;
    if (!a.dw.magic || !a.pw.magic || !b.dw.magic || !b.pw.magic) return nullptr; // bit-pattern epilogues
    return quad_group(p1, p2, a, b, nm, false);
}

// The network's one-input-channel stem in front of a quad: five operators in one launch (k_quad.hip, STEM instance).  The quad
// itself stays (mf_model_run_until, and the f32 entry point, whose boundary quantisation is fused into the stem kernel).
FusedImpl *fused_quad_stem_create(OpImpl *stem, FusedImpl *quad) {
    const bool off = switches().no_penta;
    if (off || !stem || !quad || quad->kind != FusedImpl::QUAD || quad->quad.stem || stem->fast != OpImpl::DW_STEM) return nullptr;
    const OpSpec &t = stem->s, &d1 = quad->a->s;
    if (stem->device != quad->a->device || t.u8 != d1.u8 || stem->force_generic) return nullptr;
    if (t.OH != d1.H || t.OW != d1.W || t.N != d1.C || t.sh != 2 || t.sw != 2 || t.C != 1) return nullptr; // pair A consumes the stem's output
    const int *q = quad->quad_shape;
    const char *nm = k::quad_stem_name(t.H, t.W, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9]);
    if (!nm || !stem->stem.magic) return nullptr;
    std::unique_ptr<FusedImpl> f(new FusedImpl{FusedImpl::QUAD, stem, quad->b, nullptr, {}, {}, nm});
    f->quad = quad->quad;
    for (int i = 0; i < 10; ++i) f->quad_shape[i] = q[i];
    // five operators, one epilogue mode: the single-fma form if all five have it, else everyone's two-rounding constants
    OpImpl *const *qo = quad->quad_ops;
    const bool fma = stem->fma_strict() && qo[0]->fma_strict() && qo[1]->fma_strict() && qo[2]->fma_strict() && qo[3]->fma_strict();
    f->quad.a = pair_args(qo[0], qo[1], fma ? 1 : 0), f->quad.b = pair_args(qo[2], qo[3], fma ? 1 : 0);
    k::DwStemArgs sa = stem->stem;
    if (fma) sa.use_fma();
    std::vector<uint32_t> tab(152);
    for (int l = 0; l < 64; ++l) tab[(size_t)2 * l] = sa.wmm[l][0], tab[(size_t)2 * l + 1] = sa.wmm[l][1];
    for (int c = 0; c < 8; ++c) {
        memcpy(&tab[(size_t)128 + c], &sa.A[c], 4);
        memcpy(&tab[(size_t)136 + c], &sa.S[c], 4);
        memcpy(&tab[(size_t)144 + c], &sa.Kc[c], 4);
    }
    f->quad.stem = (const uint32_t *)keep(*f, tab.data(), tab.size() * 4);
    f->quad.stem_izp4 = sa.izp4, f->quad.stem_lo = sa.lo_f, f->quad.stem_hi = sa.hi_f, f->quad.stem_magic = sa.magic;
    // the f32 entry (model.cpp sets the stem's input quantisation before the groups are built): same launch, f32 image in
    f->quad.in_scale = sa.in_scale, f->quad.in_zp_f = sa.in_zp_f, f->quad.in_sat_lo = sa.in_sat_lo, f->quad.in_sat_hi = sa.in_sat_hi;
    f->quad.in_rcp = sa.in_rcp, f->quad.in_xr4 = sa.in_xr4, f->quad.in_fast = sa.in_fast, f->quad.f32_ok = stem->accepts_f32 ? 1 : 0;
    f->epi_mode = std::min(std::min(pair_mode(f->quad.a), pair_mode(f->quad.b)), sa.magic);
    return f.release();
}

void fused_destroy(FusedImpl *f) { delete f; }
const char *fused_kernel_name(const FusedImpl *f) { return f->name.c_str(); }
int fused_epilogue_mode(const FusedImpl *f) {
    if (f->epi_mode >= 0) return f->epi_mode;
    int mode = -1; // not recorded by the builder: the minimum over the group's conv-like operators
    for (const OpImpl *o : {f->a, f->b, f->c})
        if (o && (o->s.kind == MF_OP_CONV_2D || o->s.kind == MF_OP_DEPTHWISE_CONV_2D)) mode = mode < 0 ? o->magic_mode : std::min(mode, o->magic_mode);
    return mode;
}
// the f32 entry of a group that starts with the network's first operator (M::predict: the boundary quantisation inside the launch)
bool fused_set_input_quant(FusedImpl *f, float scale, int zp, bool u8) {
    if (!f || (f->kind != FusedImpl::FCCHAIN && f->kind != FusedImpl::DWFC) || !(scale == scale) || switches().no_f32_boundary) return false;
    edge_set_in(f->edge, f->a->device, scale, zp, u8);
    return f->edge_in = true;
}
bool fused_set_output_dequant(FusedImpl *f, float scale, int zp, bool u8) {
    if (!f || switches().no_f32_boundary) return false;
    if (f->kind != FusedImpl::FCCHAIN && f->kind != FusedImpl::POOLFC && f->kind != FusedImpl::DWFC && f->kind != FusedImpl::PAIRTAIL) return false;
    edge_set_out(f->edge, scale, zp, u8);
    return f->edge_out = true;
}
bool fused_accepts_f32(const FusedImpl *f) {
    if (f && f->edge_in) return true;
    return f && f->kind == FusedImpl::QUAD && f->quad.stem && f->quad.f32_ok && !switches().no_f32_group;
}
bool fused_emits_f32(const FusedImpl *f) { return f && f->edge_out; }
void fused_run_f32(FusedImpl *f, const void *d_in, bool in_f32, size_t batch, void *d_out, bool out_f32, void *stream) {
    if (!batch) return;
    if (!in_f32 && !out_f32) return fused_run(f, (const int8_t *)d_in, batch, (int8_t *)d_out, stream);
    if (in_f32 && !fused_accepts_f32(f)) fail(MF_ERR_UNSUPPORTED, "group has no f32-input kernel");
    if (out_f32 && !fused_emits_f32(f)) fail(MF_ERR_UNSUPPORTED, "group has no f32-output kernel");
    if (!d_in || !d_out || (in_f32 && ((uintptr_t)d_in & 15)) || (out_f32 && ((uintptr_t)d_out & 3)))
        fail(MF_ERR_INVALID_ARG, "fused_run_f32: null or unaligned device pointer");
    if (batch > 0x7fffffffull / 4) fail(MF_ERR_INVALID_ARG, "batch too large for one launch");
    const int edge = (in_f32 ? k::EDGE_IN : 0) | (out_f32 ? k::EDGE_OUT : 0);
    if (f->kind == FusedImpl::FCCHAIN) {
        k::launch_fc_chain_f32(d_in, d_out, f->fcchain, f->edge, edge, (long long)(batch * f->fcchain_M), (hipStream_t)stream);
        MF_HIP(hipGetLastError());
        return;
    }
    if (f->kind == FusedImpl::POOLFC) {
        if (!fused_input_ok(f, (const int8_t *)d_in)) fail(MF_ERR_INVALID_ARG, "pool_fc_chain: the input pointer is not 16-byte aligned");
        k::launch_pool_fc_f32((const int8_t *)d_in, (float *)d_out, f->poolfc, f->edge, (long long)batch, (hipStream_t)stream);
        MF_HIP(hipGetLastError());
        return;
    }
    if (f->kind == FusedImpl::DWFC) {
        k::launch_dwfc_f32(d_in, d_out, f->dwfc, f->edge, edge, batch, (hipStream_t)stream);
        MF_HIP(hipGetLastError());
        return;
    }
    if (f->kind == FusedImpl::PAIRTAIL) { // (exit only: fused_set_input_quant refuses this kind)
        if (f->has_front) k::launch_pair_front_tail((const int8_t *)d_in, (int8_t *)d_out, f->pairtail, f->pairfront, batch, (hipStream_t)stream, &f->edge);
        else k::launch_pair_tail((const int8_t *)d_in, (int8_t *)d_out, f->pairtail, batch, (hipStream_t)stream, &f->edge);
        MF_HIP(hipGetLastError());
        return;
    }
    const int *q = f->quad_shape;
    if (!k::launch_quad_f32(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], (const float *)d_in, (int8_t *)d_out, f->quad, (int)batch, (hipStream_t)stream))
        fail(MF_ERR_UNSUPPORTED, "f32 quad kernel missing");
    MF_HIP(hipGetLastError());
}
void fused_run(FusedImpl *f, const int8_t *d_in, size_t batch, int8_t *d_out, void *stream) {
    if (!batch) return;
    if (f->kind == FusedImpl::STAGE) {
        if (batch > 0x7fffffffull / 4) fail(MF_ERR_INVALID_ARG, "batch too large for one launch");
        const OpSpec &d = f->a->s;
        if (!k::launch_stage(d.H, d.W, d.C, f->stage_pairs, d_in, d_out, f->stage, (int)batch, (hipStream_t)stream))
            fail(MF_ERR_UNSUPPORTED, "stage kernel missing");
        MF_HIP(hipGetLastError());
        return;
    }
    if (f->kind == FusedImpl::CHAIN) {
        if (batch > 0x7fffffffull / 4) fail(MF_ERR_INVALID_ARG, "batch too large for one launch");
        k::launch_chain(d_in, d_out, f->chain, (int)batch, (hipStream_t)stream);
        MF_HIP(hipGetLastError());
        return;
    }
    if (f->kind == FusedImpl::PAIRBAND) {
        if (batch > 0x7fffffffull / 4 / (size_t)f->pairband.NB) fail(MF_ERR_INVALID_ARG, "batch too large for one launch");
        if (!fused_input_ok(f, d_in)) fail(MF_ERR_INVALID_ARG, "pair_band_rt: the input pointer is not 16-byte aligned");
        if (f->pairband.KSC == 8) k::launch_pair_band_deep(d_in, d_out, f->pairband, (int)batch, (hipStream_t)stream);
        else k::launch_pair_band(d_in, d_out, f->pairband, (int)batch, (hipStream_t)stream);
        MF_HIP(hipGetLastError());
        return;
    }
    if (f->kind == FusedImpl::PAIRWZ) {
        if (batch > 0x7fffffffull / 4) fail(MF_ERR_INVALID_ARG, "batch too large for one launch");
        if (!fused_input_ok(f, d_in)) fail(MF_ERR_INVALID_ARG, "pair_wz_rt: the input pointer is not 16-byte aligned");
        k::launch_pair_wz(d_in, d_out, f->pairwz, (int)batch, (hipStream_t)stream);
        MF_HIP(hipGetLastError());
        return;
    }
    if (f->kind == FusedImpl::QUAD) {
        if (batch > 0x7fffffffull / 4) fail(MF_ERR_INVALID_ARG, "batch too large for one launch");
        const int *q = f->quad_shape;
        if (f->quad_mm) {
            k::launch_quad_mm(d_in, d_out, f->quad, (int)batch, (hipStream_t)stream);
            MF_HIP(hipGetLastError());
            return;
        }
        if (!k::launch_quad(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], d_in, d_out, f->quad, (int)batch, (hipStream_t)stream))
            fail(MF_ERR_UNSUPPORTED, "quad kernel missing");
        MF_HIP(hipGetLastError());
        return;
    }
    if (f->kind == FusedImpl::TAIL) {
        k::launch_tail(d_in, d_out, f->tail, batch, (hipStream_t)stream);
        MF_HIP(hipGetLastError());
        return;
    }
    if (f->kind == FusedImpl::PAIRTAIL) {
        if (batch && f->has_front) k::launch_pair_front_tail(d_in, d_out, f->pairtail, f->pairfront, batch, (hipStream_t)stream);
        else if (batch) k::launch_pair_tail(d_in, d_out, f->pairtail, batch, (hipStream_t)stream);
        MF_HIP(hipGetLastError());
        return;
    }
    if (f->kind == FusedImpl::DWFC) {
        if (batch) k::launch_dwfc(d_in, d_out, f->dwfc, batch, (hipStream_t)stream);
        MF_HIP(hipGetLastError());
        return;
    }
    if (f->kind == FusedImpl::FCCHAIN) { // (no pointer alignment needed: fc_chain aligns its DMA and stores itself)
        k::launch_fc_chain(d_in, d_out, f->fcchain, (long long)(batch * f->fcchain_M), (hipStream_t)stream);
        MF_HIP(hipGetLastError());
        return;
    }
    if (f->kind == FusedImpl::POOLFC) { // (any output pointer: the kernel aligns its stores itself)
        if (!fused_input_ok(f, d_in)) fail(MF_ERR_INVALID_ARG, "pool_fc_chain: the input pointer is not 16-byte aligned");
        k::launch_pool_fc(d_in, d_out, f->poolfc, (long long)batch, (hipStream_t)stream);
        MF_HIP(hipGetLastError());
        return;
    }
    if (f->kind == FusedImpl::CONV1FC) { // (any output pointer: the kernel aligns its stores itself)
        if (!fused_input_ok(f, d_in)) fail(MF_ERR_INVALID_ARG, "conv1_fc_rt: the input pointer is not 16-byte aligned");
        k::launch_conv1_fc(d_in, d_out, f->conv1fc, (long long)batch, (hipStream_t)stream);
        MF_HIP(hipGetLastError());
        return;
    }
    if (f->kind == FusedImpl::FCSM) {
        if (!k::launch_fc_rowwave_softmax(d_in, d_out, f->a->fc, f->b->sm, batch, (hipStream_t)stream))
            fail(MF_ERR_UNSUPPORTED, "fused kernel missing");
        MF_HIP(hipGetLastError());
        return;
    }
    if (batch > 0x7fffffffull / 4) fail(MF_ERR_INVALID_ARG, "batch too large for one launch");
    const OpSpec &d = f->a->s;
    if (!k::launch_dwpw(d.H, d.W, d.C, d.sh, f->b->s.N, d_in, d_out, f->dwpw, (int)batch, (hipStream_t)stream))
        fail(MF_ERR_UNSUPPORTED, "fused kernel missing");
    MF_HIP(hipGetLastError());
}

// How to run `n` consecutive single-pair chain groups: seg_len[i] = number of pairs of the chain that starts at pair i (0: pair i is
// inside a chain that started earlier); unfused[i] = pair i is cheapest as two separate operator launches.  Dynamic programme over the
// planner's cost estimates (k_chain.hip: chain_plan / chain_unfused_us_per_image).
namespace {
// The partition by MEASUREMENT (the default when a device is there, i.e. always: operators are created on one): every plannable
// candidate "pairs i .. i + len - 1 as one chain_rt launch", and every pair as its two separate operators, is run on scratch tensors
// at a batch that fills the chip for dozens of steps, and the dynamic programme takes the times.  The cost model's errors were
// 0.7 - 1.5x on single pairs and 1.0 - 1.3x on chains (profiles/r04/chain_calib.txt) -- larger than the differences it decides
// between -- and every kernel change moved them.  ~0.1 - 0.3 s per model at creation; MF_CHAIN_AUTOTUNE=0 goes back to the estimates.
struct ChainTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t st = nullptr; // a private NON-BLOCKING stream: the timing neither waits for nor stalls the caller's other streams
    DevBuf a, b, c;
    size_t cap = 0;
    bool ok = false;
    explicit ChainTimer(size_t bytes) {
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); st = nullptr; return; }
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return;
        for (DevBuf *d : {&a, &b, &c}) {
            if (hipMalloc(&d->p, bytes) != hipSuccess) { (void)hipGetLastError(); return; }
            (void)hipMemsetAsync(d->p, 0, bytes, st);
        }
        cap = bytes, ok = hipStreamSynchronize(st) == hipSuccess;
    }
    ~ChainTimer() {
        if (st) (void)hipStreamSynchronize(st);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (st) (void)hipStreamDestroy(st);
    }
    template <typename F> double us(F &&launch) { // best of five after a warm-up; < 0: failed (a throwing launch counts as failed)
        try {
            launch();
            double best = -1;
            for (int r = 0; r < 5; ++r) {
                if (hipEventRecord(e0, st) != hipSuccess) return -1;
                launch();
                if (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) return -1;
                float ms = 0;
                if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return -1;
                best = best < 0 || ms * 1e3 < best ? ms * 1e3 : best;
            }
            return best;
        } catch (const Error &) {
            (void)hipGetLastError();
            failed = true;
            return -1;
        }
    }
    bool failed = false; // a launch threw: the caller drops every measurement and plans from the estimates
};
} // namespace

void fused_chain_partition(FusedImpl *const *groups, int n, int *seg_len, bool *unfused, int *seg_G, bool autotune_opt) {
    std::vector<k::ChainGeom> geo((size_t)n);
    for (int i = 0; i < n; ++i) {
        const std::pair<OpImpl *, OpImpl *> &m = groups[i]->chain_members[0];
        geo[(size_t)i] = chain_geom(m.first, m.second);
    }
    // A forced plan (MF_CHAIN_PLAN, read NOW: one process prepares the same model under many plans) replaces both the dynamic
    // programme and the timing.  Every segment is made by the functions autotune installs its winners with -- fused_chain_create,
    // chain_create + swap -- behind the same chain_plan feasibility checks, so that the switch can install nothing autotune could
    // not; a segment that cannot be made fails the preparation (a test must never pass on the planner's plan after all).
    if (switches().dev) {
        const Switches now = switches_parse();
        if (now.chain_plan_set) {
            if (!now.chain_plan_error.empty()) fail(MF_ERR_INVALID_ARG, "MF_CHAIN_PLAN: " + now.chain_plan_error);
            const bool verbose = switches().chain_verbose;
            for (int i = 0; i < n; ++i) seg_len[i] = 0, unfused[i] = false;
            if (seg_G) for (int i = 0; i < n; ++i) seg_G[i] = 0;
            int i = 0;
            for (size_t e = 0; e < now.chain_plan.size(); ++e) {
                const ChainPlanSeg &sp = now.chain_plan[e];
                const int len = std::max(sp.len, 1);
                const std::string what = "MF_CHAIN_PLAN segment " + std::to_string(e) + " (" + std::to_string(sp.len) + ":" + std::to_string(sp.G) + ":" +
                                         std::to_string(sp.dbuf) + ", pairs " + std::to_string(i) + ".." + std::to_string(i + len - 1) + " of " + std::to_string(n) + ")";
                if (i + len > n) fail(MF_ERR_UNSUPPORTED, what + ": past the end of the run");
                seg_len[i] = len;
                const k::ChainArgs *made = nullptr;
                std::unique_ptr<FusedImpl> trial;
                if (sp.len == 0) {
                    unfused[i] = true;
                } else if (sp.len == 1) {
                    if (sp.G > 0 || sp.dbuf >= 0) {
                        trial.reset(chain_create(&groups[i]->chain_members[0], 1, sp.G, sp.dbuf));
                        if (!trial) fail(MF_ERR_UNSUPPORTED, what + ": no such plan");
                        if (sp.dbuf >= 0 && trial->chain.dbuf != sp.dbuf) fail(MF_ERR_UNSUPPORTED, what + ": the input tile does not fit twice");
                        std::swap(*groups[i], *trial);
                    }
                    made = &groups[i]->chain;
                } else {
                    if (!seg_G) fail(MF_ERR_UNSUPPORTED, what + ": the caller takes no images per step");
                    trial.reset(fused_chain_create(groups + i, len, sp.G)); // (the caller makes the same one again from seg_G)
                    if (!trial) fail(MF_ERR_UNSUPPORTED, what + ": no such plan");
                    seg_G[i] = sp.G;
                    made = &trial->chain;
                }
                if (verbose) {
                    if (made) fprintf(stderr, "[microflow_amd] chain plan forced: pairs %d..%d G %d dbuf %d nwave %d lds %d\n", i, i + len - 1, made->G, made->dbuf, made->nwave, made->lds_bytes);
                    else fprintf(stderr, "[microflow_amd] chain plan forced: pair %d unfused\n", i);
                }
                i += len;
            }
            if (i != n) fail(MF_ERR_UNSUPPORTED, "MF_CHAIN_PLAN covers " + std::to_string(i) + " pairs of a run of " + std::to_string(n));
            return;
        }
    }
    const bool force_fuse = switches().chain_force; // tests: never prefer the unfused operators
    const double INF = 1e30;
    std::vector<double> best((size_t)n + 1, INF);
    std::vector<int> choice((size_t)n + 1, 1);
    std::vector<char> choice_unf((size_t)n + 1, 0);
    best[(size_t)n] = 0;
    std::vector<k::ChainPair> tab((size_t)k::CHAIN_MAX);
    // measuring is the CALLER's choice (mf_model_set_autotune; off by default: model creation is then deterministic, allocates no
    // scratch and launches nothing); MF_CHAIN_AUTOTUNE=1 / =0 overrides it for scripts
    const int env_tune = switches().chain_autotune;
    bool autotune = env_tune < 0 ? autotune_opt : env_tune != 0;
    const bool verbose_t = switches().chain_verbose;
    const bool tune_g = switches().chain_tune_g;
    // measured[i][len]: microseconds per image of the candidate (< 0: not measured); measured_unf[i]: of the pair's two operators
    std::vector<std::vector<double>> measured((size_t)n, std::vector<double>((size_t)k::CHAIN_MAX + 1, -1.0));
    std::vector<double> measured_unf((size_t)n, -1.0);
    const size_t CAP = (size_t)512 << 20; // upper limit of a scratch tensor: dozens of steps per workgroup also for 2 KB images
    auto tensor_bytes = [&](int i, int len) { // the largest tensor any operator of pairs i .. i + len - 1 touches, per image
        size_t m = 0;
        for (int j = i; j < i + len; ++j) {
            const OpSpec &d = groups[j]->chain_members[0].first->s, &q = groups[j]->chain_members[0].second->s;
            m = std::max(m, std::max((size_t)d.H * d.W * d.C, std::max((size_t)d.OH * d.OW * d.N, (size_t)q.OH * q.OW * q.N)));
        }
        return m;
    };
    auto batch_of = [&](size_t tb) { return std::min<size_t>(CAP / std::max<size_t>(tb, 1), 262144) & ~(size_t)63; };
    if (autotune && n >= 1) {
        size_t need = 0; // the scratch the largest candidate needs (not a fixed 512 MB)
        for (int i = 0; i < n; ++i)
            for (int len = 1; len <= n - i && len <= k::CHAIN_MAX; ++len) need = std::max(need, batch_of(tensor_bytes(i, len)) * tensor_bytes(i, len));
        ChainTimer tm(need + 256);
        for (int i = 0; i < n && tm.ok; ++i) {
            for (int len = 1; len <= n - i && len <= k::CHAIN_MAX; ++len) {
                bool ok = true;
                for (int j = i; j < i + len && ok; ++j)
                    ok = groups[j]->chain_members[0].first->s.u8 == groups[i]->chain_members[0].first->s.u8 && (len == 1 || groups[j]->chain_members[0].first->s.C >= 16);
                if (!ok) break;
                const size_t B = batch_of(tensor_bytes(i, len));
                if (B < 256) continue;
                std::unique_ptr<FusedImpl> owned(len == 1 ? nullptr : fused_chain_create(groups + i, len)); // (freed on every path)
                FusedImpl *f = len == 1 ? groups[i] : owned.get();
                if (!f) continue; // (no plan: longer candidates from i may still exist -- a later pair can be smaller)
                const double t = tm.us([&] { fused_run(f, (const int8_t *)tm.a.p, B, (int8_t *)tm.b.p, tm.st); });
                if (t > 0) measured[(size_t)i][(size_t)len] = t / (double)B;
                if (len == 1 && tune_g && t > 0) {
                    // the single pair's images per step and double buffering, measured: every multiple of the column grids' images up to
                    // 4x / down to 1/4 of the planner's choice, with and without the second input buffer.  The winner's plan replaces
                    // the group's in place.
                    const int G0 = groups[i]->chain.G, cg = std::max(1, groups[i]->chain.max_cg), db0 = groups[i]->chain.dbuf;
                    double best_t = t;
                    std::unique_ptr<FusedImpl> best_f;
                    const int cands[8] = {G0 / 4, G0 / 2, 3 * G0 / 4, G0, 3 * G0 / 2, 2 * G0, 3 * G0, 4 * G0};
                    for (int ci = 0; ci < 8; ++ci) {
                        const int G = cands[ci];
                        if (G < cg || G > 128 || G % cg != 0 || (ci > 0 && G == cands[ci - 1])) continue;
                        for (int db = 0; db < 2; ++db) {
                            if (G == G0 && db == db0) continue;
                            std::unique_ptr<FusedImpl> cand(chain_create(&groups[i]->chain_members[0], 1, G, db));
                            if (!cand || cand->chain.dbuf != db) continue;
                            const double tc = tm.us([&] { fused_run(cand.get(), (const int8_t *)tm.a.p, B, (int8_t *)tm.b.p, tm.st); });
                            if (verbose_t) fprintf(stderr, "[microflow_amd] chain autotune: pair %d G %d dbuf %d: %.4f us/image (planner's G %d dbuf %d: %.4f)\n", i, G, db, tc / (double)B, G0, db0, t / (double)B);
                            if (tc > 0 && tc < (best_f ? best_t : t * 0.96)) best_t = tc, best_f = std::move(cand); // (a clear win over the planner's: 4 %)
                        }
                    }
                    if (best_f) {
                        std::swap(*groups[i], *best_f);
                        measured[(size_t)i][1] = best_t / (double)B;
                    }
                }
                if (len == 1) {
                    OpImpl *dw = groups[i]->chain_members[0].first, *pw = groups[i]->chain_members[0].second;
                    const double u = tm.us([&] {
                        op_run(dw, (const int8_t *)tm.a.p, B, (int8_t *)tm.c.p, tm.st);
                        op_run(pw, (const int8_t *)tm.c.p, B, (int8_t *)tm.b.p, tm.st);
                    });
                    if (u > 0) measured_unf[(size_t)i] = u / (double)B;
                }
                if (verbose_t)
                    fprintf(stderr, "[microflow_amd] chain autotune: pairs %d..%d batch %zu: %.4f us/image%s\n", i, i + len - 1, B, measured[(size_t)i][(size_t)len],
                            len == 1 ? (" (unfused " + std::to_string(measured_unf[(size_t)i]) + ")").c_str() : "");
            }
        }
        if (tm.st) (void)hipStreamSynchronize(tm.st);
        (void)hipGetLastError();
        // The measurements are used only as a whole: every pair must have its own time (measured us/image of the chip and estimated
        // us/image per CU are different units and must never meet in one sum); a launch that threw, a pair too large for the scratch
        // or a failed timer send the whole run back to the estimates.
        bool complete = tm.ok && !tm.failed;
        for (int i = 0; i < n && complete; ++i) complete = measured[(size_t)i][1] > 0;
        if (!complete) {
            if (verbose_t || switches().verbose) fprintf(stderr, "[microflow_amd] chain autotune incomplete: planning %d pairs from the cost model\n", n);
            autotune = false;
        }
    }
    for (int i = n - 1; i >= 0; --i) {
        for (int len = 1; len <= n - i && len <= k::CHAIN_MAX; ++len) {
            if (autotune) { // measured costs (a candidate that was not measured does not exist)
                double c = measured[(size_t)i][(size_t)len];
                if (c <= 0) continue;
                if (len > 1) c *= 1.05; // (a chain has to win clearly: isolated timings of this size repeat to 2 - 3 %)
                char unf = 0;
                if (len == 1 && !force_fuse && measured_unf[(size_t)i] > 0 && measured_unf[(size_t)i] < c) c = measured_unf[(size_t)i], unf = 1;
                if (c + best[(size_t)i + len] < best[(size_t)i]) best[(size_t)i] = c + best[(size_t)i + len], choice[(size_t)i] = len, choice_unf[(size_t)i] = unf;
                continue;
            }
            k::ChainArgs a{};
            bool ok = true;
            for (int j = i; j < i + len && ok; ++j)
                ok = groups[j]->chain_members[0].first->s.u8 == groups[i]->chain_members[0].first->s.u8 && (len == 1 || groups[j]->chain_members[0].first->s.C >= 16);
            if (!ok || !k::chain_plan(geo.data() + i, len, tab.data(), a, 150 * 1024)) {
                if (len == 1) { // (cannot happen for a group that exists; keep the programme total)
                    if (best[(size_t)i + 1] < best[(size_t)i]) best[(size_t)i] = best[(size_t)i + 1], choice[(size_t)i] = 1, choice_unf[(size_t)i] = 1;
                }
                continue;
            }
            double c = a.est_us_per_image;
            char unf = 0;
            if (len == 1 && !force_fuse) {
                const double u = k::chain_unfused_us_per_image(geo.data() + i, 1);
                if (u < c) c = u, unf = 1;
            }
            if (c + best[(size_t)i + len] < best[(size_t)i]) best[(size_t)i] = c + best[(size_t)i + len], choice[(size_t)i] = len, choice_unf[(size_t)i] = unf;
        }
    }
    for (int i = 0; i < n; ++i) seg_len[i] = 0, unfused[i] = false;
    for (int i = 0; i < n; i += choice[(size_t)i]) seg_len[i] = choice[(size_t)i], unfused[i] = choice_unf[(size_t)i] != 0;
    // the images per step of the chosen multi-pair chains, measured like the single pairs' (1/2 ... 2x the planner's)
    if (seg_G) {
        for (int i = 0; i < n; ++i) seg_G[i] = 0;
        if (autotune && tune_g) {
            std::unique_ptr<ChainTimer> tm;
            for (int i = 0; i < n; ++i) {
                const int len = seg_len[i];
                if (len < 2) continue;
                if (!tm) {
                    size_t need2 = 0;
                    for (int i2 = 0; i2 < n; ++i2)
                        if (seg_len[i2] >= 2) need2 = std::max(need2, batch_of(tensor_bytes(i2, seg_len[i2])) * tensor_bytes(i2, seg_len[i2]));
                    tm.reset(new ChainTimer(need2 + 256));
                }
                if (!tm->ok || tm->failed) break;
                const size_t B = batch_of(tensor_bytes(i, len));
                std::unique_ptr<FusedImpl> base(fused_chain_create(groups + i, len, 0));
                if (!base || B < 256) continue;
                const double t0 = tm->us([&] { fused_run(base.get(), (const int8_t *)tm->a.p, B, (int8_t *)tm->b.p, tm->st); });
                const int G0 = base->chain.G, cg = std::max(1, base->chain.max_cg);
                double best_t = t0;
                const int cands[4] = {G0 / 2, 3 * G0 / 4, 3 * G0 / 2, 2 * G0};
                for (int ci = 0; ci < 4 && t0 > 0; ++ci) {
                    const int G = cands[ci];
                    if (G < cg || G > 128 || G % cg != 0 || G == G0) continue;
                    std::unique_ptr<FusedImpl> cand(fused_chain_create(groups + i, len, G));
                    if (!cand) continue;
                    const double tc = tm->us([&] { fused_run(cand.get(), (const int8_t *)tm->a.p, B, (int8_t *)tm->b.p, tm->st); });
                    if (verbose_t) fprintf(stderr, "[microflow_amd] chain autotune: chain %d..%d G %d: %.4f us/image (planner's G %d: %.4f)\n", i, i + len - 1, G, tc / (double)B, G0, t0 / (double)B);
                    if (tc > 0 && tc < (seg_G[i] ? best_t : t0 * 0.96)) best_t = tc, seg_G[i] = G;
                }
            }
            if (tm && tm->st) (void)hipStreamSynchronize(tm->st);
            (void)hipGetLastError();
        }
    }
    const bool verbose = switches().chain_verbose || switches().verbose; // the plan, so that a run can be reproduced
    if (verbose) {
        fprintf(stderr, "[microflow_amd] chain partition of %d pairs:", n);
        for (int i = 0; i < n; ++i)
            if (seg_len[i]) fprintf(stderr, " [%d..%d%s]", i, i + seg_len[i] - 1, unfused[i] ? " unfused" : "");
        fprintf(stderr, " %s %.4f us/image%s\n", autotune ? "measured" : "est", best[0], autotune ? "" : "/CU");
    }
}

} // namespace mf
