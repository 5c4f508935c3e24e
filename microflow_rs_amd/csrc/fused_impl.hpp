// fused_impl.hpp -- what the fused-group units share: the group itself, the per-kind facts its launch path and predicates read, the
// one test for "a depthwise 3x3 + 1x1 pair", and the helpers every builder uses.  Internal to fused.hip, fused_pairs.hip,
// fused_heads.hip, fused_stages.hip and chain_partition.hip.  Host code only.
#pragma once
#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "ops_impl.hpp"
#include "wimage.hpp"

namespace mf {

// One argument block (or a named sub-struct: block + what the launch path needs beside it) per kind; a group uses its own kind's.
// Plain members, no variant: the chain planner swaps whole groups (std::swap(*groups[i], *trial)).
struct FusedImpl {
    enum Kind { DWPW, TAIL, FCSM, STAGE, DWFC, PAIRTAIL, QUAD, CHAIN, FCCHAIN, POOLFC, PAIRBAND, PAIRWZ, CONV1FC, BLOCK, CONVPOOL, SHORTCUT, PADCONV, SIDECONCAT } kind = DWPW;
    OpImpl *a = nullptr, *b = nullptr, *c = nullptr;
    std::string name;
    std::vector<std::unique_ptr<DevBuf>> owned; // the group's own operand arrays and tables (keep)
    k::DwPwArgs dwpw{};
    k::TailArgs tail{};
    // STAGE: the whole late stage in one kernel
    struct Stage {
        k::StageArgs args{};
        int pairs = 0;
    } stage;
    // DWFC: one-input-channel depthwise -> FullyConnected -> Softmax in one kernel
    k::DwFcArgs dwfc{};
    // PAIRTAIL: the last pair + the tail in one kernel; with the pair in front of it in the same launch (has_front; k_tail3.hip FRONT)
    struct PairTail {
        k::PairTailArgs args{};
        k::PairFrontArgs front{};
        bool has_front = false;
    } pairtail;
    // QUAD: two consecutive pairs in one kernel (k_quad.hip); a = the first pair's depthwise, b = the second pair's conv
    struct Quad {
        k::QuadArgs args{};
        bool mm = false; // the C = 64 quad (k_quad_mm.hip): intermediate tensors through LDS, the pairs' dwpw_mm argument blocks
        int shape[10] = {0};
        OpImpl *ops[4] = {nullptr, nullptr, nullptr, nullptr}; // the two pairs' operators (the stem variant rebuilds the blocks from them)
    } quad;
    // CHAIN: 1 .. CHAIN_MAX consecutive pairs of any geometry in one launch (k_chain.hip)
    struct Chain {
        k::ChainArgs args{};
        std::vector<std::pair<OpImpl *, OpImpl *>> members;
    } chain;
    // FCCHAIN: consecutive FullyConnected layers (+ Softmax) in one launch (k_fc_rt.hip fc_chain); the layers' fc_rt images
    struct FcChain {
        k::FcChainArgs args{};
        long long M = 1; // rows per inference
    } fcchain;
    // POOLFC: the global AveragePool2D + FullyConnected layers (+ Softmax) in one launch (k_pool_fc.hip pool_fc_chain); a = the pool
    k::PoolFcArgs poolfc{};
    // PAIRBAND: one pair too large for chain_rt's LDS plan, walked in row bands (k_pair_band.hip); a = the depthwise, b = the conv
    k::PairBandArgs pairband{};
    // PAIRWZ: one pair with filter zero points, whole images in LDS (k_pair_wz.hip); a = the depthwise, b = the conv
    k::PairWzArgs pairwz{};
    // CONV1FC: a one-input-channel convolution + FullyConnected (+ Softmax) in one launch (k_conv1_fc.hip); a = the convolution, b = the
    // FullyConnected, c = the Softmax or nullptr
    struct Conv1Fc {
        k::Conv1FcArgs args{};
        size_t max_batch = 0; // 0: any batch; else the largest batch at which the launch beat the operators' own (fused_batch_ok)
    } conv1fc;
    // BLOCK: a 1x1 expand + depthwise 3x3 + 1x1 project block in row bands (k_block_band.hip); a = the expand, b = the depthwise, c = the project
    k::BlockBandArgs block{};
    size_t block_max_batch = 0; // 0: any batch; else the largest batch at which the block launch runs (fused_batch_ok): above it the launches it replaces
    // CONVPOOL: a Conv2D + the AveragePool2D (k_conv_pool.hip) or MaxPool2D (mx; k_conv_maxpool.hip) on its output in one launch;
    // a = the convolution, b = the pool
    struct ConvPool {
        k::ConvPoolArgs args{};
        bool wz = false; // the convolution has non-zero filter zero points (internal domain)
        bool mx = false; // the pool is a MaxPool2D: conv_maxpool_rt
    } convpool;
    // SHORTCUT: a 1x1 shortcut convolution + the ADD on its result and the running tensor (k_side_join.hip); a = the convolution, b = the
    // ADD.  With SIDECONCAT the kinds with TWO inputs: fused_run2, never the launch path of the others
    k::ShortcutAddArgs shortcut{};
    // SIDECONCAT: a 1x1 Conv2D on a skip edge + the CONCATENATION of its result and the running tensor (k_side_join.hip); a = the
    // convolution, b = the CONCATENATION.  Two inputs, as SHORTCUT: fused_run2
    k::SideConcatArgs sideconcat{};
    // PADCONV: a PAD + the VALID Conv2D / DepthwiseConv2D on its output as one launch of the convolution's own run-time-geometry kernel;
    // a = the PAD, b = the convolution.  padconv = that convolution taken as an operator on the UNPADDED image with the PAD's top / left
    // rows and columns as its window placement (ops.hip op_create_padded_conv): it borrows b's weights and constants, owns the images
    // and tables of its plan, and has no generic kernel -- the group runs it on 16-byte aligned pointers only
    std::shared_ptr<OpImpl> padconv;
    // the model's f32 boundary inside this group's launch (fused_set_input_quant / fused_set_output_dequant; KindFacts f32_in / f32_out)
    k::F32Edge edge{};
    bool edge_in = false, edge_out = false;
    int epi_mode = -1; // epilogue mode (k_common.hpp) of the launch's requantising operators; -1: not recorded (the operators' minimum)
};

// What the launch path (fused.hip) and the predicates need to know of a kind.  No `default`: -Wall names a kind that is missing here
// (the return behind the switch is there for -Wreturn-type alone; the warning-free build is what keeps a kind from reaching it).
struct KindFacts {
    const char *in16;      // the launch reads 16-byte words at the input pointer: its name in the error text; nullptr: any pointer
    bool batch_limit;      // at most 0x7fffffff / 4 images per launch (PAIRBAND: / NB of that); the others take any size_t
    bool f32_in, f32_out;  // the launch takes the model's f32 entry / exit (the stem quad's entry is its stem operator's: fused_accepts_f32)
};
inline KindFacts kind_facts(FusedImpl::Kind kind) {
    switch (kind) {
    case FusedImpl::DWPW: return {nullptr, true, false, false};
    case FusedImpl::TAIL: return {nullptr, false, false, false};
    case FusedImpl::FCSM: return {nullptr, false, false, false};
    case FusedImpl::STAGE: return {nullptr, true, false, false};
    case FusedImpl::DWFC: return {nullptr, false, true, true};
    case FusedImpl::PAIRTAIL: return {nullptr, false, false, true};
    case FusedImpl::QUAD: return {nullptr, true, false, false};
    case FusedImpl::CHAIN: return {nullptr, true, false, false};
    case FusedImpl::FCCHAIN: return {nullptr, false, true, true}; // (no pointer alignment needed: fc_chain aligns its DMA and stores itself)
    case FusedImpl::POOLFC: return {"pool_fc_chain", false, false, true};
    case FusedImpl::PAIRBAND: return {"pair_band_rt", true, false, false};
    case FusedImpl::PAIRWZ: return {"pair_wz_rt", true, false, false};
    case FusedImpl::CONV1FC: return {"conv1_fc_rt", false, false, false};
    case FusedImpl::BLOCK: return {"block_band_rt", true, false, false};
    case FusedImpl::CONVPOOL: return {"conv_pool_rt", true, false, false};
    case FusedImpl::PADCONV: return {"pad+conv", true, false, false};
    case FusedImpl::SIDECONCAT: return {nullptr, false, false, false}; // (as SHORTCUT)
    case FusedImpl::SHORTCUT: return {nullptr, false, false, false}; // (16-byte words at all three pointers, the caller's output buffer among them: fused_run2 checks the alignment itself)
    }
    return {nullptr, false, false, false};
}
// the most images one launch of the group takes; 0: any size_t.  The band kernels (conv_pool_rt among them) count steps, NB bands per image.  A launch with an
// f32 end (`edge`) is limited whatever the kind: batch x 4 bytes per element stay below 2^31
inline size_t batch_limit(const FusedImpl &f, int edge) {
    if (!kind_facts(f.kind).batch_limit && !edge) return 0;
    return 0x7fffffffull / 4 / (f.kind == FusedImpl::PAIRBAND ? (size_t)f.pairband.NB : f.kind == FusedImpl::BLOCK ? (size_t)f.block.b.NB :
                                 f.kind == FusedImpl::CONVPOOL ? (size_t)f.convpool.args.NB : 1);
}

inline std::unique_ptr<FusedImpl> make_group(FusedImpl::Kind kind, OpImpl *a, OpImpl *b, OpImpl *c, std::string name) {
    std::unique_ptr<FusedImpl> f(new FusedImpl);
    f->kind = kind, f->a = a, f->b = b, f->c = c, f->name = std::move(name);
    return f;
}

// ---- the pair every pair kernel starts from ----
// the depthwise member's argument block where it runs a table kernel or dw3x3_rt; nullptr: another kernel
inline const k::DwFastArgs *dw_fast(const OpImpl *dw) {
    return dw->fast == OpImpl::DW_NHWC ? &dw->dwf : dw->fast == OpImpl::DW_RT ? &dw->dwrt.dw : nullptr;
}
struct PairMatch {
    const OpSpec *d = nullptr, *q = nullptr; // the depthwise's and the 1x1's spec; nullptr: not such a pair
    const k::DwFastArgs *f = nullptr;        // dw_fast(dw)
    k::ChainGeom geom{};                     // the pair as the planners take it (izp4 from f; 0 without)
    explicit operator bool() const { return d != nullptr; }
};
// A DepthwiseConv2D 3x3 SAME with equal strides 1 or 2 and one output per channel, followed by a Conv2D 1x1 at stride 1 on exactly
// its output; same device, same element type, finite constants.  ONLY what chain_pair_ok, pair_band_create, pair_wz_create,
// fused_pair_tail_create and fused_front_pair_tail_create all ask: which kernels the members run alone, filter zero points, channel
// ranges, width rules and force_generic differ between them and stay with each caller.
inline PairMatch match_dw3x3_pw1x1(const OpImpl *dw, const OpImpl *pw) {
    PairMatch no;
    if (!dw || !pw) return no;
    const OpSpec &d = dw->s, &q = pw->s;
    // (the pair + tail builders do not spell out the next two lines: their pair is an existing DWPW or single-pair CHAIN group, whose
    // builder compared the devices, and both demand Fast kinds that only a DepthwiseConv2D / Conv2D ever gets -- ops.hip's routes)
    if (dw->device != pw->device) return no;
    if (d.kind != MF_OP_DEPTHWISE_CONV_2D || q.kind != MF_OP_CONV_2D) return no;
    if (d.u8 != q.u8) return no;
    if (d.KH != 3 || d.KW != 3 || d.pad != MF_PAD_SAME || d.C != d.N) return no;
    // (pair + tail demands sh == sw == 1; front pair + tail sh == sw and pair_front_supported's stride, 2)
    if (d.sh != d.sw || (d.sh != 1 && d.sh != 2)) return no;
    // (pair + tail and front pair + tail test KH, KW only: the 1x1 kinds they demand, PW_MFMA / PW_RT, are given at stride 1 alone)
    if (q.KH != 1 || q.KW != 1 || q.sh != 1 || q.sw != 1 || q.OH != q.H || q.OW != q.W) return no;
    // (pair + tail and front pair + tail test q.C only: H and W were compared when their pair's group was built)
    if (q.H != d.OH || q.W != d.OW || q.C != d.N) return no;
    if (!dw->finite_consts || !pw->finite_consts) return no;
    PairMatch m;
    m.d = &d, m.q = &q, m.f = dw_fast(dw);
    m.geom = k::ChainGeom{d.H, d.W, d.C, d.sh, d.OH, d.OW, q.N, m.f ? m.f->izp4 : 0u};
    return m;
}
// ---- the block block_band_rt starts from (k_block_band.hip) ----
// A Conv2D 1x1 at stride 1 (the expand, C -> E) on exactly the input of a pair match_dw3x3_pw1x1 accepts (depthwise on E, project
// E -> N), with the tensor inside the widest: E > C and E > N.  One device, one element type, finite constants, zero filter zero points
// in the i8 domain on all three, none forced generic, W even at stride 2, and the channel ranges of block_band_plan.  Everything
// fused_block_create asks short of the plan, the compiled instance and the measured exclusions.
struct BlockMatch {
    PairMatch pair;      // the depthwise + project pair (geom.C = E; geom.izp4 = the depthwise's input zero point in every byte)
    int CI = 0;          // the expand's input channels
    bool ok = false;
    explicit operator bool() const { return ok; }
};
inline BlockMatch match_expand_block(const OpImpl *ex, const OpImpl *dw, const OpImpl *pw) {
    BlockMatch no, m;
    m.pair = match_dw3x3_pw1x1(dw, pw);
    if (!ex || !m.pair) return no;
    const OpSpec &e = ex->s, &d = *m.pair.d, &q = *m.pair.q;
    if (e.kind != MF_OP_CONV_2D || ex->device != dw->device || e.u8 != d.u8 || !ex->finite_consts) return no;
    if (e.KH != 1 || e.KW != 1 || e.sh != 1 || e.sw != 1 || e.OH != e.H || e.OW != e.W) return no;
    if (e.H != d.H || e.W != d.W || e.N != d.C) return no; // on exactly the depthwise's input
    if (ex->force_generic || dw->force_generic || pw->force_generic) return no; // (generic operators stay launches of their own)
    for (const OpImpl *o : {ex, dw, pw})
        for (int32_t z : o->h_wzp)
            if (z != 0) return no;
    if (d.sh == 2 && d.W % 2 != 0) return no; // (the plan's stride-2 column units)
    const int C = e.C, E = d.C, N = q.N;
    if (E <= C || E <= N) return no; // the tensor inside is the widest: what makes the launch pay, and what no chain of pairs has
    if (E % 16 != 0 || E < 32 || E > 256 || C % 4 != 0 || C < 4 || C > 128 || N % 4 != 0 || N < 4 || N > 256) return no;
    m.pair.geom.izp4 = 0x01010101u * (uint32_t)(uint8_t)(int8_t)dw->conv.izp; // (whatever kernel the depthwise runs alone)
    m.CI = C, m.ok = true;
    return m;
}
// the pair's ten requantisation constants, from the members' argument blocks (A, S, Kc, lo_f, hi_f), into any block that names them
// dwA .. pw_hi; the operand images differ per kernel and stay with the caller
template <typename T, typename D, typename P> void set_pair_consts(T &dst, const D &dw, const P &pw) {
    dst.dwA = dw.A, dst.dwS = dw.S, dst.dwK = dw.Kc, dst.dw_lo = dw.lo_f, dst.dw_hi = dw.hi_f;
    dst.pwA = pw.A, dst.pwS = pw.S, dst.pwK = pw.Kc, dst.pw_lo = pw.lo_f, dst.pw_hi = pw.hi_f;
}
// "HxWxC[s2]-N", the pair inside a group's name
inline std::string pair_label(const OpSpec &d, const OpSpec &q) {
    return std::to_string(d.H) + "x" + std::to_string(d.W) + "x" + std::to_string(d.C) + (d.sh == 2 ? "s2" : "") + "-" + std::to_string(q.N);
}

// the pair's argument blocks as the operators hold them (two-rounding constants), and switched to the single-fma form when
// both operators have it
// fma: 0 = the two-rounding constants; 1 = the single-fma form if both operators have it WITHOUT patched accumulators (quads,
// register-resident pairs); 2 = ... with or without (dwpw_mm, the stage: kernels that apply the patch list)
inline k::DwPwArgs pair_args(const OpImpl *dw, const OpImpl *pw, int fma) {
    k::DwPwArgs a;
    a.dw = dw->dwf, a.pw = pw->pw;
    if ((fma == 1 && dw->fma_strict() && pw->fma_strict()) || (fma == 2 && dw->fma_ok && pw->fma_ok)) a.dw.use_fma(true), a.pw.use_fma(true);
    return a;
}
inline int pair_mode(const k::DwPwArgs &a) { return std::min(a.dw.magic, a.pw.magic); }
// An operator's patch list as the table a kernel reads: one EpiPatchRec per tile, `tile_of(channel, reg, lane_group)` = the tile
// index of the channel in that kernel (and which of a lane's four accumulators / which 16-lane group hold it).  false: two patched
// channels share a tile -- the kernel's record holds one -- so this launch cannot use the single-fma form.
template <typename F> bool patch_table(const k::EpiPatch &pl, std::vector<k::EpiPatchRec> &tab, size_t base, F tile_of) {
    for (int e = 0; e < pl.n; ++e) {
        int reg = 0, grp = 0;
        const int t = tile_of(pl.ch[e], reg, grp);
        if (t < 0 || base + (size_t)t >= tab.size() || tab[base + (size_t)t].P != 0) return false;
        tab[base + (size_t)t] = k::epi_patch_rec(pl.P[e], pl.R[e], reg, grp);
    }
    return true;
}

// a device array the group owns: uploaded now, freed with the group
inline const void *keep(FusedImpl &f, const void *src, size_t bytes) {
    f.owned.emplace_back(new DevBuf);
    f.owned.back()->upload(src, bytes);
    return f.owned.back()->p;
}
// the host copy of the Kc array an operator's argument block points at: its two-rounding constants or its single-fma ones
inline const std::vector<int32_t> &host_kc(const OpImpl *op, const int *d_kc) { return d_kc == op->d_Kc3.as<int>() ? op->h_Kc3 : op->h_Kc; }
// Kc + the bit-pattern offset of requant_t<true> (k_common.hpp), as an array of the group's own
inline const int *kc_with_magic(FusedImpl &owner, const std::vector<int32_t> &h_Kc) {
    std::vector<int32_t> h = h_Kc;
    for (int32_t &v : h) v = wrap_add(v, 0x4B400000);
    return (const int *)keep(owner, h.data(), h.size() * 4);
}
// a 1x1 convolution's weights ([N][1][1][C], i8 domain, as uploaded) as the stage and tail kernels' operand A
inline const void *plain_pw_image(FusedImpl &owner, const OpImpl *pw) {
    const std::vector<int8_t> prep = wimage::build_pw_plain_weights(pw->h_w.data(), pw->s.C, pw->s.N);
    return keep(owner, prep.data(), prep.size());
}
// a planned pair's unit offset table (k::chain_rtab), as an array of the group's own
inline void upload_rtab(FusedImpl &group, k::ChainPair &pair) {
    std::vector<int> rt;
    k::chain_rtab(pair, rt);
    pair.rtab = (const int *)keep(group, rt.data(), rt.size() * sizeof(int));
}

// ---- FullyConnected layers, a Softmax behind them, a global pool in front (fused_heads.hip) ----
// `n` FullyConnected layers with fc_rt images, M rows per inference, of one element type on one device, as a.l[0 .. n-1]; the launch's
// mode is their minimum.  false: a member is not such a layer
inline bool fc_layers_fill(OpImpl *const *fcs, int n, k::FcChainArgs &a, int M, bool u8, int device) {
    a = k::FcChainArgs{};
    a.L = n;
    int mode = 3;
    for (int l = 0; l < n; ++l) {
        const OpImpl *o = fcs[l];
        if (!o || o->s.kind != MF_OP_FULLY_CONNECTED || !o->fcrt_ok || o->s.M != M || o->s.u8 != u8 || o->device != device) return false;
        const k::FcRtArgs &f = o->fcrt;
        k::FcChainLayer &y = a.l[l];
        y.wimg = f.wimg, y.A = f.A, y.Kc = f.Kc, y.S = f.S, y.lo_f = f.lo_f, y.hi_f = f.hi_f, y.K = f.K, y.N = f.N, y.wzp = f.wzp;
        mode = std::min(mode, f.magic);
    }
    a.magic = mode, a.xr = fcs[0]->fcrt.xr;
    return true;
}
// a Softmax over exactly the N outputs of one row, of this element type on this device
inline bool softmax_over_row(const OpImpl *sm, int N, bool u8, int device) {
    return sm && sm->s.kind == MF_OP_SOFTMAX && sm->s.M == 1 && sm->s.N == N && sm->s.u8 == u8 && sm->device == device;
}
// the tap shift of a pool's single window (focus (0,0); src/tensor.rs:180-228): tap (ky, kx) reads pixel (ky - shy, kx - shx)
inline void pool_window_shift(const OpSpec &p, int &shy, int &shx) {
    shy = p.pad == MF_PAD_SAME ? (p.KH - 1) / 2 : 0, shx = p.pad == MF_PAD_SAME ? (p.KW - 1) / 2 : 0;
}

// ---- between the units ----
// fused_pairs.hip, for the planner (chain_partition.hip): the geometry the planner sees, and `n` pairs as one chain_rt launch
k::ChainGeom chain_geom(const OpImpl *dw, const OpImpl *pw);
std::unique_ptr<FusedImpl> chain_create(const std::pair<OpImpl *, OpImpl *> *mem, int n, int force_G = 0, int force_dbuf = -1);

} // namespace mf
