// model_groups.cpp -- the grouping rules of the model runtime: which operators of a parsed model run as one launch.  One function
// per rule over a builder; build_groups at the end of the file lists them in the order they depend on.
#include <cmath>
#include <memory>

#include "model_groups.hpp"

namespace mf {

void ModelGroups::clear() {
    for (const Stage &st : stages) fused_destroy(st.f); // they borrow the groups' buffers: first
    for (FusedImpl *f : side_join) fused_destroy(f);
    for (FusedImpl *f : fused) fused_destroy(f);
    for (OpImpl *o : ops) op_destroy(o);
    stages.clear(), side_join.clear(), fused.clear(), fused_last.clear(), ops.clear();
}

bool group_splits(const ParsedModel &pm, size_t first, size_t last) {
    for (size_t k = 0; k < pm.ops.size(); ++k) {
        if (pm.ops[k].side() && k >= first && k <= last) return true;
        if (!pm.ops[k].join()) continue;
        if (k >= first && k <= last) return true;
        const int s = pm.skip_real(k);
        if (s >= (int)first && s < (int)last) return true;
    }
    return false;
}

int side_join_candidate(const ParsedModel &pm, size_t join) {
    const int s = pm.side_of_join(join);
    if (s < 0) return -1;
    const ParsedOp &po = pm.ops[(size_t)s], &pj = pm.ops[join];
    bool zero_wzp = true, finite = std::isfinite(pj.c0[0]) && std::isfinite(pj.c1[0]);
    for (int z : po.wzp) zero_wzp = zero_wzp && z - (pm.u8 ? 128 : 0) == 0;
    for (float c : po.c0) finite = finite && std::isfinite(c);
    for (float c : po.c1) finite = finite && std::isfinite(c);
    OpSpec d;
    d.kind = po.kind, d.KH = po.KH, d.KW = po.KW, d.sh = po.sh, d.sw = po.sw, d.H = po.H, d.W = po.W, d.C = po.C, d.N = po.N, d.OH = po.OH, d.OW = po.OW;
    if (pj.kind == MF_OP_ADD) return shortcut_add_class(d, zero_wzp, finite) ? s : -1;
    return side_concat_class(d, pj.run_input == 0 ? pj.cat_ca : pj.cat_cb, zero_wzp, finite) ? s : -1; // (the running operand's channels)
}

namespace {

// The groups under construction, the parsed model, and what the rules ask about both.
struct GroupBuilder {
    const ParsedModel &pm;
    const int device;
    const bool autotune;
    ModelGroups g;
    size_t n = 0; // operators, Reshapes included

    const ParsedOp &po(size_t i) const { return pm.ops[i]; }
    int kind(size_t i) const { return pm.ops[i].kind; }
    void add_stage(FusedImpl *f, size_t first, size_t last) { g.stages.push_back({f, (int)first, (int)last}); }
    // inside a second-level stage built so far
    bool covered(size_t i) const {
        for (const ModelGroups::Stage &st : g.stages)
            if ((int)i >= st.first && (int)i <= st.last) return true;
        return false;
    }
    // swallowed by a first-level group that starts before it
    bool owned(size_t i) const {
        for (size_t j = 0; j < i; ++j)
            if (g.fused[j] && g.fused_last[j] >= (int)i) return true;
        return false;
    }
    // a first-level pair group: operators i and i + 1
    // (a depthwise + 1x1 pair of rule (1): the PAD + convolution group has two operators too and is none)
    bool is_pair_group(size_t i) const { return g.fused[i] && g.fused_last[i] == (int)i + 1 && kind(i) != MF_OP_PAD; }
    // an operator with a launch of its own that no group starts at, covers or owns
    bool free_op(size_t i) const { return g.ops[i] && !g.fused[i] && !covered(i) && !owned(i); }
    bool free_fc(size_t i) const { return i < n && kind(i) == MF_OP_FULLY_CONNECTED && free_op(i); }
    bool free_sm(size_t i) const { return i < n && kind(i) == MF_OP_SOFTMAX && free_op(i); }
    // A fork tensor -- an operator's output that a later join (ADD, CONCATENATION) reads beside the running value -- has to exist in memory, so no group
    // may hold one strictly inside: true when operators first .. last as ONE launch would swallow such a tensor (the operator that
    // launches it at or behind `first` and in front of `last`; a group may end at one or start behind one), or would hold a join,
    // which is a launch of its own.  A candidate this refuses falls back exactly as an unmatched one does
    // A side operator (ParsedOp::side) runs at its join, not at its own index: no group of consecutive operators may hold one either
    bool splits(size_t first, size_t last) const { return group_splits(pm, first, last); }
    size_t skip_reshapes(size_t j) const {
        while (j < n && kind(j) == MF_OP_RESHAPE) ++j;
        return j;
    }
};

} // namespace

static OpSpec op_spec(const ParsedModel &pm, const ParsedOp &po, float cur_scale, int cur_zp) {
    OpSpec s;
    s.kind = po.kind;
    s.u8 = pm.u8;
    s.M = po.M, s.K = po.K, s.N = po.N;
    s.H = po.H, s.W = po.W, s.C = po.C, s.KH = po.KH, s.KW = po.KW;
    s.sh = po.sh ? po.sh : 1, s.sw = po.sw ? po.sw : 1, s.pad = po.pad;
    s.OH = po.OH, s.OW = po.OW, s.act = po.act;
    s.izp = cur_zp;          // input.zero_point[0] of the running tensor (conv_2d.rs:56)
    s.in_scale = cur_scale;  // input.scale[0] of the running tensor (softmax.rs:20)
    s.oscale = po.out_scale, s.ozp = po.out_zp;
    s.weights = po.weights.empty() ? nullptr : po.weights.data();
    s.wzp = po.wzp.empty() ? nullptr : po.wzp.data();
    s.nq = (int)po.wzp.size();
    s.c0 = po.c0.empty() ? nullptr : po.c0.data();
    s.c1 = po.c1.empty() ? nullptr : po.c1.data();
    s.nc1 = (int)po.c1.size();
    s.c2 = po.c2.empty() ? nullptr : po.c2.data();
    s.c3 = po.c3;
    if (po.kind == MF_OP_AVERAGE_POOL_2D || po.kind == MF_OP_MAX_POOL_2D) s.pool_c0 = po.c0[0], s.pool_c1 = po.c1[0];
    if (po.kind == MF_OP_ADD) { // (the operands' quantisation is the file's, by input position: izp / in_scale are not used)
        s.add_elems = po.in_elems;
    }
    if (po.kind == MF_OP_CONCATENATION) {
        s.cat_rows = po.cat_rows, s.cat_ca = po.cat_ca, s.cat_cb = po.cat_cb, s.cat_copy_a = po.cat_copy_a, s.cat_copy_b = po.cat_copy_b;
        s.act = MF_ACT_NONE;
    }
    if (po.join()) s.join_za = po.a_zp, s.join_zb = po.b_zp, s.join_ca = po.c0[0], s.join_cb = po.c1[0];
    if (po.kind == MF_OP_PAD)
        for (int k = 0; k < 4; ++k) s.pads[k] = po.pads[k];
    return s;
}

static void create_operators(GroupBuilder &b) {
    std::vector<OpImpl *> &ops = b.g.ops;
    // predict_inner's running tensor: every op stamps its output scale / zero point on
    // it (Tensor::new(output, output_scale, output_zero_point)); Reshape keeps them.
    float cur_scale = b.pm.in_scale;
    int cur_zp = b.pm.in_zp;
    for (const ParsedOp &po : b.pm.ops) {
        ops.push_back(nullptr); // reserve the slot first: a throwing push_back must not leak the operator
        if (po.kind == MF_OP_RESHAPE) continue;
        if (po.side()) { // a side operator reads T, not the running tensor: what T's launcher stamped on it; it stamps nothing itself
            const int t = b.pm.launcher(po.side_src);
            ops.back() = op_create(b.device, op_spec(b.pm, po, t < 0 ? b.pm.in_scale : b.pm.ops[(size_t)t].out_scale, t < 0 ? b.pm.in_zp : b.pm.ops[(size_t)t].out_zp));
            continue;
        }
        ops.back() = op_create(b.device, op_spec(b.pm, po, cur_scale, cur_zp));
        cur_scale = po.out_scale;
        cur_zp = po.out_zp;
    }
    b.n = ops.size();
    b.g.fused.assign(b.n, nullptr);
    b.g.fused_last.assign(b.n, -1);
    b.g.side_join.assign(b.n, nullptr);
    while (b.g.first_real < (int)b.n && !ops[(size_t)b.g.first_real]) ++b.g.first_real;
    b.g.last_real = (int)b.n - 1;
    while (b.g.last_real >= 0 && !ops[(size_t)b.g.last_real]) --b.g.last_real;
    // peephole (0): the boundary quantize of M::predict folds into operator 0 when that is the stem -- unless a join reads the
    // quantised model input later: nothing would materialise it (the runtime never copies a skip tensor)
    if (!ops.empty() && ops[0] && !b.pm.input_skip) (void)op_set_input_quant(ops[0], b.pm.in_scale, b.pm.in_zp, b.pm.u8);
}

// peepholes.  (1) DepthwiseConv2D 3x3 directly followed by a 1x1 Conv2D -> one fused kernel.
// (2) AveragePool2D (1x1 output) -> Conv2D 1x1 -> [Reshape] -> Softmax -> one tail kernel.
// (3) FullyConnected (few outputs, one row) -> [Reshape] -> Softmax -> one kernel.
// (0p) a PAD directly followed by a VALID Conv2D / DepthwiseConv2D -> one launch of the convolution's kernel with explicit pads.
// In the same loop as (1)-(3) and in front of them: the group at i owns the convolution at i + 1 (the loop continues behind it), so a
// depthwise there is never also offered to (1) with the 1x1 behind it -- that pair would be formed over the padded tensor, which this
// launch never writes.  The PAD's output has one reader (the parser's chain: the convolution) unless a join reads it too: splits
static void rule_1_2_3_first_level(GroupBuilder &b) {
    const std::vector<OpImpl *> &ops = b.g.ops;
    std::vector<FusedImpl *> &fused = b.g.fused;
    std::vector<int> &fused_last = b.g.fused_last;
    for (size_t i = 0; i + 1 < b.n; ++i) {
        if (b.kind(i) == MF_OP_PAD && (b.kind(i + 1) == MF_OP_CONV_2D || b.kind(i + 1) == MF_OP_DEPTHWISE_CONV_2D)) {
            if (!b.splits(i, i + 1) && (fused[i] = fused_pad_conv_create(ops[i], ops[i + 1]))) fused_last[i] = (int)i + 1;
        } else if (b.kind(i) == MF_OP_DEPTHWISE_CONV_2D && b.kind(i + 1) == MF_OP_CONV_2D) {
            if (!b.splits(i, i + 1) && (fused[i] = fused_create(ops[i], ops[i + 1]))) fused_last[i] = (int)i + 1;
        } else if (b.kind(i) == MF_OP_AVERAGE_POOL_2D && b.kind(i + 1) == MF_OP_CONV_2D) {
            const size_t j = b.skip_reshapes(i + 2);
            if (j < b.n && b.kind(j) == MF_OP_SOFTMAX && !b.splits(i, j) && (fused[i] = fused_tail_create(ops[i], ops[i + 1], ops[j]))) fused_last[i] = (int)j;
        } else if (b.kind(i) == MF_OP_FULLY_CONNECTED) { // (3) FC -> [Reshape] -> Softmax
            const size_t j = b.skip_reshapes(i + 1);
            if (j < b.n && b.kind(j) == MF_OP_SOFTMAX && !b.splits(i, j) && (fused[i] = fused_fc_softmax_create(ops[i], ops[j]))) fused_last[i] = (int)j;
        }
        if (fused[i]) i = (size_t)fused_last[i]; // groups do not overlap
    }
}

// (4) runs of consecutive pair groups on one tensor shape -> a persistent stage kernel, if one exists for that
// shape and count (fused_stages.hip: fused_stage_create)
static void rule_4_stage_runs(GroupBuilder &b) {
    for (size_t i = 0; i + 1 < b.n; ++i) {
        if (!b.is_pair_group(i)) continue;
        std::vector<FusedImpl *> run;
        size_t a = i;
        while (a + 1 < b.n && b.is_pair_group(a) && b.po(a).H == b.po(i).H && b.po(a).W == b.po(i).W && b.po(a).C == b.po(i).C &&
               b.po(a + 1).N == b.po(i).C && b.po(a).sh == 1 && !(a > i && b.splits(a - 1, a))) { // (a fork tensor ends the run)
            run.push_back(b.g.fused[a]);
            a += 2;
        }
        // the longest prefix of the run a stage kernel accepts (differing zero points, a run longer than the kernel's
        // limit ...); what is left forms the next run
        size_t used = 0;
        for (size_t k = run.size(); k >= 2 && !used; --k)
            if (FusedImpl *f = fused_stage_create(run.data(), (int)k)) {
                b.add_stage(f, i, i + 2 * k - 1);
                used = k;
            }
        if (used) i += 2 * used - 1;             // continue with the pair after the stage
        else if (!run.empty()) i = a - 1;        // no stage for any prefix: continue after the run
    }
}

// (4b) two consecutive pair groups whose shapes have a quad kernel (k_quad.hip: a VALU-bound stride-1 pair with the
// HBM-bound stride-2 pair behind it; the tensor between them stays in LDS)
static void rule_4b_quads(GroupBuilder &b) {
    for (size_t i = 0; i + 3 < b.n; ++i) {
        if (!b.is_pair_group(i) || b.covered(i) || b.covered(i + 2)) continue;
        if (!b.is_pair_group(i + 2)) continue;
        if (b.splits(i, i + 3)) continue;
        if (FusedImpl *f = fused_quad_create(b.g.fused[i], b.g.fused[i + 2])) {
            b.add_stage(f, i, i + 3);
            // ... and with the stem in front of it: ops i - 1 .. i + 3 in one launch.  Both stay: a run that does not
            // start at the stem (mf_model_run_until pieces, the f32 entry whose stem kernel quantises) uses the quad.
            // (The stem test asks owned(i - 1): fused_quad_stem_create takes a one-channel depthwise stem only, and a depthwise operator
            // is a later member of a first-level group in one place -- the convolution of a PAD + convolution group (0p); (1) starts at
            // one, (2) and (3) hold none.  The other operator that can sit there owned, the 1x1 of a pair group at i - 2, is refused by its kind)
            if (i >= 1 && b.g.ops[i - 1] && !b.g.fused[i - 1] && !b.covered(i - 1) && !b.owned(i - 1) && !b.splits(i - 1, i + 3))
                if (FusedImpl *g = fused_quad_stem_create(b.g.ops[i - 1], f)) b.add_stage(g, i - 1, i + 3);
            i += 3;
        }
    }
}

// (4b') the last pair group directly followed by the tail group -> one kernel (fused_stages.hip: fused_pair_tail_create).  Before the
// chain partition below, so that a run-time-geometry pair taken here is not also a candidate there
static void rule_4b1_pair_tail(GroupBuilder &b) {
    const std::vector<FusedImpl *> &fused = b.g.fused;
    for (size_t i = 0; i + 2 < b.n; ++i) {
        if (!b.is_pair_group(i) || b.covered(i)) continue;
        const size_t j = i + 2;
        if (fused[j] && !b.covered(j) && !b.splits(i, (size_t)b.g.fused_last[j]))
            if (FusedImpl *f = fused_pair_tail_create(fused[i], fused[j])) {
                b.add_stage(f, i, (size_t)b.g.fused_last[j]);
                // ... and with the pair group in front of it: ops i - 2 .. the tail's end in one launch.  Both stay (a run that
                // ends before the tail uses the pair groups, mf_model_run_until pieces that start at i the pair + tail stage)
                if (i >= 2 && b.is_pair_group(i - 2) && !b.covered(i - 2) && !b.splits(i - 2, (size_t)b.g.fused_last[j]))
                    if (FusedImpl *g = fused_front_pair_tail_create(fused[i - 2], f)) b.add_stage(g, i - 2, (size_t)b.g.fused_last[j]);
            }
    }
}

// (4c) runs of consecutive run-time-geometry pairs (single-pair chain groups, k_chain.hip): the planner's cost model
// decides how the run is cut into chain launches (chain_partition.hip: fused_chain_partition); a pair that is cheapest as two
// separate launches loses its group
static void rule_4c_chains(GroupBuilder &b) {
    std::vector<FusedImpl *> &fused = b.g.fused;
    auto chain_pair = [&](size_t i) { return b.is_pair_group(i) && fused_is_chain_single(fused[i]) && !b.covered(i); };
    bool chain_runs = false;
    for (size_t i = 0; i + 1 < b.n; ++i) {
        if (!chain_pair(i)) continue;
        chain_runs = true;
        std::vector<FusedImpl *> run;
        size_t a = i;
        for (; a + 1 < b.n && chain_pair(a) && !(a > i && b.splits(a - 1, a)); a += 2) run.push_back(fused[a]); // (a fork tensor ends the run)
        const int rn = (int)run.size();
        std::vector<int> seg((size_t)rn, 0);
        std::unique_ptr<bool[]> unf(new bool[(size_t)rn]);
        std::vector<int> segG((size_t)rn, 0);
        fused_chain_partition(run.data(), rn, seg.data(), unf.get(), segG.data(), b.autotune);
        for (int k = 0; k < rn; ++k) {
            const size_t at = i + 2 * (size_t)k, len = (size_t)seg[(size_t)k];
            if (len >= 2) {
                if (FusedImpl *f = fused_chain_create(run.data() + k, (int)len, segG[(size_t)k])) b.add_stage(f, at, at + 2 * len - 1);
            } else if (len == 1 && unf[(size_t)k]) {
                fused_destroy(fused[at]);
                fused[at] = nullptr, b.g.fused_last[at] = -1;
            }
        }
        i = a - 1;
    }
    // (a forced chain plan that met no run was applied to nothing: the caller must not take the result for that plan's)
    if (!chain_runs && switches().dev && switches_parse().chain_plan_set)
        fail(MF_ERR_UNSUPPORTED, "MF_CHAIN_PLAN segment 0: the model has no run of run-time-geometry pairs");
}

// (4d) Conv2D 1x1 (expand) -> DepthwiseConv2D 3x3 -> Conv2D 1x1 (project) with the tensor inside the widest -> one block_band_rt
// launch (fused_pairs.hip: fused_block_create).  Behind the chain partition, so that a pair a chain of pairs took is not a
// candidate; a first-level pair group at i + 1 stays under the stage (mf_model_run_until pieces use it)
static void rule_4d_expand_blocks(GroupBuilder &b) {
    const std::vector<OpImpl *> &ops = b.g.ops;
    for (size_t i = 0; i + 2 < b.n; ++i) {
        if (b.kind(i) != MF_OP_CONV_2D || !b.free_op(i)) continue;
        if (!ops[i + 1] || !ops[i + 2] || b.covered(i + 1) || b.covered(i + 2) || b.splits(i, i + 2)) continue;
        if (FusedImpl *f = fused_block_create(ops[i], ops[i + 1], ops[i + 2], b.g.fused[i + 1] != nullptr)) {
            b.add_stage(f, i, i + 2);
            i += 2;
        }
    }
}

// (5) DepthwiseConv2D with one input channel -> [Reshape] -> the FullyConnected + Softmax group -> one kernel.
// (The test on operator i asks owned(i): a depthwise operator is a later member of a first-level group in one place, the convolution
// of a PAD + convolution group (0p) -- (1) starts at the depthwise, (2) is pool + Conv2D + Softmax, (3) FullyConnected + Softmax.
// The group at j is a group's FIRST operator, which owned() does not concern)
static void rule_5_dwfc(GroupBuilder &b) {
    for (size_t i = 0; i + 1 < b.n; ++i) {
        if (!b.g.ops[i] || b.g.fused[i] || b.covered(i) || b.kind(i) != MF_OP_DEPTHWISE_CONV_2D || b.owned(i)) continue; // (owned: by a PAD + convolution group)
        const size_t j = b.skip_reshapes(i + 1);
        if (j < b.n && b.g.fused[j] && !b.covered(j) && !b.splits(i, (size_t)b.g.fused_last[j]))
            if (FusedImpl *f = fused_dwfc_create(b.g.ops[i], b.g.fused[j])) b.add_stage(f, i, (size_t)b.g.fused_last[j]);
    }
}

// (5a) a DepthwiseConv2D or Conv2D with one input channel -> [Reshape] -> FullyConnected (one row per inference) -> [Reshape] ->
// [Softmax] -> one conv1_fc_rt launch (fused_heads.hip: fused_conv1_fc_create) at any geometry its plan accepts; speech.tflite's own
// geometry is refused there and keeps (5).  Where the FullyConnected + Softmax already are a group of (3), this stage sits over
// conv .. softmax and that group stays for mf_model_run_until pieces.  One FullyConnected only: a run behind it is left to (6)
static void rule_5a_conv1_fc(GroupBuilder &b) {
    const std::vector<OpImpl *> &ops = b.g.ops;
    for (size_t i = 0; i + 1 < b.n; ++i) {
        if (!b.free_op(i) || (b.kind(i) != MF_OP_DEPTHWISE_CONV_2D && b.kind(i) != MF_OP_CONV_2D) || b.po(i).C != 1) continue;
        const size_t j0 = b.skip_reshapes(i + 1);
        if (j0 >= b.n || !ops[j0] || b.kind(j0) != MF_OP_FULLY_CONNECTED || b.po(j0).M != 1 || b.covered(j0) || b.owned(j0)) continue;
        if (b.splits(i, j0)) continue;
        if (b.g.fused[j0]) {
            const int last = b.g.fused_last[j0];
            if (last > (int)j0 && b.kind((size_t)last) == MF_OP_SOFTMAX && !b.splits(i, (size_t)last))
                if (FusedImpl *f = fused_conv1_fc_create(ops[i], ops[j0], ops[(size_t)last])) b.add_stage(f, i, (size_t)last);
            continue;
        }
        const size_t smi = b.skip_reshapes(j0 + 1);
        OpImpl *sm = b.free_sm(smi) && !b.splits(i, smi) ? ops[smi] : nullptr;
        if (sm && !fused_conv1_fc_fits(ops[i], ops[j0], sm)) sm = nullptr; // (the two operators without the Softmax)
        if (FusedImpl *f = fused_conv1_fc_create(ops[i], ops[j0], sm)) b.add_stage(f, i, sm ? smi : j0);
    }
}

// (5b) AveragePool2D over the whole image -> [Reshape] -> FullyConnected layers (one row per inference) -> [Softmax] -> one
// pool_fc_chain launch (fused_heads.hip: fused_pool_fc_create), the longest run of layers whose images fit.  Before (6), so that the
// FullyConnected run behind a pool is offered here first; what does not fit stays for (6) or keeps its own launches.  Where the
// head's FullyConnected + Softmax already are a group of (3), this stage sits over pool .. softmax and that group stays for
// mf_model_run_until pieces
static void rule_5b_pool_fc(GroupBuilder &b) {
    const std::vector<OpImpl *> &ops = b.g.ops;
    for (size_t i = 0; i + 1 < b.n; ++i) {
        if (!b.free_op(i) || b.kind(i) != MF_OP_AVERAGE_POOL_2D) continue;
        const size_t j0 = b.skip_reshapes(i + 1);
        if (j0 < b.n && b.g.fused[j0] && !b.covered(j0) && b.kind(j0) == MF_OP_FULLY_CONNECTED && b.g.fused_last[j0] > (int)j0 &&
            b.kind((size_t)b.g.fused_last[j0]) == MF_OP_SOFTMAX) {
            OpImpl *fc = ops[j0];
            const size_t last = (size_t)b.g.fused_last[j0];
            if (b.splits(i, last)) continue;
            if (FusedImpl *f = fused_pool_fc_create(ops[i], &fc, 1, ops[last])) b.add_stage(f, i, last);
            continue;
        }
        if (!b.free_fc(j0) || b.po(j0).M != 1 || b.splits(i, j0)) continue;
        std::vector<size_t> idx{j0};
        for (;;) {
            const size_t j = b.skip_reshapes(idx.back() + 1);
            if (!b.free_fc(j) || b.po(j).M != 1 || b.po(j).K != b.po(idx.back()).N || b.splits(i, j)) break;
            idx.push_back(j);
        }
        std::vector<OpImpl *> run;
        for (size_t j : idx) run.push_back(ops[j]);
        for (size_t len = run.size(); len >= 1; --len) {
            const size_t smi = b.skip_reshapes(idx[len - 1] + 1);
            OpImpl *sm = b.free_sm(smi) && !b.splits(i, smi) ? ops[smi] : nullptr;
            if (sm && !fused_pool_fc_fits(ops[i], run.data(), (int)len, sm)) sm = nullptr; // (the layers without their Softmax)
            if (FusedImpl *f = fused_pool_fc_create(ops[i], run.data(), (int)len, sm)) {
                b.add_stage(f, i, sm ? smi : idx[len - 1]);
                break;
            }
        }
    }
}

// (6), one run: operators idx[] (run[] beside them) and the Softmax behind them (sm at smi, or nullptr), cut greedily into the
// longest chains whose weights fit the LDS budget
static void cut_fc_run(GroupBuilder &b, const std::vector<size_t> &idx, const std::vector<OpImpl *> &run, OpImpl *sm, size_t smi) {
    size_t pos = 0;
    while (pos < run.size()) {
        int best = 0;
        bool best_sm = false;
        for (size_t len = 2; pos + len <= run.size(); ++len) {
            const bool end = pos + len == run.size();
            if (fused_fc_chain_fits(run.data() + pos, (int)len, end ? sm : nullptr)) {
                best = (int)len, best_sm = end && sm;
            } else {
                if (end && sm && fused_fc_chain_fits(run.data() + pos, (int)len, nullptr)) best = (int)len, best_sm = false;
                break;
            }
        }
        if (best >= 2) {
            if (FusedImpl *f = fused_fc_chain_create(run.data() + pos, best, best_sm ? sm : nullptr))
                b.add_stage(f, idx[pos], best_sm ? smi : idx[pos + (size_t)best - 1]);
            pos += (size_t)best;
        } else {
            ++pos;
        }
    }
}

// (6) runs of consecutive FullyConnected operators (Reshapes between them keeping the [M][N] rows; + a Softmax over one row at
// the end) that no group above took -> fc_chain launches (k_fc_rt.hip), cut greedily into the longest chains whose weights fit
// the LDS budget; a layer that fits no chain keeps its own launch
static void rule_6_fc_chains(GroupBuilder &b) {
    for (size_t i = 0; i < b.n; ++i) {
        if (!b.free_fc(i)) continue;
        std::vector<size_t> idx{i};
        for (;;) {
            const size_t j = b.skip_reshapes(idx.back() + 1);
            if (!b.free_fc(j) || b.po(j).M != b.po(idx.back()).M || b.po(j).K != b.po(idx.back()).N || b.splits(i, j)) break;
            idx.push_back(j);
        }
        const size_t smi = b.skip_reshapes(idx.back() + 1);
        OpImpl *sm = b.free_sm(smi) && !b.splits(i, smi) ? b.g.ops[smi] : nullptr;
        std::vector<OpImpl *> run;
        for (size_t j : idx) run.push_back(b.g.ops[j]);
        cut_fc_run(b, idx, run, sm, smi);
        i = idx.back();
    }
}

// (6a) a Conv2D directly followed by an AveragePool2D or a MaxPool2D with more than one output pixel -> one conv_pool_rt /
// conv_maxpool_rt launch (fused_heads.hip:
// fused_conv_pool_create).  Behind every peephole above: a global pool stays with the tail and pool_fc_chain groups, the Conv2D of a
// depthwise pair with its pair.  A first operator that takes the f32 input inside its own launch keeps that launch (the entry is
// predict's quantisation inside a launch; the group has no f32 entry)
static void rule_6a_conv_pool(GroupBuilder &b) {
    for (size_t i = 0; i + 1 < b.n; ++i) {
        const int pk = b.kind(i + 1); // (an AveragePool2D: conv_pool_rt; a MaxPool2D: conv_maxpool_rt)
        if (b.kind(i) != MF_OP_CONV_2D || (pk != MF_OP_AVERAGE_POOL_2D && pk != MF_OP_MAX_POOL_2D) || !b.free_op(i) || !b.free_op(i + 1)) continue;
        if (b.po(i + 1).OH * b.po(i + 1).OW < 2 || b.splits(i, i + 1)) continue;
        if ((int)i == b.g.first_real && op_accepts_f32(b.g.ops[i])) continue;
        if (FusedImpl *f = fused_conv_pool_create(b.g.ops[i], b.g.ops[i + 1])) {
            b.add_stage(f, i, i + 1);
            ++i;
        }
    }
}

// (6b) a side operator -- one Conv2D on a skip edge -- and the join that reads its output -> one launch at the join: shortcut_add_rt
// with an ADD (fused_heads.hip: fused_shortcut_add_create), side_concat_rt with a CONCATENATION (fused_side_concat_create: a fire
// module's 1x1 expand and its join), wherever the two stand in file order.  No other rule matches a side operator (splits), so the pair
// is free; outside the kernel's class the side operator runs its own launch at the join, then the join
static void rule_6b_side_join(GroupBuilder &b) {
    for (size_t i = 0; i < b.n; ++i) {
        const int s = side_join_candidate(b.pm, i); // (what the file says; the builder asks the prepared operators again)
        if (s < 0) continue;
        const bool conv_first = b.po(i).run_input == 1; // (run_input 1: input a is the side operator's)
        b.g.side_join[i] = (b.kind(i) == MF_OP_ADD ? fused_shortcut_add_create : fused_side_concat_create)(b.g.ops[(size_t)s], b.g.ops[i], conv_first);
    }
}

// (7) the boundary conversions of M::predict inside the launches at the two ends of the whole model: every launch that can
// start a run at operator 0 learns the input's scale and zero point, every one that can end at the last operator the ones
// that operator stamped (the stem was told above; a kernel without such an instance says no and keeps the separate pass)
static void rule_7_boundaries(GroupBuilder &b) {
    const ParsedModel &pm = b.pm;
    const ModelGroups &g = b.g;
    const size_t first_real = (size_t)g.first_real;
    const bool entry = !pm.input_skip; // (a join that reads the quantised model input needs it in memory: no f32 entry)
    if (entry && first_real < b.n && g.fused[first_real]) (void)fused_set_input_quant(g.fused[first_real], pm.in_scale, pm.in_zp, pm.u8);
    if (entry && first_real > 0 && first_real < b.n) (void)op_set_input_quant(g.ops[first_real], pm.in_scale, pm.in_zp, pm.u8);
    if (g.last_real >= 0) (void)op_set_output_dequant(g.ops[(size_t)g.last_real], pm.out_scale, pm.out_zp, pm.u8);
    for (size_t i = 0; i < b.n; ++i)
        if (g.fused[i] && g.fused_last[i] == g.last_real) (void)fused_set_output_dequant(g.fused[i], pm.out_scale, pm.out_zp, pm.u8);
    for (const ModelGroups::Stage &st : g.stages) {
        if (entry && st.first == g.first_real) (void)fused_set_input_quant(st.f, pm.in_scale, pm.in_zp, pm.u8);
        if (st.last == g.last_real) (void)fused_set_output_dequant(st.f, pm.out_scale, pm.out_zp, pm.u8);
    }
}

ModelGroups build_groups(const ParsedModel &pm, int device, bool autotune) {
    GroupBuilder b{pm, device, autotune};
    // The order is part of what the rules mean; each later rule sees what the earlier ones took (covered / owned / fused[]):
    //   - operators first: every group borrows their device buffers; (0) tells the stem the input's quantisation before any group
    //     is built over it (fused_stages.hip: the quad + stem's f32 entry reads it)
    //   - (0p), the PAD + convolution group, with (1)-(3) and ahead of them at every index: where it is formed, the convolution is its
    //     member and no pair (1) is formed from a depthwise there and the 1x1 behind it; where it is not (no planner accepts,
    //     MF_NO_PAD_CONV), the convolution is a VALID operator on the padded tensor like any other and (1) may take it
    //   - (1)-(3) before every second-level rule: stages are built from first-level groups
    //   - (4) before (4b), (4b), (4b') before (4c): a pair a stage, a quad or the pair + tail took is no chain candidate; (4c) may
    //     also take a pair's group away
    //   - (4d) behind (4c): a pair a chain of pairs took is no expand-block candidate
    //   - (5) before (5a): speech.tflite's own geometry keeps (5); (5a), (5b) before (6): a FullyConnected run behind a one-channel
    //     convolution or a global pool is offered there first, (6) takes what they left
    //   - (6a) behind every rule above: a global pool stays with the tail and pool_fc_chain groups, a pair's Conv2D with its pair
    //   - (6b) anywhere behind the operators: it looks at side operators and their joins, which no other rule touches
    //   - (7) last: it tells every launch that exists by then, at either end of the model, the boundary's quantisation
    create_operators(b);
    rule_1_2_3_first_level(b);
    rule_4_stage_runs(b);
    rule_4b_quads(b);
    rule_4b1_pair_tail(b);
    rule_4c_chains(b);
    rule_4d_expand_blocks(b);
    rule_5_dwfc(b);
    rule_5a_conv1_fc(b);
    rule_5b_pool_fc(b);
    rule_6_fc_chains(b);
    rule_6a_conv_pool(b);
    rule_6b_side_join(b);
    rule_7_boundaries(b);
    return std::move(b.g);
}

} // namespace mf
