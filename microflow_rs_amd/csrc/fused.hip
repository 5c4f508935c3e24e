// fused.hip -- fused groups: consecutive prepared operators (ops.hip) as one launch.  A group borrows its operators' device
// arrays and builds the operand images its kernel needs beyond them from the operators' host copies (ops_impl.hpp).  This unit is
// what every kind shares after creation: destroy / name / mode, the f32 edge setters and THE launch path.  The builders are in
// fused_pairs.hip, fused_heads.hip and fused_stages.hip, the chain planner in chain_partition.hip, the group itself in fused_impl.hpp.
// Host code only; the kernels are in k_*.hip.
#include "fused_impl.hpp"

namespace mf {

void fused_destroy(FusedImpl *f) { delete f; }
const char *fused_kernel_name(const FusedImpl *f) { return f->name.c_str(); }
int fused_epilogue_mode(const FusedImpl *f) {
    if (f->epi_mode >= 0) return f->epi_mode;
    int mode = -1; // not recorded by the builder: the minimum over the group's conv-like operators
    for (const OpImpl *o : {f->a, f->b, f->c})
        if (o && (o->s.kind == MF_OP_CONV_2D || o->s.kind == MF_OP_DEPTHWISE_CONV_2D)) mode = mode < 0 ? o->magic_mode : std::min(mode, o->magic_mode);
    return mode;
}
bool fused_input_ok(const FusedImpl *f, const int8_t *d_in) { return !kind_facts(f->kind).in16 || ((uintptr_t)d_in & 15) == 0; }
bool fused_batch_ok(const FusedImpl *f, size_t batch) {
    if (f->kind == FusedImpl::BLOCK) return f->block_max_batch == 0 || batch <= f->block_max_batch;
    return f->kind != FusedImpl::CONV1FC || f->conv1fc.max_batch == 0 || batch <= f->conv1fc.max_batch;
}
// the f32 entry of a group that starts with the network's first operator (M::predict: the boundary quantisation inside the launch)
bool fused_set_input_quant(FusedImpl *f, float scale, int zp, bool u8) {
    if (!f || !kind_facts(f->kind).f32_in || !(scale == scale) || switches().no_f32_boundary) return false;
    edge_set_in(f->edge, f->a->device, scale, zp, u8);
    return f->edge_in = true;
}
bool fused_set_output_dequant(FusedImpl *f, float scale, int zp, bool u8) {
    if (!f || switches().no_f32_boundary || !kind_facts(f->kind).f32_out) return false;
    edge_set_out(f->edge, scale, zp, u8);
    return f->edge_out = true;
}
bool fused_accepts_f32(const FusedImpl *f) {
    if (f && f->edge_in) return true;
    return f && f->kind == FusedImpl::QUAD && f->quad.args.stem && f->quad.args.f32_ok && !switches().no_f32_group;
}
bool fused_emits_f32(const FusedImpl *f) { return f && f->edge_out; }

// The launch of every kind.  edge: which ends of the launch are f32 (k::EDGE_IN | k::EDGE_OUT; 0: d_in and d_out hold the element
// type), checked against the group by fused_run_f32.  No `default`: -Wall names a kind that is missing.
static void launch(FusedImpl *f, const void *in, size_t batch, void *out, int edge, hipStream_t st) {
    const int8_t *d_in = (const int8_t *)in;
    int8_t *d_out = (int8_t *)out;
    const size_t limit = batch_limit(*f, edge);
    if (limit && batch > limit) fail(MF_ERR_INVALID_ARG, "batch too large for one launch");
    if (!fused_input_ok(f, d_in)) fail(MF_ERR_INVALID_ARG, std::string(kind_facts(f->kind).in16) + ": the input pointer is not 16-byte aligned");
    switch (f->kind) {
    case FusedImpl::STAGE: {
        const OpSpec &d = f->a->s;
        if (!k::launch_stage(d.H, d.W, d.C, f->stage.pairs, d_in, d_out, f->stage.args, (int)batch, st)) fail(MF_ERR_UNSUPPORTED, "stage kernel missing");
        break;
    }
    case FusedImpl::CHAIN: k::launch_chain(d_in, d_out, f->chain.args, (int)batch, st); break;
    case FusedImpl::PAIRBAND:
        if (f->pairband.KSC == 8) k::launch_pair_band_deep(d_in, d_out, f->pairband, (int)batch, st);
        else k::launch_pair_band(d_in, d_out, f->pairband, (int)batch, st);
        break;
    case FusedImpl::BLOCK: k::launch_block_band(d_in, d_out, f->block, (int)batch, st); break;
    case FusedImpl::CONVPOOL:
        if (f->convpool.mx) k::launch_conv_maxpool(d_in, d_out, f->convpool.args, f->convpool.wz, (int)batch, st);
        else k::launch_conv_pool(d_in, d_out, f->convpool.args, f->convpool.wz, (int)batch, st);
        break;
    case FusedImpl::PAIRWZ: k::launch_pair_wz(d_in, d_out, f->pairwz, (int)batch, st); break;
    case FusedImpl::QUAD: {
        const int *q = f->quad.shape;
        if (edge) { // (the stem's f32 entry: fused_accepts_f32)
            if (!k::launch_quad_f32(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], (const float *)in, d_out, f->quad.args, (int)batch, st))
                fail(MF_ERR_UNSUPPORTED, "f32 quad kernel missing");
        } else if (f->quad.mm) {
            k::launch_quad_mm(d_in, d_out, f->quad.args, (int)batch, st);
        } else if (!k::launch_quad(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], d_in, d_out, f->quad.args, (int)batch, st)) {
            fail(MF_ERR_UNSUPPORTED, "quad kernel missing");
        }
        break;
    }
    case FusedImpl::TAIL: k::launch_tail(d_in, d_out, f->tail, batch, st); break;
    case FusedImpl::PAIRTAIL: { // (exit only: fused_set_input_quant refuses this kind)
        const k::F32Edge *eg = edge ? &f->edge : nullptr;
        if (f->pairtail.has_front) k::launch_pair_front_tail(d_in, d_out, f->pairtail.args, f->pairtail.front, batch, st, eg);
        else k::launch_pair_tail(d_in, d_out, f->pairtail.args, batch, st, eg);
        break;
    }
    case FusedImpl::DWFC:
        if (edge) k::launch_dwfc_f32(in, out, f->dwfc, f->edge, edge, batch, st);
        else k::launch_dwfc(d_in, d_out, f->dwfc, batch, st);
        break;
    case FusedImpl::FCCHAIN:
        if (edge) k::launch_fc_chain_f32(in, out, f->fcchain.args, f->edge, edge, (long long)(batch * f->fcchain.M), st);
        else k::launch_fc_chain(d_in, d_out, f->fcchain.args, (long long)(batch * f->fcchain.M), st);
        break;
    case FusedImpl::POOLFC: // (any output pointer: the kernel aligns its stores itself)
        if (edge) k::launch_pool_fc_f32(d_in, (float *)out, f->poolfc, f->edge, (long long)batch, st);
        else k::launch_pool_fc(d_in, d_out, f->poolfc, (long long)batch, st);
        break;
    case FusedImpl::CONV1FC: k::launch_conv1_fc(d_in, d_out, f->conv1fc.args, (long long)batch, st); break; // (any output pointer, as POOLFC)
    case FusedImpl::FCSM:
        if (!k::launch_fc_rowwave_softmax(d_in, d_out, f->a->fc, f->b->sm, batch, st)) fail(MF_ERR_UNSUPPORTED, "fused kernel missing");
        break;
    case FusedImpl::PADCONV: // (the inner operator's generic kernel knows no explicit pads: never an unaligned pointer)
        if ((uintptr_t)d_out & 15) fail(MF_ERR_INVALID_ARG, "pad+conv: the output pointer is not 16-byte aligned");
        op_run(f->padconv.get(), d_in, batch, d_out, st);
        break;
    case FusedImpl::SHORTCUT: fail(MF_ERR_INVALID_ARG, "shortcut_add_rt takes two inputs: fused_run2"); break;
    case FusedImpl::SIDECONCAT: fail(MF_ERR_INVALID_ARG, "side_concat_rt takes two inputs: fused_run2"); break;
    case FusedImpl::DWPW: {
        const OpSpec &d = f->a->s;
        if (!k::launch_dwpw(d.H, d.W, d.C, d.sh, f->b->s.N, d_in, d_out, f->dwpw, (int)batch, st)) fail(MF_ERR_UNSUPPORTED, "fused kernel missing");
        break;
    }
    }
    MF_HIP(hipGetLastError());
}
void fused_run(FusedImpl *f, const int8_t *d_in, size_t batch, int8_t *d_out, void *stream) {
    if (batch) launch(f, d_in, batch, d_out, 0, (hipStream_t)stream);
}
// The two-input groups.  Pixels of T are read while others are written, so the output never overlaps T.  shortcut_add_rt: the output
// may be exactly the running tensor (a lane reads its bytes before it writes them), any other overlap is refused; side_concat_rt: the
// output overlaps neither input (the pitches differ).  16-byte loads and stores at all three pointers (the runtime's buffers are aligned)
void fused_run2(FusedImpl *f, const int8_t *d_t, const int8_t *d_run, size_t batch, int8_t *d_out, void *stream) {
    const bool cat = f->kind == FusedImpl::SIDECONCAT;
    if (!cat && f->kind != FusedImpl::SHORTCUT) fail(MF_ERR_INVALID_ARG, "fused_run2: not a two-input group");
    if (!batch) return;
    const std::string name = cat ? "side_concat_rt" : "shortcut_add_rt";
    const k::SideConvArgs &c = cat ? f->sideconcat.conv : f->shortcut.conv;
    const size_t tb = batch * f->a->in_elems, ob = batch * (cat ? f->b->out_elems : f->b->s.add_elems);
    const size_t rb = cat ? batch * (size_t)c.OH * c.OW * (size_t)f->sideconcat.CR : ob;
    const uintptr_t t0 = (uintptr_t)d_t, o0 = (uintptr_t)d_out, r0 = (uintptr_t)d_run;
    if (!d_t || !d_run || !d_out) fail(MF_ERR_INVALID_ARG, name + ": null device pointer");
    if ((t0 < o0 + ob && o0 < t0 + tb) || ((cat || d_out != d_run) && r0 < o0 + ob && o0 < r0 + rb)) fail(MF_ERR_INVALID_ARG, name + ": the output overlaps an input");
    if ((t0 | o0 | r0) & 15) fail(MF_ERR_INVALID_ARG, name + ": a pointer is not 16-byte aligned");
    if (cat) k::launch_side_concat(d_t, d_run, d_out, f->sideconcat, (long long)batch, (hipStream_t)stream);
    else k::launch_shortcut_add(d_t, d_run, d_out, f->shortcut, (long long)batch, (hipStream_t)stream);
    MF_HIP(hipGetLastError());
}
void fused_run_f32(FusedImpl *f, const void *d_in, bool in_f32, size_t batch, void *d_out, bool out_f32, void *stream) {
    if (!batch) return;
    if (in_f32 && !fused_accepts_f32(f)) fail(MF_ERR_UNSUPPORTED, "group has no f32-input kernel");
    if (out_f32 && !fused_emits_f32(f)) fail(MF_ERR_UNSUPPORTED, "group has no f32-output kernel");
    if ((in_f32 || out_f32) && (!d_in || !d_out || (in_f32 && ((uintptr_t)d_in & 15)) || (out_f32 && ((uintptr_t)d_out & 3))))
        fail(MF_ERR_INVALID_ARG, "fused_run_f32: null or unaligned device pointer");
    launch(f, d_in, batch, d_out, (in_f32 ? k::EDGE_IN : 0) | (out_f32 ? k::EDGE_OUT : 0), (hipStream_t)stream);
}

} // namespace mf
