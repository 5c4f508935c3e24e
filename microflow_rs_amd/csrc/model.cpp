// model.cpp -- the runtime half of what #[model("x.tflite")] generates
// (microflow-macros/src/lib.rs:185-203): predict / predict_quantized /
// predict_inner over a BATCH of independent inferences.
//
// Device memory plan (sized for 288 GB of HBM, no reuse tricks needed):
//   weights + folded constants : resident per op (person_detect: ~0.3 MB)
//   act[0], act[1]             : ping-pong activation buffers, batch x max tensor bytes
//   in_q / io_f32              : staging for host-fed batches
// Every op reads one buffer and writes the other; Reshape is an alias (the 2D<->4D
// maps of src/tensor.rs:103-141 are the identity in NHWC memory).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <memory>
#include <vector>

#include "mf_internal.hpp"

namespace mf {

#define MF_HIP(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            fail(e_ == hipErrorOutOfMemory ? MF_ERR_OOM : MF_ERR_HIP,                         \
                 std::string(#call) + ": " + hipGetErrorString(e_));                          \
    } while (0)

struct ModelImpl {
    ParsedModel pm;
    int device = -1;
    bool prepared = false;
    bool generic = false;
    hipStream_t stream = nullptr;
    std::vector<OpImpl *> ops; // nullptr for Reshape
    // fused[i] != nullptr: ops i .. fused_last[i] run as ONE kernel (depthwise + 1x1 conv pairs;
    // the pool -> head conv -> [reshape] -> softmax tail)
    std::vector<FusedImpl *> fused;
    std::vector<int> fused_last;
    // second level: ops first .. last (several first-level groups / operators) as ONE kernel: a run of identical pair
    // groups (k_stage.hip), a one-input-channel depthwise + FullyConnected + Softmax (k_dwfc.hip), the last pair + the
    // tail (k_tail3.hip).  They do not overlap; what is inside stays available for mf_model_run_until.
    struct Stage {
        FusedImpl *f;
        int first, last;
    };
    std::vector<Stage> stages;
    bool fusion = true;
    bool autotune = false; // model_set_autotune: time the run-time-geometry chain candidates at creation
    size_t cap_batch = 0;
    int8_t *act[2] = {nullptr, nullptr};
    int8_t *in_q = nullptr;   // quantized input staging (host-fed or f32 path)
    float *io_f32 = nullptr;  // f32 input / output staging
    size_t io_f32_elems = 0;
    float *o_f32 = nullptr;   // f32 output staging of a host-fed batch whose last launch dequantises (its input slice is still being
                              // read): cap_batch x out_elems floats, allocated by the first such call

    // hipGraph replay of the device-resident path (mf_model_set_graph): the launch sequence of one
    // (input, output, batch) triple is captured the second time it is seen and replayed afterwards,
    // so a small-batch predict costs one graph launch instead of one launch per operator.
    struct GraphKey {
        const void *in = nullptr, *out = nullptr;
        size_t batch = 0;
        int last_op = 0;
        bool in_f32 = false, out_f32 = false;
        uint64_t epoch = 0;
        bool operator==(const GraphKey &o) const {
            return in == o.in && out == o.out && batch == o.batch && last_op == o.last_op &&
                   in_f32 == o.in_f32 && out_f32 == o.out_f32 && epoch == o.epoch;
        }
    };
    bool use_graph = false;
    uint64_t epoch = 0; // bumped whenever buffers or kernel routing change
    hipStream_t cap_stream = nullptr;
    hipStream_t copy_stream = nullptr; // H2D of host-fed batches, overlapped with compute
    hipGraphExec_t gexec = nullptr;
    GraphKey gkey, gcand;
    bool gvalid = false, gcand_valid = false;
    uint64_t graph_launches = 0;
    uint64_t device_ops = 0; // kernel launches and device-side copies enqueued so far (mf_model_device_ops)

    // sliding windows (model_run_windows): its own buffers, which no captured graph refers to
    size_t win_chunk = 0;     // windows per step (0: window_chunk_default)
    int8_t *win_q = nullptr;  // the gathered chunk: win_chunk x in_elems bytes, 16-byte aligned (what fused_input_ok asks)
    void *win_src = nullptr;  // a host-fed source, as it is
    void *win_out = nullptr;  // the results of a host-fed call, chunk after chunk, until they have crossed back
    size_t win_q_cap = 0, win_src_cap = 0, win_out_cap = 0; // bytes
    int win_fast = -1;        // quant_div's fast form verified for the model's input (scale, zero point, type): -1 not asked yet

    ~ModelImpl() {
        if (device >= 0) (void)hipSetDevice(device);
        drop_graph();
        if (win_q) (void)hipFree(win_q);
        if (win_src) (void)hipFree(win_src);
        if (win_out) (void)hipFree(win_out);
        if (cap_stream) (void)hipStreamDestroy(cap_stream);
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
        for (const Stage &st : stages) fused_destroy(st.f); // they borrow the groups' buffers: first
        for (FusedImpl *f : fused) fused_destroy(f);
        for (OpImpl *o : ops) op_destroy(o);
        free_buffers();
    }
    void drop_graph() {
        if (gexec) (void)hipGraphExecDestroy(gexec);
        gexec = nullptr;
        gvalid = gcand_valid = false;
        ++epoch;
    }
    void free_buffers() {
        for (auto &p : act) {
            if (p) (void)hipFree(p);
            p = nullptr;
        }
        if (in_q) (void)hipFree(in_q);
        if (io_f32) (void)hipFree(io_f32);
        if (o_f32) (void)hipFree(o_f32);
        in_q = nullptr;
        io_f32 = nullptr;
        o_f32 = nullptr;
        cap_batch = 0;
    }
};

ModelImpl *model_create(const uint8_t *buf, size_t len) {
    std::unique_ptr<ModelImpl> m(new ModelImpl);
    m->pm = parse_tflite(buf, len);
    return m.release();
}
void model_destroy(ModelImpl *m) { delete m; }
const ParsedModel &model_parsed(const ModelImpl *m) { return m->pm; }
static bool fused_at(const ModelImpl *m, int i) {
    return m->fusion && !m->generic && i >= 0 && i < (int)m->fused.size() && m->fused[(size_t)i];
}
// the second-level group that starts at op i and ends at or before last_op, if any
static const ModelImpl::Stage *stage_at(const ModelImpl *m, int i, int last_op) {
    if (!m->fusion || m->generic) return nullptr;
    for (const ModelImpl::Stage &st : m->stages)
        if (st.first == i && st.last <= last_op) return &st;
    return nullptr;
}
// index of the fused group that swallows op i (without being its first op), or -1
static int fused_owner(const ModelImpl *m, int i) {
    for (int j = i - 1; j >= 0 && j >= i - 4; --j)
        if (fused_at(m, j) && m->fused_last[(size_t)j] >= i) return j;
    return -1;
}
const char *model_op_kernel(const ModelImpl *m, int i) {
    if (!m->prepared || i < 0 || i >= (int)m->ops.size() || !m->ops[i]) return "";
    if (m->fusion && !m->generic) { // the stage a run from operator 0 uses for op i: the covering one that starts first
        const ModelImpl::Stage *best = nullptr;
        for (const ModelImpl::Stage &st : m->stages)
            if (i >= st.first && i <= st.last && (!best || st.first < best->first)) best = &st;
        if (best) return best->first == i ? fused_kernel_name(best->f) : "(fused into the previous operator)";
    }
    if (fused_at(m, i)) return fused_kernel_name(m->fused[(size_t)i]);
    if (fused_owner(m, i) >= 0) return "(fused into the previous operator)";
    return op_kernel_name(m->ops[i]);
}

int model_op_epilogue_mode(const ModelImpl *m, int i) {
    if (!m->prepared || i < 0 || i >= (int)m->ops.size() || !m->ops[i]) return -1;
    if (m->fusion && !m->generic) {
        const ModelImpl::Stage *best = nullptr;
        for (const ModelImpl::Stage &st : m->stages)
            if (i >= st.first && i <= st.last && (!best || st.first < best->first)) best = &st;
        if (best && best->first == i) return fused_epilogue_mode(best->f);
        if (!best && fused_at(m, i)) return fused_epilogue_mode(m->fused[(size_t)i]);
    }
    return op_epilogue_mode(m->ops[i]);
}

static void ensure_capacity(ModelImpl *m, size_t batch) {
    if (batch <= m->cap_batch) return;
    MF_HIP(hipSetDevice(m->device));
    MF_HIP(hipStreamSynchronize(m->stream));
    m->drop_graph();
    m->free_buffers();
    const ParsedModel &pm = m->pm;
    const size_t act_bytes = ((batch * pm.max_elems + 255) / 256) * 256 + 256;
    for (auto &p : m->act) MF_HIP(hipMalloc((void **)&p, act_bytes));
    MF_HIP(hipMalloc((void **)&m->in_q, ((batch * pm.in_elems + 255) / 256) * 256 + 256));
    m->io_f32_elems = batch * std::max(pm.in_elems, pm.out_elems);
    MF_HIP(hipMalloc((void **)&m->io_f32, m->io_f32_elems * sizeof(float) + 256));
    m->cap_batch = batch;
}

void model_prepare(ModelImpl *m, int device, size_t max_batch) {
    dev_require(device);
    if (m->prepared && m->device != device)
        fail(MF_ERR_INVALID_ARG, "model already prepared on another device");
    if (!m->prepared) {
        // Everything is built in locals and committed only when all of it exists: a failure half way
        // (a HIP error, OOM, a geometry the operator rejects) leaves the model unprepared and retryable,
        // on this or another device.
        struct Pending {
            std::vector<OpImpl *> ops;
            std::vector<FusedImpl *> fused;
            ~Pending() {
                for (FusedImpl *f : fused) fused_destroy(f);
                for (OpImpl *o : ops) op_destroy(o);
            }
        } pend;
        std::vector<OpImpl *> &ops = pend.ops;
        // predict_inner's running tensor: every op stamps its output scale / zero point on
        // it (Tensor::new(output, output_scale, output_zero_point)); Reshape keeps them.
        float cur_scale = m->pm.in_scale;
        int cur_zp = m->pm.in_zp;
        for (const ParsedOp &po : m->pm.ops) {
            if (po.kind == MF_OP_RESHAPE) {
                ops.push_back(nullptr);
                continue;
            }
            OpSpec s;
            s.kind = po.kind;
            s.u8 = m->pm.u8;
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
            ops.push_back(nullptr); // reserve the slot first: a throwing push_back must not leak the operator
            ops.back() = op_create(device, s);
            cur_scale = po.out_scale;
            cur_zp = po.out_zp;
        }
        // peephole (0): the boundary quantize of M::predict folds into operator 0 when that is the stem
        if (!ops.empty() && ops[0]) (void)op_set_input_quant(ops[0], m->pm.in_scale, m->pm.in_zp, m->pm.u8);
        // peepholes.  (1) DepthwiseConv2D 3x3 directly followed by a 1x1 Conv2D -> one fused kernel.
        // (2) AveragePool2D (1x1 output) -> Conv2D 1x1 -> [Reshape] -> Softmax -> one tail kernel.
        // (3) FullyConnected (few outputs, one row) -> [Reshape] -> Softmax -> one kernel.
        const size_t n = ops.size();
        std::vector<FusedImpl *> &fused = pend.fused;
        fused.assign(n, nullptr);
        std::vector<int> fused_last(n, -1);
        for (size_t i = 0; i + 1 < n; ++i) {
            if (m->pm.ops[i].kind == MF_OP_DEPTHWISE_CONV_2D && m->pm.ops[i + 1].kind == MF_OP_CONV_2D) {
                if ((fused[i] = fused_create(ops[i], ops[i + 1]))) fused_last[i] = (int)i + 1;
            } else if (m->pm.ops[i].kind == MF_OP_AVERAGE_POOL_2D && m->pm.ops[i + 1].kind == MF_OP_CONV_2D) {
                size_t j = i + 2;
                while (j < n && m->pm.ops[j].kind == MF_OP_RESHAPE) ++j;
                if (j < n && m->pm.ops[j].kind == MF_OP_SOFTMAX &&
                    (fused[i] = fused_tail_create(ops[i], ops[i + 1], ops[j])))
                    fused_last[i] = (int)j;
            } else if (m->pm.ops[i].kind == MF_OP_FULLY_CONNECTED) { // (3) FC -> [Reshape] -> Softmax
                size_t j = i + 1;
                while (j < n && m->pm.ops[j].kind == MF_OP_RESHAPE) ++j;
                if (j < n && m->pm.ops[j].kind == MF_OP_SOFTMAX &&
                    (fused[i] = fused_fc_softmax_create(ops[i], ops[j])))
                    fused_last[i] = (int)j;
            }
            if (fused[i]) i = (size_t)fused_last[i]; // groups do not overlap
        }
        // second level (the guard destroys what was built if anything below throws)
        struct StageGuard {
            std::vector<ModelImpl::Stage> v;
            ~StageGuard() {
                for (const ModelImpl::Stage &st : v) fused_destroy(st.f);
            }
        } sg;
        auto covered = [&](size_t i) {
            for (const ModelImpl::Stage &st : sg.v)
                if ((int)i >= st.first && (int)i <= st.last) return true;
            return false;
        };
        // (4) runs of consecutive pair groups on one tensor shape -> a persistent stage kernel, if one exists for that
        // shape and count (fused_stages.hip: fused_stage_create)
        for (size_t i = 0; i + 1 < n; ++i) {
            if (!fused[i] || fused_last[i] != (int)i + 1) continue;
            std::vector<FusedImpl *> run;
            size_t a = i;
            while (a + 1 < n && fused[a] && fused_last[a] == (int)a + 1 && m->pm.ops[a].H == m->pm.ops[i].H &&
                   m->pm.ops[a].W == m->pm.ops[i].W && m->pm.ops[a].C == m->pm.ops[i].C &&
                   m->pm.ops[a + 1].N == m->pm.ops[i].C && m->pm.ops[a].sh == 1) {
                run.push_back(fused[a]);
                a += 2;
            }
            // the longest prefix of the run a stage kernel accepts (differing zero points, a run longer than the kernel's
            // limit ...); what is left forms the next run
            size_t used = 0;
            for (size_t k = run.size(); k >= 2 && !used; --k)
                if (FusedImpl *f = fused_stage_create(run.data(), (int)k)) {
                    sg.v.push_back({f, (int)i, (int)(i + 2 * k) - 1});
                    used = k;
                }
            if (used) i += 2 * used - 1;             // continue with the pair after the stage
            else if (!run.empty()) i = a - 1;        // no stage for any prefix: continue after the run
        }
        // (4b) two consecutive pair groups whose shapes have a quad kernel (k_quad.hip: a VALU-bound stride-1 pair with the
        // HBM-bound stride-2 pair behind it; the tensor between them stays in LDS)
        for (size_t i = 0; i + 3 < n; ++i) {
            if (!fused[i] || fused_last[i] != (int)i + 1 || covered(i) || covered(i + 2)) continue;
            if (!fused[i + 2] || fused_last[i + 2] != (int)i + 3) continue;
            if (FusedImpl *f = fused_quad_create(fused[i], fused[i + 2])) {
                sg.v.push_back({f, (int)i, (int)i + 3});
                // ... and with the stem in front of it: ops i - 1 .. i + 3 in one launch.  Both stay: a run that does not
                // start at the stem (mf_model_run_until pieces, the f32 entry whose stem kernel quantises) uses the quad
                if (i >= 1 && ops[i - 1] && !fused[i - 1] && !covered(i - 1))
                    if (FusedImpl *g = fused_quad_stem_create(ops[i - 1], f)) sg.v.push_back({g, (int)i - 1, (int)i + 3});
                i += 3;
            }
        }
        // (4b') the last pair group directly followed by the tail group -> one kernel (fused_stages.hip: fused_pair_tail_create).  Before the
        // chain partition below, so that a run-time-geometry pair taken here is not also a candidate there
        for (size_t i = 0; i + 2 < n; ++i) {
            if (!fused[i] || fused_last[i] != (int)i + 1 || covered(i)) continue;
            const size_t j = i + 2;
            if (fused[j] && !covered(j))
                if (FusedImpl *f = fused_pair_tail_create(fused[i], fused[j])) {
                    sg.v.push_back({f, (int)i, fused_last[j]});
                    // ... and with the pair group in front of it: ops i - 2 .. the tail's end in one launch.  Both stay (a run that
                    // ends before the tail uses the pair groups, mf_model_run_until pieces that start at i the pair + tail stage)
                    if (i >= 2 && fused[i - 2] && fused_last[i - 2] == (int)i - 1 && !covered(i - 2))
                        if (FusedImpl *g = fused_front_pair_tail_create(fused[i - 2], f)) sg.v.push_back({g, (int)i - 2, fused_last[j]});
                }
        }
        // (4c) runs of consecutive run-time-geometry pairs (single-pair chain groups, k_chain.hip): the planner's cost model
        // decides how the run is cut into chain launches (chain_partition.hip: fused_chain_partition); a pair that is cheapest as two
        // separate launches loses its group
        bool chain_runs = false;
        for (size_t i = 0; i + 1 < n; ++i) {
            if (!fused_is_chain_single(fused[i]) || fused_last[i] != (int)i + 1 || covered(i)) continue;
            chain_runs = true;
            std::vector<FusedImpl *> run;
            size_t a = i;
            while (a + 1 < n && fused_is_chain_single(fused[a]) && fused_last[a] == (int)a + 1 && !covered(a)) {
                run.push_back(fused[a]);
                a += 2;
            }
            const int rn = (int)run.size();
            std::vector<int> seg((size_t)rn, 0);
            std::unique_ptr<bool[]> unf(new bool[(size_t)rn]);
            std::vector<int> segG((size_t)rn, 0);
            fused_chain_partition(run.data(), rn, seg.data(), unf.get(), segG.data(), m->autotune);
            for (int k = 0; k < rn; ++k) {
                const size_t at = i + 2 * (size_t)k;
                if (seg[(size_t)k] >= 2) {
                    if (FusedImpl *f = fused_chain_create(run.data() + k, seg[(size_t)k], segG[(size_t)k])) sg.v.push_back({f, (int)at, (int)(at + 2 * (size_t)seg[(size_t)k]) - 1});
                } else if (seg[(size_t)k] == 1 && unf[(size_t)k]) {
                    fused_destroy(fused[at]);
                    fused[at] = nullptr, fused_last[at] = -1;
                }
            }
            i = a - 1;
        }
        // (a forced chain plan that met no run was applied to nothing: the caller must not take the result for that plan's)
        if (!chain_runs && switches().dev && switches_parse().chain_plan_set)
            fail(MF_ERR_UNSUPPORTED, "MF_CHAIN_PLAN segment 0: the model has no run of run-time-geometry pairs");
        auto owned = [&](size_t i) {
            for (size_t j = 0; j < i; ++j)
                if (fused[j] && fused_last[j] >= (int)i) return true;
            return false;
        };
        // (4d) Conv2D 1x1 (expand) -> DepthwiseConv2D 3x3 -> Conv2D 1x1 (project) with the tensor inside the widest -> one block_band_rt
        // launch (fused_pairs.hip: fused_block_create).  Behind the chain partition, so that a pair a chain of pairs took is not a
        // candidate; a first-level pair group at i + 1 stays under the stage (mf_model_run_until pieces use it)
        for (size_t i = 0; i + 2 < n; ++i) {
            if (!ops[i] || m->pm.ops[i].kind != MF_OP_CONV_2D || fused[i] || covered(i) || owned(i)) continue;
            if (!ops[i + 1] || !ops[i + 2] || covered(i + 1) || covered(i + 2)) continue;
            if (FusedImpl *f = fused_block_create(ops[i], ops[i + 1], ops[i + 2], fused[i + 1] != nullptr)) {
                sg.v.push_back({f, (int)i, (int)i + 2});
                i += 2;
            }
        }
        // (5) DepthwiseConv2D with one input channel -> [Reshape] -> the FullyConnected + Softmax group -> one kernel
        for (size_t i = 0; i + 1 < n; ++i) {
            if (!ops[i] || fused[i] || covered(i) || m->pm.ops[i].kind != MF_OP_DEPTHWISE_CONV_2D) continue;
            size_t j = i + 1;
            while (j < n && m->pm.ops[j].kind == MF_OP_RESHAPE) ++j;
            if (j < n && fused[j] && !covered(j))
                if (FusedImpl *f = fused_dwfc_create(ops[i], fused[j])) sg.v.push_back({f, (int)i, fused_last[j]});
        }
        auto free_fc = [&](size_t i) {
            return i < n && ops[i] && m->pm.ops[i].kind == MF_OP_FULLY_CONNECTED && !fused[i] && !covered(i) && !owned(i);
        };
        auto free_sm = [&](size_t i) {
            return i < n && ops[i] && m->pm.ops[i].kind == MF_OP_SOFTMAX && !fused[i] && !covered(i) && !owned(i);
        };
        auto skip_reshapes = [&](size_t j) {
            while (j < n && m->pm.ops[j].kind == MF_OP_RESHAPE) ++j;
            return j;
        };
        // (5a) a DepthwiseConv2D or Conv2D with one input channel -> [Reshape] -> FullyConnected (one row per inference) -> [Reshape] ->
        // [Softmax] -> one conv1_fc_rt launch (fused_heads.hip: fused_conv1_fc_create) at any geometry its plan accepts; speech.tflite's own
        // geometry is refused there and keeps (5).  Where the FullyConnected + Softmax already are a group of (3), this stage sits over
        // conv .. softmax and that group stays for mf_model_run_until pieces.  One FullyConnected only: a run behind it is left to (6)
        for (size_t i = 0; i + 1 < n; ++i) {
            const int kind = m->pm.ops[i].kind;
            if (!ops[i] || fused[i] || covered(i) || owned(i) || (kind != MF_OP_DEPTHWISE_CONV_2D && kind != MF_OP_CONV_2D) || m->pm.ops[i].C != 1) continue;
            const size_t j0 = skip_reshapes(i + 1);
            if (j0 >= n || !ops[j0] || m->pm.ops[j0].kind != MF_OP_FULLY_CONNECTED || m->pm.ops[j0].M != 1 || covered(j0) || owned(j0)) continue;
            if (fused[j0]) {
                if (fused_last[j0] > (int)j0 && m->pm.ops[(size_t)fused_last[j0]].kind == MF_OP_SOFTMAX)
                    if (FusedImpl *f = fused_conv1_fc_create(ops[i], ops[j0], ops[(size_t)fused_last[j0]])) sg.v.push_back({f, (int)i, fused_last[j0]});
                continue;
            }
            const size_t smi = skip_reshapes(j0 + 1);
            OpImpl *sm = free_sm(smi) ? ops[smi] : nullptr;
            if (sm && !fused_conv1_fc_fits(ops[i], ops[j0], sm)) sm = nullptr; // (the two operators without the Softmax)
            if (FusedImpl *f = fused_conv1_fc_create(ops[i], ops[j0], sm)) sg.v.push_back({f, (int)i, (int)(sm ? smi : j0)});
        }
        // (5b) AveragePool2D over the whole image -> [Reshape] -> FullyConnected layers (one row per inference) -> [Softmax] -> one
        // pool_fc_chain launch (fused_heads.hip: fused_pool_fc_create), the longest run of layers whose images fit.  Before (6), so that the
        // FullyConnected run behind a pool is offered here first; what does not fit stays for (6) or keeps its own launches.  Where the
        // head's FullyConnected + Softmax already are a group of (3), this stage sits over pool .. softmax and that group stays for
        // mf_model_run_until pieces
        for (size_t i = 0; i + 1 < n; ++i) {
            if (!ops[i] || fused[i] || covered(i) || owned(i) || m->pm.ops[i].kind != MF_OP_AVERAGE_POOL_2D) continue;
            const size_t j0 = skip_reshapes(i + 1);
            if (j0 < n && fused[j0] && !covered(j0) && m->pm.ops[j0].kind == MF_OP_FULLY_CONNECTED && fused_last[j0] > (int)j0 &&
                m->pm.ops[(size_t)fused_last[j0]].kind == MF_OP_SOFTMAX) {
                OpImpl *fc = ops[j0];
                if (FusedImpl *f = fused_pool_fc_create(ops[i], &fc, 1, ops[(size_t)fused_last[j0]])) sg.v.push_back({f, (int)i, fused_last[j0]});
                continue;
            }
            if (!free_fc(j0) || m->pm.ops[j0].M != 1) continue;
            std::vector<size_t> idx{j0};
            for (;;) {
                const size_t j = skip_reshapes(idx.back() + 1);
                if (!free_fc(j) || m->pm.ops[j].M != 1 || m->pm.ops[j].K != m->pm.ops[idx.back()].N) break;
                idx.push_back(j);
            }
            std::vector<OpImpl *> run;
            for (size_t j : idx) run.push_back(ops[j]);
            for (size_t len = run.size(); len >= 1; --len) {
                const size_t smi = skip_reshapes(idx[len - 1] + 1);
                OpImpl *sm = free_sm(smi) ? ops[smi] : nullptr;
                if (sm && !fused_pool_fc_fits(ops[i], run.data(), (int)len, sm)) sm = nullptr; // (the layers without their Softmax)
                if (FusedImpl *f = fused_pool_fc_create(ops[i], run.data(), (int)len, sm)) {
                    sg.v.push_back({f, (int)i, (int)(sm ? smi : idx[len - 1])});
                    break;
                }
            }
        }
        // (6) runs of consecutive FullyConnected operators (Reshapes between them keeping the [M][N] rows; + a Softmax over one row at
        // the end) that no group above took -> fc_chain launches (k_fc_rt.hip), cut greedily into the longest chains whose weights fit
        // the LDS budget; a layer that fits no chain keeps its own launch
        for (size_t i = 0; i < n; ++i) {
            if (!free_fc(i)) continue;
            std::vector<size_t> idx{i};
            for (;;) {
                size_t j = idx.back() + 1;
                while (j < n && m->pm.ops[j].kind == MF_OP_RESHAPE) ++j;
                if (!free_fc(j) || m->pm.ops[j].M != m->pm.ops[idx.back()].M || m->pm.ops[j].K != m->pm.ops[idx.back()].N) break;
                idx.push_back(j);
            }
            size_t smi = idx.back() + 1;
            while (smi < n && m->pm.ops[smi].kind == MF_OP_RESHAPE) ++smi;
            OpImpl *sm = (smi < n && ops[smi] && m->pm.ops[smi].kind == MF_OP_SOFTMAX && !fused[smi] && !covered(smi) && !owned(smi)) ? ops[smi] : nullptr;
            std::vector<OpImpl *> run;
            for (size_t j : idx) run.push_back(ops[j]);
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
                        sg.v.push_back({f, (int)idx[pos], (int)(best_sm ? smi : idx[pos + (size_t)best - 1])});
                    pos += (size_t)best;
                } else {
                    ++pos;
                }
            }
            i = idx.back();
        }
        // (6a) a Conv2D directly followed by an AveragePool2D or a MaxPool2D with more than one output pixel -> one conv_pool_rt /
        // conv_maxpool_rt launch (fused_heads.hip:
        // fused_conv_pool_create).  Behind every peephole above: a global pool stays with the tail and pool_fc_chain groups, the Conv2D of a
        // depthwise pair with its pair.  A first operator that takes the f32 input inside its own launch keeps that launch (the entry is
        // predict's quantisation inside a launch; the group has no f32 entry)
        {
            size_t first_real = 0;
            while (first_real < n && !ops[first_real]) ++first_real;
            auto free_op = [&](size_t i) { return ops[i] && !fused[i] && !covered(i) && !owned(i); };
            for (size_t i = 0; i + 1 < n; ++i) {
                const int pk = m->pm.ops[i + 1].kind; // (an AveragePool2D: conv_pool_rt; a MaxPool2D: conv_maxpool_rt)
                if (m->pm.ops[i].kind != MF_OP_CONV_2D || (pk != MF_OP_AVERAGE_POOL_2D && pk != MF_OP_MAX_POOL_2D) || !free_op(i) || !free_op(i + 1)) continue;
                if (m->pm.ops[i + 1].OH * m->pm.ops[i + 1].OW < 2) continue;
                if (i == first_real && op_accepts_f32(ops[i])) continue;
                if (FusedImpl *f = fused_conv_pool_create(ops[i], ops[i + 1])) {
                    sg.v.push_back({f, (int)i, (int)i + 1});
                    ++i;
                }
            }
        }
        // (7) the boundary conversions of M::predict inside the launches at the two ends of the whole model: every launch that can
        // start a run at operator 0 learns the input's scale and zero point, every one that can end at the last operator the ones
        // that operator stamped (the stem was told above; a kernel without such an instance says no and keeps the separate pass)
        {
            int last_real = (int)n - 1;
            while (last_real >= 0 && !ops[(size_t)last_real]) --last_real;
            size_t first_real = 0;
            while (first_real < n && !ops[first_real]) ++first_real;
            if (first_real < n && fused[first_real]) (void)fused_set_input_quant(fused[first_real], m->pm.in_scale, m->pm.in_zp, m->pm.u8);
            if (first_real > 0 && first_real < n) (void)op_set_input_quant(ops[first_real], m->pm.in_scale, m->pm.in_zp, m->pm.u8);
            if (last_real >= 0) (void)op_set_output_dequant(ops[(size_t)last_real], m->pm.out_scale, m->pm.out_zp, m->pm.u8);
            for (size_t i = 0; i < n; ++i)
                if (fused[i] && fused_last[i] == last_real) (void)fused_set_output_dequant(fused[i], m->pm.out_scale, m->pm.out_zp, m->pm.u8);
            for (const ModelImpl::Stage &st : sg.v) {
                if (st.first == (int)first_real) (void)fused_set_input_quant(st.f, m->pm.in_scale, m->pm.in_zp, m->pm.u8);
                if (st.last == last_real) (void)fused_set_output_dequant(st.f, m->pm.out_scale, m->pm.out_zp, m->pm.u8);
            }
        }
        // commit (nothing below throws)
        m->stages.swap(sg.v);
        m->device = device;
        m->ops.swap(pend.ops);
        m->fused.swap(pend.fused);
        m->fused_last.swap(fused_last);
        m->prepared = true;
        model_set_generic(m, m->generic);
    }
    if (max_batch) ensure_capacity(m, max_batch);
}

void model_set_stream(ModelImpl *m, void *stream) { m->stream = (hipStream_t)stream; }

void model_sync(ModelImpl *m) {
    if (!m->prepared) return;
    MF_HIP(hipSetDevice(m->device));
    MF_HIP(hipStreamSynchronize(m->stream));
}

void model_set_autotune(ModelImpl *m, bool enabled) {
    if (m->prepared) fail(MF_ERR_INVALID_ARG, "mf_model_set_autotune: call it before mf_model_prepare");
    m->autotune = enabled;
}

void model_set_fusion(ModelImpl *m, bool enabled) {
    m->fusion = enabled;
    m->drop_graph();
}
void model_set_graph(ModelImpl *m, bool enabled) {
    m->use_graph = enabled;
    if (!enabled) m->drop_graph();
}
uint64_t model_graph_launches(const ModelImpl *m) { return m->graph_launches; }
uint64_t model_device_ops(const ModelImpl *m) { return m->device_ops; }

void model_set_generic(ModelImpl *m, bool generic) {
    m->generic = generic;
    m->drop_graph();
    for (OpImpl *o : m->ops)
        if (o) op_set_generic(o, generic);
}

// Which launch of a run of ops [0 .. last_op] takes the f32 input itself (the boundary quantize inside it)?  1: the second-level
// group that starts at the first operator (penta_rr, fc_chain, dwc1_fc_softmax), 2: the first-level group there, 3: that operator alone (the stem kernel, fc_rt: the
// groups behind it run as usual), 0: none
static int first_real_op(const ModelImpl *m) { // leading Reshapes alias the input (speech.tflite starts with one)
    int i = 0;
    while (i < (int)m->ops.size() && !m->ops[(size_t)i]) ++i;
    return i;
}
static int f32_entry(const ModelImpl *m, int last_op) {
    const int f = first_real_op(m);
    if (!m->fusion || m->generic || f > last_op || f >= (int)m->ops.size()) return 0;
    const ModelImpl::Stage *st0 = stage_at(m, f, last_op);
    if (st0 && fused_accepts_f32(st0->f)) return 1;
    if (!st0 && fused_at(m, f) && m->fused_last[(size_t)f] <= last_op && fused_accepts_f32(m->fused[(size_t)f])) return 2;
    if (!fused_at(m, f) && op_accepts_f32(m->ops[(size_t)f])) return 3;
    return 0;
}

// run ops [0..last_op]; `src_f32` != nullptr (only where f32_entry says so): the first launch consumes the f32 input directly.
// `final_dst` != nullptr: the launch that produces operator last_op's tensor writes it there instead of into an activation buffer
// (no copy of the result afterwards: 16 MB per step for the 4096^3 FullyConnected).  `final_f32` != nullptr: that launch stores the
// dequantised floats there if it has such an instance.  The return value says where the int8 result is; nullptr: it left as floats.
static const int8_t *run_ops(ModelImpl *m, const int8_t *src, size_t batch, int last_op, hipStream_t stream,
                             const float *src_f32 = nullptr, int8_t *final_dst = nullptr, float *final_f32 = nullptr) {
    const int8_t *cur = src;
    int which = 0;
    // the last operator that launches anything (trailing Reshapes alias its output)
    int last_real = last_op;
    while (last_real >= 0 && !m->ops[last_real]) --last_real;
    const int entry = src_f32 ? f32_entry(m, last_op) : 0;
    if (src_f32 && !entry) fail(MF_ERR_UNSUPPORTED, "no launch takes the f32 input");
    const int first_real = first_real_op(m);
    for (int i = 0; i <= last_op; ++i) {
        OpImpl *o = m->ops[i];
        if (!o) continue; // Reshape: alias
        const bool f32in = src_f32 && i == first_real;
        int8_t *dst = m->act[which];
        if (dst == cur) {
            which ^= 1;
            dst = m->act[which];
        }
        const ModelImpl::Stage *staged = stage_at(m, i, last_op);
        bool grouped;
        if (f32in) {
            if (entry != 1) staged = nullptr;
            grouped = entry == 2;
        } else {
            if (staged && (!fused_input_ok(staged->f, cur) || !fused_batch_ok(staged->f, batch))) staged = nullptr; // (the operators' own launches take any pointer and batch)
            grouped = !staged && fused_at(m, i) && m->fused_last[(size_t)i] <= last_op && fused_input_ok(m->fused[(size_t)i], cur);
        }
        const int end = staged ? staged->last : (grouped ? m->fused_last[(size_t)i] : i);
        const bool f32out = final_f32 && end >= last_real &&
                            (staged ? fused_emits_f32(staged->f) : grouped ? fused_emits_f32(m->fused[(size_t)i]) : op_emits_f32(o));
        if (final_dst && end >= last_real) dst = final_dst;
        if (f32in || f32out) { // a model boundary inside the launch
            const void *in = f32in ? (const void *)src_f32 : (const void *)cur;
            void *out = f32out ? (void *)final_f32 : (void *)dst;
            if (staged) fused_run_f32(staged->f, in, f32in, batch, out, f32out, stream);
            else if (grouped) fused_run_f32(m->fused[(size_t)i], in, f32in, batch, out, f32out, stream);
            else op_run_f32(o, in, f32in, batch, out, f32out, stream);
            if (f32out) return nullptr;
        } else if (staged) { // several groups in one launch
            fused_run(staged->f, cur, batch, dst, stream);
        } else if (grouped) { // the whole group in one launch
            fused_run(m->fused[(size_t)i], cur, batch, dst, stream);
        } else {
            op_run(o, cur, batch, dst, stream);
        }
        i = end;
        cur = dst;
        which ^= 1;
    }
    return cur;
}

// Which of M::predict's two boundary conversions run inside the first / last launch of this call: only with fusion on, the
// shape-specialised kernels, the whole model, a 16-byte aligned f32 input (float4 loads) and a 4-byte aligned f32 output; and the
// exit only where the output range does not overlap the input's, which the first launch -- possibly the same one -- is still reading.
// Otherwise that side keeps its separate pass, with the same bits.
// can any launch that ends the whole model store floats?
static bool f32_exit_any(const ModelImpl *m) {
    int last_real = (int)m->ops.size() - 1;
    while (last_real >= 0 && !m->ops[(size_t)last_real]) --last_real;
    if (last_real < 0) return false;
    if (op_emits_f32(m->ops[(size_t)last_real])) return true;
    for (size_t i = 0; i < m->fused.size(); ++i)
        if (m->fused[i] && m->fused_last[i] == last_real && fused_emits_f32(m->fused[i])) return true;
    for (const ModelImpl::Stage &st : m->stages)
        if (st.last == last_real && fused_emits_f32(st.f)) return true;
    return false;
}
struct Boundary {
    bool in = false, out = false;
};
static Boundary boundary_plan(const ModelImpl *m, const float *in_f32, const float *out_f32, size_t out_count, const void *in_any, size_t in_bytes,
                              int last_op) {
    Boundary b;
    if (!m->fusion || m->generic || last_op != (int)m->pm.ops.size() - 1) return b;
    b.in = in_f32 && ((uintptr_t)in_f32 & 15) == 0 && f32_entry(m, last_op) != 0;
    if (out_f32 && ((uintptr_t)out_f32 & 3) == 0) {
        const uintptr_t ob = (uintptr_t)out_f32, oe = ob + out_count * sizeof(float);
        const uintptr_t ib = (uintptr_t)in_any, ie = ib + in_bytes;
        b.out = !(ob < ie && ib < oe);
    }
    return b;
}

// The whole device-resident sequence (boundary conversion -> ops -> boundary conversion) on
// `s`: every pointer is a device pointer, nothing synchronizes -- so it can be stream-captured.
static void enqueue_device(ModelImpl *m, const float *in_f32, const int8_t *in_i8, size_t batch,
                           float *out_f32, int8_t *out_i8, int last_op, hipStream_t s) {
    const ParsedModel &pm = m->pm;
    const int nops = (int)pm.ops.size();
    const size_t out_elems = last_op == nops - 1 ? pm.out_elems : pm.ops[last_op].out_elems;
    const int8_t *q_in;
    const Boundary bd = boundary_plan(m, in_f32, out_f32, batch * out_elems, in_f32 ? (const void *)in_f32 : (const void *)in_i8,
                                      batch * pm.in_elems * (in_f32 ? sizeof(float) : 1), last_op);
    const bool fuse_q = bd.in;
    if (fuse_q) {
        q_in = nullptr; // the first launch quantises while it stages (dw3x3_stem8<.., F32IN>, fc_chain_f32 ...)
    } else if (in_f32) { // Tensor::quantize(input, scale, zero_point)  (lib.rs:189)
        dev_quantize(m->device, in_f32, batch * pm.in_elems, pm.in_scale, pm.in_zp, pm.u8, m->in_q, s);
        q_in = m->in_q;
    } else if (pm.u8) { // u8 -> internal i8 domain
        dev_xor80(m->device, in_i8, batch * pm.in_elems, m->in_q, s);
        q_in = m->in_q;
    } else if (((uintptr_t)in_i8 & 15) != 0) { // the fast kernels read 16-byte words: realign an odd caller pointer
        MF_HIP(hipMemcpyAsync(m->in_q, in_i8, batch * pm.in_elems, hipMemcpyDeviceToDevice, s));
        ++dev_launch_counter();
        q_in = m->in_q;
    } else {
        q_in = in_i8; // consumed in place
    }
    // An i8 model's result is written straight into the caller's buffer by the last launch -- unless that buffer overlaps
    // the caller's input, which the first launch may still be reading (in_i8 is consumed in place): a model that is ONE
    // launch would then read and write the same memory.  Overlapping buffers take the activation buffer + copy path.
    int8_t *direct = (out_i8 && !pm.u8 && ((uintptr_t)out_i8 & 15) == 0) ? out_i8 : nullptr; // (16-byte vector stores)
    if (direct) {
        const uintptr_t ob = (uintptr_t)out_i8, oe = ob + batch * out_elems;
        const uintptr_t ib = (uintptr_t)(in_f32 ? (const void *)in_f32 : (const void *)in_i8);
        const uintptr_t ie = ib + batch * pm.in_elems * (in_f32 ? sizeof(float) : 1);
        if (ob < ie && ib < oe) direct = nullptr;
    }
    const int8_t *res = run_ops(m, q_in, batch, last_op, s, fuse_q ? in_f32 : nullptr, direct, bd.out ? out_f32 : nullptr);
    if (out_i8) {
        if (pm.u8) dev_xor80(m->device, res, batch * out_elems, out_i8, s);
        else if (res != out_i8) {
            MF_HIP(hipMemcpyAsync(out_i8, res, batch * out_elems, hipMemcpyDeviceToDevice, s));
            ++dev_launch_counter();
        }
    } else if (res) { // .dequantize()  (lib.rs:190) with the parameters the last op stamped on the tensor
        float oscale = pm.out_scale;
        int ozp = pm.out_zp;
        if (last_op != nops - 1) oscale = pm.ops[last_op].out_scale, ozp = pm.ops[last_op].out_zp;
        dev_dequantize(m->device, res, batch * out_elems, oscale, ozp, pm.u8, out_f32, s);
    }
}

// device path with graph replay: eager the first time a key is seen, captured the second time
static void run_device(ModelImpl *m, const float *in_f32, const int8_t *in_i8, size_t batch,
                       float *out_f32, int8_t *out_i8, int last_op) {
    hipStream_t s = m->stream;
    // what this call enqueues, for mf_model_device_ops: the launches and device-to-device copies of an eager pass; one for a call that
    // launches the graph -- a replay, and also the call that captures it, which records its launches instead of enqueueing them and
    // then launches the new graph once
    struct Count {
        ModelImpl *m;
        unsigned long long before = dev_launch_counter();
        bool replay = false;
        ~Count() { m->device_ops += replay ? 1 : dev_launch_counter() - before; }
    } count{m};
    if (!m->use_graph) return enqueue_device(m, in_f32, in_i8, batch, out_f32, out_i8, last_op, s);
    ModelImpl::GraphKey k;
    k.in = in_f32 ? (const void *)in_f32 : (const void *)in_i8;
    k.out = out_f32 ? (const void *)out_f32 : (const void *)out_i8;
    k.batch = batch, k.last_op = last_op, k.in_f32 = in_f32 != nullptr, k.out_f32 = out_f32 != nullptr;
    k.epoch = m->epoch;
    if (m->gvalid && m->gkey == k) {
        count.replay = true;
        MF_HIP(hipGraphLaunch(m->gexec, s));
        ++m->graph_launches;
        return;
    }
    if (!(m->gcand_valid && m->gcand == k)) { // first sighting: run eagerly (lets operators size their scratch)
        m->gcand = k, m->gcand_valid = true;
        return enqueue_device(m, in_f32, in_i8, batch, out_f32, out_i8, last_op, s);
    }
    count.replay = true;
    if (!m->cap_stream) MF_HIP(hipStreamCreateWithFlags(&m->cap_stream, hipStreamNonBlocking));
    MF_HIP(hipStreamBeginCapture(m->cap_stream, hipStreamCaptureModeRelaxed));
    hipGraph_t g = nullptr;
    try {
        enqueue_device(m, in_f32, in_i8, batch, out_f32, out_i8, last_op, m->cap_stream);
    } catch (...) {
        (void)hipStreamEndCapture(m->cap_stream, &g);
        if (g) (void)hipGraphDestroy(g);
        throw;
    }
    MF_HIP(hipStreamEndCapture(m->cap_stream, &g));
    hipGraphExec_t e = nullptr;
    hipError_t err = hipGraphInstantiate(&e, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (err != hipSuccess) fail(MF_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(err));
    if (m->gexec) (void)hipGraphExecDestroy(m->gexec);
    m->gexec = e, m->gkey = k, m->gvalid = true, m->gcand_valid = false;
    MF_HIP(hipGraphLaunch(m->gexec, s));
    ++m->graph_launches;
}

void model_run(ModelImpl *m, const float *in_f32, const int8_t *in_i8, size_t batch, float *out_f32,
               int8_t *out_i8, int mem, int last_op) {
    if (!m->prepared) fail(MF_ERR_INVALID_ARG, "model not prepared: call mf_model_prepare first");
    if (!batch) return; // zero inferences: nothing to read or write (empty buffers may be null)
    if ((in_f32 == nullptr) == (in_i8 == nullptr) || (out_f32 == nullptr) == (out_i8 == nullptr))
        fail(MF_ERR_INVALID_ARG, "null buffer");
    if (mem != MF_MEM_HOST && mem != MF_MEM_DEVICE) fail(MF_ERR_INVALID_ARG, "bad mem kind");
    const ParsedModel &pm = m->pm;
    const int nops = (int)pm.ops.size();
    if (last_op < 0) last_op = nops - 1;
    if (last_op >= nops) fail(MF_ERR_INVALID_ARG, "op index out of range");
    if (!batch) return;
    MF_HIP(hipSetDevice(m->device));
    ensure_capacity(m, batch);
    const size_t out_elems = last_op == nops - 1 ? pm.out_elems : pm.ops[last_op].out_elems;
    const bool host = mem == MF_MEM_HOST;
    hipStream_t s = m->stream;
    if (!host) return run_device(m, in_f32, in_i8, batch, out_f32, out_i8, last_op);

    // ---- host buffers staged through HBM ----
    // The batch is cut into chunks of ~64 MB of input: chunk c+1 crosses PCIe on the copy stream
    // while chunk c computes (pinned host memory makes the copies truly asynchronous; pageable
    // memory still works, serialized by the runtime).  Each chunk has its own slice of the
    // staging buffers; the activation ping-pong buffers are reused chunk after chunk, in order.
    const size_t in_bytes = pm.in_elems * (in_f32 ? sizeof(float) : 1);
    const size_t out_bytes = out_elems * (out_f32 ? sizeof(float) : 1);
    size_t chunk = batch;
    if (in_bytes && out_bytes <= in_bytes) { // (a chunk's f32 output slice must not reach later chunks' input slices)
        const size_t per = std::max<size_t>(256, ((64u << 20) / in_bytes) & ~(size_t)255);
        if (batch > per + per / 2) chunk = per;
    }
    if (chunk < batch && !m->copy_stream) MF_HIP(hipStreamCreateWithFlags(&m->copy_stream, hipStreamNonBlocking));
    std::vector<hipEvent_t> evs;
    float oscale = pm.out_scale;
    int ozp = pm.out_zp;
    if (last_op != nops - 1) oscale = pm.ops[last_op].out_scale, ozp = pm.ops[last_op].out_zp;
    // (what this call enqueues on the device, for mf_model_device_ops: added on every way out)
    struct OpsAdded {
        ModelImpl *m;
        unsigned long long before = dev_launch_counter();
        ~OpsAdded() { m->device_ops += dev_launch_counter() - before; }
    } ops_added{m};
    if (out_f32 && !m->o_f32 && m->fusion && !m->generic && last_op == nops - 1 && f32_exit_any(m))
        MF_HIP(hipMalloc((void **)&m->o_f32, m->cap_batch * pm.out_elems * sizeof(float) + 256));
    try {
        if (chunk < batch) { // the copy stream starts after whatever the caller queued on the compute stream
            hipEvent_t e;
            MF_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            evs.push_back(e);
            MF_HIP(hipEventRecord(e, s));
            MF_HIP(hipStreamWaitEvent(m->copy_stream, e, 0));
        }
        for (size_t first = 0; first < batch; first += chunk) {
            const size_t n = std::min(chunk, batch - first);
            hipStream_t cs = chunk < batch ? m->copy_stream : s;
            int8_t *q = m->in_q + first * pm.in_elems;
            float *f = m->io_f32 + first * pm.in_elems;
            if (in_f32) MF_HIP(hipMemcpyAsync(f, in_f32 + first * pm.in_elems, n * in_bytes, hipMemcpyHostToDevice, cs));
            else MF_HIP(hipMemcpyAsync(q, in_i8 + first * pm.in_elems, n * in_bytes, hipMemcpyHostToDevice, cs));
            if (cs != s) {
                hipEvent_t e;
                MF_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                evs.push_back(e);
                MF_HIP(hipEventRecord(e, cs));
                MF_HIP(hipStreamWaitEvent(s, e, 0));
            }
            // (the f32 result of a last launch that dequantises goes to its own staging slice: the chunk's f32 input slice, which the
            // separate pass may overwrite, is still being read by that launch)
            float *fo = m->io_f32 + first * out_elems;
            float *fo_direct = m->o_f32 ? m->o_f32 + first * out_elems : nullptr;
            const Boundary bd = boundary_plan(m, in_f32 ? f : nullptr, out_f32 ? fo_direct : nullptr, n * out_elems,
                                              in_f32 ? (const void *)f : (const void *)q, n * in_bytes, last_op);
            const bool fuse_q = bd.in;
            if (in_f32 && !fuse_q) // Tensor::quantize(input, scale, zero_point)  (lib.rs:189)
                dev_quantize(m->device, f, n * pm.in_elems, pm.in_scale, pm.in_zp, pm.u8, q, s);
            else if (!in_f32 && pm.u8)
                dev_xor80(m->device, q, n * pm.in_elems, q, s); // u8 -> internal i8 domain
            const int8_t *res = run_ops(m, q, n, last_op, s, fuse_q ? f : nullptr, nullptr, bd.out ? fo_direct : nullptr); // predict_inner
            if (out_i8) {
                if (pm.u8) { // internal i8 domain -> u8, in place in the scratch buffer holding the result
                    int8_t *tmp = res == q ? m->act[0] : const_cast<int8_t *>(res);
                    dev_xor80(m->device, res, n * out_elems, tmp, s);
                    res = tmp;
                }
                MF_HIP(hipMemcpyAsync(out_i8 + first * out_elems, res, n * out_elems, hipMemcpyDeviceToHost, s));
            } else { // .dequantize()  (lib.rs:190) with the parameters the last op stamped on the tensor
                if (res) dev_dequantize(m->device, res, n * out_elems, oscale, ozp, pm.u8, fo, s);
                MF_HIP(hipMemcpyAsync(out_f32 + first * out_elems, res ? fo : fo_direct, n * out_bytes, hipMemcpyDeviceToHost, s));
            }
        }
        MF_HIP(hipStreamSynchronize(s));
    } catch (...) {
        if (m->copy_stream) (void)hipStreamSynchronize(m->copy_stream);
        (void)hipStreamSynchronize(s);
        for (hipEvent_t e : evs) (void)hipEventDestroy(e);
        throw;
    }
    for (hipEvent_t e : evs) (void)hipEventDestroy(e);
}

// ---- sliding windows (include/microflow_amd.h, section 5) ----
// Windows run chunk by chunk: the gather (k_windows.hip) writes a dense chunk into win_q -- quantising an f32 source, moving a u8
// source into the internal domain on the way, so neither boundary pass runs -- and run_ops takes it from there as it takes any
// resident batch; the f32 exit stays inside the last launch where the model has one.  Always eager: nothing here looks at or
// changes the graph kept for model_run's triples, and under set_graph the chunk never outgrows the activation buffers (growing
// them would drop that graph).
// The chunk: the sweep (profiles/r16/windows.txt) found every model faster the larger the chunk, up to the whole batch
// -- a chunk is a gather and a whole launch sequence, and the persistent step-queue kernels want tens of thousands of inputs
// -- and no step down where the staged bytes outgrow the 256 MiB Infinity Cache.  128 MiB (half that cache) is where the
// curves have flattened to within a few per cent of the whole batch, and what bounds the staging buffer.
constexpr size_t WINDOW_CHUNK_BYTES = 128u << 20;
static size_t window_chunk_default(const ParsedModel &pm) {
    const size_t per = (WINDOW_CHUNK_BYTES / std::max<size_t>(pm.in_elems, 1)) & ~(size_t)255;
    return std::max<size_t>(per, 256);
}
void model_set_window_chunk(ModelImpl *m, size_t windows) { m->win_chunk = windows; }
static void window_buffer(ModelImpl *m, void **p, size_t *cap, size_t bytes) {
    if (*cap >= bytes && *p) return;
    MF_HIP(hipStreamSynchronize(m->stream)); // an earlier call's launches may still read the old one
    if (*p) (void)hipFree(*p);
    *p = nullptr, *cap = 0;
    MF_HIP(hipMalloc(p, bytes + 256));
    *cap = bytes;
}

void model_run_windows(ModelImpl *m, const float *src_f32, const int8_t *src_i8, const mf_windows *w, size_t first, size_t count,
                       float *out_f32, int8_t *out_i8, int mem) {
    // ---- arguments: all of it before the device is looked at ----
    const ParsedModel &pm = m->pm;
    WindowsGeom g;
    const char *err = "";
    if (windows_check(w, pm.in_elems, &g, &err) != MF_OK) fail(MF_ERR_INVALID_ARG, err);
    if (windows_range_check(g, first, count, &err) != MF_OK) fail(MF_ERR_INVALID_ARG, err);
    if (mem != MF_MEM_HOST && mem != MF_MEM_DEVICE) fail(MF_ERR_INVALID_ARG, "bad mem kind");
    const size_t esz = src_f32 ? sizeof(float) : 1, osz = out_f32 ? sizeof(float) : 1;
    size_t lo = 0, span = 0;
    windows_span(*w, g, first, count, &lo, &span);
    if (count) {
        if ((src_f32 == nullptr) == (src_i8 == nullptr) || (out_f32 == nullptr) == (out_i8 == nullptr)) fail(MF_ERR_INVALID_ARG, "null buffer");
        if (((uintptr_t)src_f32 & 3) || ((uintptr_t)out_f32 & 3)) fail(MF_ERR_INVALID_ARG, "src / out: f32 buffers must be 4-byte aligned");
        const uintptr_t sb = (src_f32 ? (uintptr_t)src_f32 : (uintptr_t)src_i8) + lo * esz, se = sb + span * esz;
        const uintptr_t ob = out_f32 ? (uintptr_t)out_f32 : (uintptr_t)out_i8, oe = ob + count * pm.out_elems * osz;
        if (ob < se && sb < oe) fail(MF_ERR_INVALID_ARG, "src and out overlap");
    }
    if (!m->prepared) {
        if (dev_count() <= 0) fail(MF_ERR_NO_DEVICE, "no HIP device available: libmicroflow_amd has no CPU fallback");
        fail(MF_ERR_INVALID_ARG, "model not prepared: call mf_model_prepare first");
    }
    if (!count) return;

    MF_HIP(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    const bool host = mem == MF_MEM_HOST;
    const int last_op = (int)pm.ops.size() - 1;
    size_t chunk = std::min(count, m->win_chunk ? m->win_chunk : window_chunk_default(pm));
    if (m->use_graph && m->cap_batch) chunk = std::min(chunk, m->cap_batch);
    ensure_capacity(m, chunk);
    window_buffer(m, (void **)&m->win_q, &m->win_q_cap, chunk * pm.in_elems);
    if (src_f32 && m->win_fast < 0) m->win_fast = dev_quant_div_fast(m->device, pm.in_scale, pm.in_zp, pm.u8) ? 1 : 0;

    // the source as the gather sees it: a host source crosses once, whole sources from the first window's to the last window's
    const void *d_src = src_f32 ? (const void *)src_f32 : (const void *)src_i8;
    size_t d_first = first;
    if (host) {
        window_buffer(m, &m->win_src, &m->win_src_cap, span * esz);
        window_buffer(m, &m->win_out, &m->win_out_cap, count * pm.out_elems * osz);
        MF_HIP(hipMemcpyAsync(m->win_src, (const char *)d_src + lo * esz, span * esz, hipMemcpyHostToDevice, s));
        d_src = m->win_src;
        d_first = first - (first / g.per_source) * g.per_source;
    }
    const bool many = chunk < count;
    if (host && many && !m->copy_stream) MF_HIP(hipStreamCreateWithFlags(&m->copy_stream, hipStreamNonBlocking));
    std::vector<hipEvent_t> evs;
    struct OpsAdded {
        ModelImpl *m;
        unsigned long long before = dev_launch_counter();
        ~OpsAdded() { m->device_ops += dev_launch_counter() - before; }
    } ops_added{m};
    try {
        for (size_t done = 0; done < count; done += chunk) {
            const size_t n = std::min(chunk, count - done);
            if (src_f32)
                dev_window_gather_quantize(m->device, (const float *)d_src, *w, g, d_first + done, n, pm.in_scale, pm.in_zp, pm.u8,
                                           m->win_fast == 1, pm.u8, m->win_q, s);
            else
                dev_window_gather(m->device, d_src, *w, g, d_first + done, n, pm.u8, m->win_q, s);
            // where this chunk's results go on the device: the caller's buffer, or win_out on their way to the host
            const size_t off = done * pm.out_elems;
            float *t_f32 = out_f32 ? (host ? (float *)m->win_out : out_f32) + off : nullptr;
            int8_t *t_i8 = out_i8 ? (host ? (int8_t *)m->win_out : out_i8) + off : nullptr;
            const void *from; // (host) where the chunk's results lie when its launches are through
            if (t_f32) {
                const int8_t *res = run_ops(m, m->win_q, n, last_op, s, nullptr, nullptr, (m->fusion && !m->generic) ? t_f32 : nullptr);
                if (res) dev_dequantize(m->device, res, n * pm.out_elems, pm.out_scale, pm.out_zp, pm.u8, t_f32, s);
                from = t_f32;
            } else if (pm.u8) {
                const int8_t *res = run_ops(m, m->win_q, n, last_op, s);
                dev_xor80(m->device, res, n * pm.out_elems, t_i8, s);
                from = t_i8;
            } else {
                const int8_t *res = run_ops(m, m->win_q, n, last_op, s, nullptr, ((uintptr_t)t_i8 & 15) == 0 ? t_i8 : nullptr);
                from = res; // (an activation buffer where the slice is not aligned for the last launch's 16-byte stores)
                if (!host && res != t_i8) {
                    MF_HIP(hipMemcpyAsync(t_i8, res, n * pm.out_elems, hipMemcpyDeviceToDevice, s));
                    ++dev_launch_counter();
                }
            }
            if (!host) continue;
            char *h_out = (out_f32 ? (char *)out_f32 : (char *)out_i8) + off * osz;
            const bool in_win_out = from == (const void *)t_f32 || from == (const void *)t_i8;
            if (many && in_win_out) { // the slice is not written again: it crosses on the copy stream while the next chunk runs
                hipEvent_t e;
                MF_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                evs.push_back(e);
                MF_HIP(hipEventRecord(e, s));
                MF_HIP(hipStreamWaitEvent(m->copy_stream, e, 0));
                MF_HIP(hipMemcpyAsync(h_out, from, n * pm.out_elems * osz, hipMemcpyDeviceToHost, m->copy_stream));
            } else {
                MF_HIP(hipMemcpyAsync(h_out, from, n * pm.out_elems * osz, hipMemcpyDeviceToHost, s));
            }
        }
        if (host) {
            MF_HIP(hipStreamSynchronize(s));
            if (many) MF_HIP(hipStreamSynchronize(m->copy_stream));
        }
    } catch (...) {
        if (m->copy_stream) (void)hipStreamSynchronize(m->copy_stream);
        (void)hipStreamSynchronize(s);
        for (hipEvent_t e : evs) (void)hipEventDestroy(e);
        throw;
    }
    for (hipEvent_t e : evs) (void)hipEventDestroy(e);
}

void model_time_device(ModelImpl *m, const int8_t *d_in, size_t batch, int8_t *d_out, int warmup,
                       int iters, float *avg_ms, float *per_op_ms) {
    if (!m->prepared) fail(MF_ERR_INVALID_ARG, "model not prepared");
    if (iters <= 0 || !batch) fail(MF_ERR_INVALID_ARG, "iters and batch must be positive");
    MF_HIP(hipSetDevice(m->device));
    ensure_capacity(m, batch);
    const int nops = (int)m->pm.ops.size();
    hipStream_t s = m->stream;
    hipEvent_t e0, e1;
    MF_HIP(hipEventCreate(&e0));
    MF_HIP(hipEventCreate(&e1));
    for (int i = 0; i < warmup; ++i) model_run(m, nullptr, d_in, batch, nullptr, d_out, MF_MEM_DEVICE, -1);
    MF_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) model_run(m, nullptr, d_in, batch, nullptr, d_out, MF_MEM_DEVICE, -1);
    MF_HIP(hipEventRecord(e1, s));
    MF_HIP(hipEventSynchronize(e1));
    float ms = 0;
    MF_HIP(hipEventElapsedTime(&ms, e0, e1));
    if (avg_ms) *avg_ms = ms / (float)iters;

    if (per_op_ms) { // second sweep: one event pair per op, on the same stream
        std::vector<hipEvent_t> ev((size_t)nops + 1);
        for (auto &e : ev) MF_HIP(hipEventCreate(&e));
        std::vector<std::vector<float>> samples((size_t)nops); // per operator: one duration per iteration
        for (int it = 0; it < iters; ++it) {
            const int8_t *cur = d_in;
            int which = 0;
            MF_HIP(hipEventRecord(ev[0], s));
            for (int i = 0; i < nops; ++i) {
                OpImpl *o = m->ops[i];
                if (o) {
                    int8_t *dst = m->act[which];
                    if (dst == cur) {
                        which ^= 1;
                        dst = m->act[which];
                    }
                    const ModelImpl::Stage *st = stage_at(m, i, nops - 1);
                    if (st && (!fused_input_ok(st->f, cur) || !fused_batch_ok(st->f, (size_t)batch))) st = nullptr;
                    if (st) { // timed as one unit (index i), its other ops 0
                        fused_run(st->f, cur, batch, dst, s);
                        for (int j = i; j < st->last; ++j) MF_HIP(hipEventRecord(ev[(size_t)j + 1], s));
                        i = st->last;
                    } else if (fused_at(m, i) && fused_input_ok(m->fused[(size_t)i], cur)) { // the group is timed as one unit (index i), its other ops 0
                        fused_run(m->fused[(size_t)i], cur, batch, dst, s);
                        for (int j = i; j < m->fused_last[(size_t)i]; ++j) MF_HIP(hipEventRecord(ev[(size_t)j + 1], s));
                        i = m->fused_last[(size_t)i];
                    } else {
                        op_run(o, cur, batch, dst, s);
                    }
                    cur = dst;
                    which ^= 1;
                }
                MF_HIP(hipEventRecord(ev[(size_t)i + 1], s));
            }
            MF_HIP(hipEventSynchronize(ev[(size_t)nops]));
            for (int i = 0; i < nops; ++i) {
                float t = 0;
                MF_HIP(hipEventElapsedTime(&t, ev[(size_t)i], ev[(size_t)i + 1]));
                samples[(size_t)i].push_back(t);
            }
        }
        for (int i = 0; i < nops; ++i) { // median over the iterations
            std::vector<float> &v = samples[(size_t)i];
            std::sort(v.begin(), v.end());
            const size_t n = v.size();
            per_op_ms[i] = n % 2 ? v[n / 2] : 0.5f * (v[n / 2 - 1] + v[n / 2]);
        }
        for (auto &e : ev) (void)hipEventDestroy(e);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
}

} // namespace mf
