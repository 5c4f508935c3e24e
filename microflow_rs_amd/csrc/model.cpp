// model.cpp -- the runtime half of what #[model("x.tflite")] generates
// (microflow-macros/src/lib.rs:185-203): predict / predict_quantized /
// predict_inner over a BATCH of independent inferences.
//
// Device memory plan (sized for 288 GB of HBM, no reuse tricks needed):
//   weights + folded constants : resident per op (person_detect: ~0.3 MB)
//   act[0], act[1]             : ping-pong activation buffers, batch x max tensor bytes
//   in_q / io_f32              : staging for host-fed batches
//   fork[0], fork[1]           : models with a join (ADD, CONCATENATION) only -- where a tensor that a later join reads beside the running one is
//                                written, batch x largest such tensor; the ping-pong never writes there, so no skip is ever copied.
//                                A side operator's result (a Conv2D on a skip edge, run at its join) goes to the one that holds
//                                neither its input nor the running tensor -- where the two are not one launch, which writes neither
// Every op reads one buffer and writes the other; Reshape is an alias (the 2D<->4D
// maps of src/tensor.rs:103-141 are the identity in NHWC memory).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <memory>
#include <vector>

#include "mf_internal.hpp"
#include "model_groups.hpp"

namespace mf {

using Stage = ModelGroups::Stage;

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
    ModelGroups g; // operators, first-level groups, second-level stages (model_groups.hpp); empty until prepared
    bool fusion = true;
    bool autotune = false; // model_set_autotune: time the run-time-geometry chain candidates at creation
    size_t cap_batch = 0;
    int8_t *act[2] = {nullptr, nullptr};
    int8_t *fork[2] = {nullptr, nullptr}; // skip tensors (pm.max_fork_elems != 0): two, for a join whose result is the next skip
    std::vector<char> forks;  // per operator: its tensor (through the Reshapes behind it) is read by a later join (ADD, CONCATENATION) beside the running one
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
        g.clear();
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
        for (auto &p : fork) {
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
    m->forks.assign(m->pm.ops.size(), 0);
    for (size_t i = 0; i < m->pm.ops.size(); ++i)
        if (m->pm.ops[i].join() && m->pm.skip_real(i) >= 0) m->forks[(size_t)m->pm.skip_real(i)] = 1;
    return m.release();
}
void model_destroy(ModelImpl *m) { delete m; }
const ParsedModel &model_parsed(const ModelImpl *m) { return m->pm; }

// ---- which launch runs operator i ----
// The launch that starts at an operator: a second-level stage or a first-level group (f) over operators i .. last, or the
// operator's own (f == nullptr, last == i).  last < 0: no launch
struct Launch {
    FusedImpl *f;
    int last;
};
static bool fused_at(const ModelImpl *m, int i) {
    return m->fusion && !m->generic && i >= 0 && i < (int)m->g.fused.size() && m->g.fused[(size_t)i];
}
// the second-level group that starts at op i and ends at or before last_op, if any
static const Stage *stage_at(const ModelImpl *m, int i, int last_op) {
    if (!m->fusion || m->generic) return nullptr;
    for (const Stage &st : m->g.stages)
        if (st.first == i && st.last <= last_op) return &st;
    return nullptr;
}
// ... and the first-level group
static FusedImpl *group_at(const ModelImpl *m, int i, int last_op) {
    return fused_at(m, i) && m->g.fused_last[(size_t)i] <= last_op ? m->g.fused[(size_t)i] : nullptr;
}
// The launch of a run that ends at last_op, at operator i, on this input pointer and batch: the stage, else the group, else the
// operator (the operators' own launches take any pointer and batch; a group is not asked about the batch)
static Launch launch_at(const ModelImpl *m, int i, int last_op, const int8_t *d_in, size_t batch) {
    const Stage *st = stage_at(m, i, last_op);
    if (st && fused_input_ok(st->f, d_in) && fused_batch_ok(st->f, batch)) return {st->f, st->last};
    FusedImpl *f = group_at(m, i, last_op);
    if (f && fused_input_ok(f, d_in)) return {f, m->g.fused_last[(size_t)i]};
    return {nullptr, i};
}
// the stage a run from operator 0 uses for op i: the covering one that starts first
static const Stage *covering_stage(const ModelImpl *m, int i) {
    const Stage *best = nullptr;
    if (m->fusion && !m->generic)
        for (const Stage &st : m->g.stages)
            if (i >= st.first && i <= st.last && (!best || st.first < best->first)) best = &st;
    return best;
}
// index of the fused group that swallows op i (without being its first op), or -1
static int fused_owner(const ModelImpl *m, int i) {
    for (int j = i - 1; j >= 0 && j >= i - 4; --j)
        if (fused_at(m, j) && m->g.fused_last[(size_t)j] >= i) return j;
    return -1;
}
// the side operator + join launch (shortcut_add_rt at an ADD, side_concat_rt at a CONCATENATION) at join i, if the model has one there
// and nothing switched it off
static FusedImpl *side_join_at(const ModelImpl *m, int i) {
    return m->fusion && !m->generic && i >= 0 && i < (int)m->g.side_join.size() ? m->g.side_join[(size_t)i] : nullptr;
}
// ... and seen from the side operator: the join that reads its output
static int join_of_side(const ModelImpl *m, int i) {
    for (size_t k = (size_t)i + 1; k < m->pm.ops.size(); ++k)
        if (m->pm.side_of_join(k) == i) return (int)k;
    return -1;
}
const char *model_op_kernel(const ModelImpl *m, int i) {
    if (!m->prepared || i < 0 || i >= (int)m->g.ops.size() || !m->g.ops[i]) return "";
    // (the launch is named where it runs and where time_device(per_op) books its time: at the join)
    if (m->pm.ops[(size_t)i].side() && side_join_at(m, join_of_side(m, i)))
        return m->pm.ops[(size_t)join_of_side(m, i)].kind == MF_OP_CONCATENATION ? "(fused into its CONCATENATION)" : "(fused into its ADD)";
    if (side_join_at(m, i)) return fused_kernel_name(side_join_at(m, i));
    if (const Stage *best = covering_stage(m, i)) return best->first == i ? fused_kernel_name(best->f) : "(fused into the previous operator)";
    if (fused_at(m, i)) return fused_kernel_name(m->g.fused[(size_t)i]);
    if (fused_owner(m, i) >= 0) return "(fused into the previous operator)";
    return op_kernel_name(m->g.ops[i]);
}

int model_op_epilogue_mode(const ModelImpl *m, int i) { // (a swallowed operator answers with its own launch's mode)
    if (!m->prepared || i < 0 || i >= (int)m->g.ops.size() || !m->g.ops[i]) return -1;
    if (side_join_at(m, i)) return fused_epilogue_mode(side_join_at(m, i));
    const Stage *best = covering_stage(m, i);
    if (best && best->first == i) return fused_epilogue_mode(best->f);
    if (!best && fused_at(m, i)) return fused_epilogue_mode(m->g.fused[(size_t)i]);
    return op_epilogue_mode(m->g.ops[i]);
}

// ---- small helpers of the run paths ----
static bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t ab = (uintptr_t)a, ae = ab + a_bytes, bb = (uintptr_t)b, be = bb + b_bytes;
    return ab < be && bb < ae;
}
// operator last_op's tensor as a run that ends there returns it: the scale and zero point the operator stamped on it, elements per inference
struct OutQuant {
    float scale;
    int zp;
    size_t elems;
};
static OutQuant out_quant(const ParsedModel &pm, int last_op) {
    if (last_op == (int)pm.ops.size() - 1) return {pm.out_scale, pm.out_zp, pm.out_elems};
    const ParsedOp &po = pm.ops[(size_t)last_op];
    return {po.out_scale, po.out_zp, po.out_elems};
}
// What a call enqueues on the device, for mf_model_device_ops, added on every way out: its launches and device-to-device copies;
// one for a call that launches a graph (replay)
struct LaunchCount {
    ModelImpl *m;
    unsigned long long before = dev_launch_counter();
    bool replay = false;
    ~LaunchCount() { m->device_ops += replay ? 1 : dev_launch_counter() - before; }
};
// events of one call, destroyed on every way out
struct EventList {
    std::vector<hipEvent_t> v;
    EventList() = default;
    EventList(const EventList &) = delete;
    EventList &operator=(const EventList &) = delete;
    ~EventList() {
        for (hipEvent_t e : v)
            if (e) (void)hipEventDestroy(e);
    }
    hipEvent_t add(unsigned flags) {
        v.push_back(nullptr); // the slot first: a throwing push_back must not leak the event
        MF_HIP(hipEventCreateWithFlags(&v.back(), flags));
        return v.back();
    }
};

static void ensure_capacity(ModelImpl *m, size_t batch) {
    if (batch <= m->cap_batch) return;
    MF_HIP(hipSetDevice(m->device));
    MF_HIP(hipStreamSynchronize(m->stream));
    m->drop_graph();
    m->free_buffers();
    const ParsedModel &pm = m->pm;
    const size_t act_bytes = ((batch * pm.max_elems + 255) / 256) * 256 + 256;
    for (auto &p : m->act) MF_HIP(hipMalloc((void **)&p, act_bytes));
    if (pm.max_fork_elems)
        for (auto &p : m->fork) MF_HIP(hipMalloc((void **)&p, ((batch * pm.max_fork_elems + 255) / 256) * 256 + 256));
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
        // Everything is built in a local and committed only when all of it exists: a failure half way
        // (a HIP error, OOM, a geometry the operator rejects) leaves the model unprepared and retryable,
        // on this or another device.
        m->g = build_groups(m->pm, device, m->autotune);
        m->device = device;
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
    for (OpImpl *o : m->g.ops)
        if (o) op_set_generic(o, generic);
}

// Which launch of a run of ops [0 .. last_op] takes the f32 input itself (the boundary quantize inside it)?  The second-level
// group that starts at the first operator (penta_rr, fc_chain, dwc1_fc_softmax), else the first-level group there, else that operator alone (the stem kernel, fc_rt: the
// groups behind it run as usual); last < 0: none.  A stage there that does not take f32 blocks the group, a group the operator
static Launch f32_entry(const ModelImpl *m, int last_op) {
    const Launch none{nullptr, -1};
    const int f = m->g.first_real;
    if (!m->fusion || m->generic || f > last_op || f >= (int)m->g.ops.size() || m->pm.input_skip) return none;
    const Stage *st0 = stage_at(m, f, last_op);
    if (st0 && fused_accepts_f32(st0->f)) return {st0->f, st0->last};
    FusedImpl *g = group_at(m, f, last_op);
    if (!st0 && g && fused_accepts_f32(g)) return {g, m->g.fused_last[(size_t)f]};
    if (!fused_at(m, f) && op_accepts_f32(m->g.ops[(size_t)f])) return {nullptr, f};
    return none;
}
// the last operator at or before last_op that launches anything (trailing Reshapes alias its output)
// (a side operator in front of them is not on the chain they alias: passed over, unless the run ends at it)
static int last_real_upto(const ModelImpl *m, int last_op) {
    const int end = last_op;
    while (last_op >= 0 && (!m->g.ops[(size_t)last_op] || (last_op != end && m->pm.ops[(size_t)last_op].side()))) --last_op;
    return last_op;
}

// A run of ops [0 .. last_op] in flight: where the running tensor is, and what the two ends of the run ask for (run_ops)
struct Run {
    const int8_t *cur; // the running tensor
    const int8_t *skip; // the live skip tensor, which the next join (ADD, CONCATENATION) reads beside it: the model input where a join reads that (start_run), then every fork tensor as it is written
    size_t batch;
    int last_op, last_real;
    hipStream_t stream;
    const float *src_f32 = nullptr;
    Launch entry{nullptr, -1}; // with src_f32: the launch that takes it (f32_entry)
    int8_t *final_dst = nullptr;
    float *final_f32 = nullptr;
    int which = 0;         // the activation buffer the next launch writes, unless it is reading it
    bool left_f32 = false; // the last launch stored floats at final_f32: there is no int8 result
};
// The launch of the run at operator i (not a Reshape): picks the destination of the ping-pong, selects the launch, runs it -- the int8
// form or, with a model boundary inside it, the f32-edge form -- and returns the last operator it covered
static int run_step(ModelImpl *m, Run &r, int i) {
    OpImpl *o = m->g.ops[(size_t)i];
    const bool f32in = r.src_f32 && i == m->g.first_real;
    const bool join = m->pm.ops[(size_t)i].join(); // an ADD or a CONCATENATION: a launch of its own: the running tensor and the live skip tensor
    int8_t *dst = m->act[r.which];
    if (dst == r.cur) {
        r.which ^= 1;
        dst = m->act[r.which];
    }
    const int side = join ? m->pm.side_of_join((size_t)i) : -1; // the join reads a side operator's output: that operator runs here, from the live skip
    const bool side_alone = m->pm.ops[(size_t)i].side();      // a run that ends at a side operator (run_until): its result from the live skip
    const Launch l = f32in ? r.entry : (join || side_alone) ? Launch{nullptr, i} : launch_at(m, i, r.last_op, r.cur, r.batch);
    // A launch whose result a later join reads beside the running value writes it where the ping-pong never writes: the fork buffer
    // that does not hold the live skip (a join may read one and write the other).  No group holds such a tensor inside
    // (model_groups.cpp: splits), so it is always a launch's result
    const bool forks = m->forks[(size_t)l.last] != 0;
    if (forks) dst = (m->fork[0] == r.skip || m->fork[0] == r.cur) ? m->fork[1] : m->fork[0];
    const bool ends = l.last >= r.last_real;
    const bool f32out = r.final_f32 && ends && (l.f ? fused_emits_f32(l.f) : op_emits_f32(o));
    if (r.final_dst && ends) dst = r.final_dst;
    if (f32in || f32out) { // a model boundary inside the launch
        const void *in = f32in ? (const void *)r.src_f32 : (const void *)r.cur;
        void *out = f32out ? (void *)r.final_f32 : (void *)dst;
        if (l.f) fused_run_f32(l.f, in, f32in, r.batch, out, f32out, r.stream);
        else op_run_f32(o, in, f32in, r.batch, out, f32out, r.stream);
        r.left_f32 = f32out;
    } else if (l.f) { // several groups, or the whole group, in one launch
        fused_run(l.f, r.cur, r.batch, dst, r.stream);
    } else if (side >= 0 && side_join_at(m, i)) { // the side operator and the join in one launch: its result is never written
        fused_run2(side_join_at(m, i), r.skip, r.cur, r.batch, dst, r.stream);
    } else if (join) { // (the operand order is the file's: it matters for an ADD's f32 sum)
        const int8_t *other = r.skip;
        if (side >= 0) { // T stays where it is; S goes to the fork buffer that holds neither T nor the running tensor
            int8_t *s_buf = (m->fork[0] == r.skip || m->fork[0] == r.cur) ? m->fork[1] : m->fork[0];
            // (a CONCATENATION writes beside both inputs: where its own result goes to that fork buffer, S takes the activation
            // buffer that holds neither the running tensor nor that result)
            if (m->pm.ops[(size_t)i].kind == MF_OP_CONCATENATION && s_buf == dst) s_buf = m->act[0] == r.cur ? m->act[1] : m->act[0];
            op_run(m->g.ops[(size_t)side], r.skip, r.batch, s_buf, r.stream);
            other = s_buf;
        }
        const bool run_first = m->pm.ops[(size_t)i].run_input == 0;
        op_run2(o, run_first ? r.cur : other, run_first ? other : r.cur, r.batch, dst, r.stream, false);
    } else if (side_alone) {
        op_run(o, r.skip, r.batch, dst, r.stream);
    } else {
        op_run(o, r.cur, r.batch, dst, r.stream);
    }
    if (forks) r.skip = dst;
    r.cur = dst;
    r.which ^= 1;
    return l.last;
}

// run ops [0..last_op]; `src_f32` != nullptr (only where f32_entry says so): the first launch consumes the f32 input directly.
// `final_dst` != nullptr: the launch that produces operator last_op's tensor writes it there instead of into an activation buffer
// (no copy of the result afterwards: 16 MB per step for the 4096^3 FullyConnected).  `final_f32` != nullptr: that launch stores the
// dequantised floats there if it has such an instance.  The return value says where the int8 result is; nullptr: it left as floats.
static const int8_t *run_ops(ModelImpl *m, const int8_t *src, size_t batch, int last_op, hipStream_t stream,
                             const float *src_f32 = nullptr, int8_t *final_dst = nullptr, float *final_f32 = nullptr) {
    Run r{src, m->pm.input_skip ? src : nullptr, batch, last_op, last_real_upto(m, last_op), stream, src_f32};
    if (src_f32) r.entry = f32_entry(m, last_op);
    if (src_f32 && r.entry.last < 0) fail(MF_ERR_UNSUPPORTED, "no launch takes the f32 input");
    r.final_dst = final_dst, r.final_f32 = final_f32;
    for (int i = 0; i <= last_op && !r.left_f32; ++i) // (a Reshape is an alias; a side operator runs at its join, or where the run ends at it)
        if (m->g.ops[(size_t)i] && !(m->pm.ops[(size_t)i].side() && i != last_op)) i = run_step(m, r, i);
    return r.left_f32 ? nullptr : r.cur;
}

// Can any launch that ends the whole model -- the last real operator's own, a group or a stage that ends there -- store floats?
static bool f32_exit_any(const ModelImpl *m) {
    const ModelGroups &g = m->g;
    if (g.last_real < 0) return false;
    if (op_emits_f32(g.ops[(size_t)g.last_real])) return true;
    for (size_t i = 0; i < g.fused.size(); ++i)
        if (g.fused[i] && g.fused_last[i] == g.last_real && fused_emits_f32(g.fused[i])) return true;
    for (const Stage &st : g.stages)
        if (st.last == g.last_real && fused_emits_f32(st.f)) return true;
    return false;
}
// Which of M::predict's two boundary conversions run inside the first / last launch of this call: only with fusion on, the
// shape-specialised kernels, the whole model, a 16-byte aligned f32 input (float4 loads) and a 4-byte aligned f32 output; and the
// exit only where the output range does not overlap the input's, which the first launch -- possibly the same one -- is still reading.
// Otherwise that side keeps its separate pass, with the same bits.
struct Boundary {
    bool in = false, out = false;
};
static Boundary boundary_plan(const ModelImpl *m, const float *in_f32, const float *out_f32, size_t out_count, const void *in_any, size_t in_bytes,
                              int last_op) {
    Boundary b;
    if (!m->fusion || m->generic || last_op != (int)m->pm.ops.size() - 1) return b;
    // (a model whose join reads the quantised input has no f32 entry -- nothing would materialise it: rule (7) -- so f32_entry says no)
    b.in = in_f32 && ((uintptr_t)in_f32 & 15) == 0 && f32_entry(m, last_op).last >= 0;
    b.out = out_f32 && ((uintptr_t)out_f32 & 3) == 0 && !ranges_overlap(out_f32, out_count * sizeof(float), in_any, in_bytes);
    return b;
}

// The whole device-resident sequence (boundary conversion -> ops -> boundary conversion) on
// `s`: every pointer is a device pointer, nothing synchronizes -- so it can be stream-captured.
static void enqueue_device(ModelImpl *m, const float *in_f32, const int8_t *in_i8, size_t batch,
                           float *out_f32, int8_t *out_i8, int last_op, hipStream_t s) {
    const ParsedModel &pm = m->pm;
    const OutQuant oq = out_quant(pm, last_op);
    const size_t out_elems = oq.elems;
    const void *in_any = in_f32 ? (const void *)in_f32 : (const void *)in_i8;
    const size_t in_bytes = batch * pm.in_elems * (in_f32 ? sizeof(float) : 1);
    const int8_t *q_in;
    const Boundary bd = boundary_plan(m, in_f32, out_f32, batch * out_elems, in_any, in_bytes, last_op);
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
    if (direct && ranges_overlap(out_i8, batch * out_elems, in_any, in_bytes)) direct = nullptr;
    const int8_t *res = run_ops(m, q_in, batch, last_op, s, fuse_q ? in_f32 : nullptr, direct, bd.out ? out_f32 : nullptr);
    if (out_i8) {
        if (pm.u8) dev_xor80(m->device, res, batch * out_elems, out_i8, s);
        else if (res != out_i8) {
            MF_HIP(hipMemcpyAsync(out_i8, res, batch * out_elems, hipMemcpyDeviceToDevice, s));
            ++dev_launch_counter();
        }
    } else if (res) { // .dequantize()  (lib.rs:190) with the parameters the last op stamped on the tensor
        dev_dequantize(m->device, res, batch * out_elems, oq.scale, oq.zp, pm.u8, out_f32, s);
    }
}

// device path with graph replay: eager the first time a key is seen, captured the second time
static void run_device(ModelImpl *m, const float *in_f32, const int8_t *in_i8, size_t batch,
                       float *out_f32, int8_t *out_i8, int last_op) {
    hipStream_t s = m->stream;
    // what this call enqueues, for mf_model_device_ops: the launches and device-to-device copies of an eager pass; one for a call that
    // launches the graph -- a replay, and also the call that captures it, which records its launches instead of enqueueing them and
    // then launches the new graph once
    LaunchCount count{m};
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
    MF_HIP(hipSetDevice(m->device));
    ensure_capacity(m, batch);
    const OutQuant oq = out_quant(pm, last_op); // (host path) .dequantize() takes the parameters the last op stamped on the tensor
    const size_t out_elems = oq.elems;
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
    EventList evs;
    LaunchCount ops_added{m};
    if (out_f32 && !m->o_f32 && m->fusion && !m->generic && last_op == nops - 1 && f32_exit_any(m))
        MF_HIP(hipMalloc((void **)&m->o_f32, m->cap_batch * pm.out_elems * sizeof(float) + 256));
    try {
        if (chunk < batch) { // the copy stream starts after whatever the caller queued on the compute stream
            hipEvent_t e = evs.add(hipEventDisableTiming);
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
                hipEvent_t e = evs.add(hipEventDisableTiming);
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
                if (res) dev_dequantize(m->device, res, n * out_elems, oq.scale, oq.zp, pm.u8, fo, s);
                MF_HIP(hipMemcpyAsync(out_f32 + first * out_elems, res ? fo : fo_direct, n * out_bytes, hipMemcpyDeviceToHost, s));
            }
        }
        MF_HIP(hipStreamSynchronize(s));
    } catch (...) {
        if (m->copy_stream) (void)hipStreamSynchronize(m->copy_stream);
        (void)hipStreamSynchronize(s);
        throw;
    }
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
        const void *sb = (const void *)((src_f32 ? (uintptr_t)src_f32 : (uintptr_t)src_i8) + lo * esz);
        const void *ob = out_f32 ? (const void *)out_f32 : (const void *)out_i8;
        if (ranges_overlap(ob, count * pm.out_elems * osz, sb, span * esz)) fail(MF_ERR_INVALID_ARG, "src and out overlap");
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
    EventList evs;
    LaunchCount ops_added{m};
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
                hipEvent_t e = evs.add(hipEventDisableTiming);
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
        throw;
    }
}

void model_time_device(ModelImpl *m, const int8_t *d_in, size_t batch, int8_t *d_out, int warmup,
                       int iters, float *avg_ms, float *per_op_ms) {
    if (!m->prepared) fail(MF_ERR_INVALID_ARG, "model not prepared");
    if (iters <= 0 || !batch) fail(MF_ERR_INVALID_ARG, "iters and batch must be positive");
    MF_HIP(hipSetDevice(m->device));
    ensure_capacity(m, batch);
    const int nops = (int)m->pm.ops.size();
    hipStream_t s = m->stream;
    EventList evs; // e0, e1, then the sweep's nops + 1
    const hipEvent_t e0 = evs.add(hipEventDefault), e1 = evs.add(hipEventDefault);
    for (int i = 0; i < warmup; ++i) model_run(m, nullptr, d_in, batch, nullptr, d_out, MF_MEM_DEVICE, -1);
    MF_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) model_run(m, nullptr, d_in, batch, nullptr, d_out, MF_MEM_DEVICE, -1);
    MF_HIP(hipEventRecord(e1, s));
    MF_HIP(hipEventSynchronize(e1));
    float ms = 0;
    MF_HIP(hipEventElapsedTime(&ms, e0, e1));
    if (avg_ms) *avg_ms = ms / (float)iters;
    if (!per_op_ms) return;

    // second sweep: one event pair per op, on the same stream; run_ops' steps with an event behind each (these launches are not
    // added to mf_model_device_ops)
    for (int i = 0; i <= nops; ++i) evs.add(hipEventDefault);
    const hipEvent_t *ev = evs.v.data() + 2;
    std::vector<std::vector<float>> samples((size_t)nops); // per operator: one duration per iteration
    for (int it = 0; it < iters; ++it) {
        Run r{d_in, m->pm.input_skip ? d_in : nullptr, batch, nops - 1, m->g.last_real, s};
        MF_HIP(hipEventRecord(ev[0], s));
        for (int i = 0; i < nops; ++i) {
            if (m->g.ops[(size_t)i] && !m->pm.ops[(size_t)i].side()) { // a stage or a group is timed as one unit (index i), its other ops 0; a side operator at its join
                const int end = run_step(m, r, i);
                for (; i < end; ++i) MF_HIP(hipEventRecord(ev[(size_t)i + 1], s));
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
}

} // namespace mf
