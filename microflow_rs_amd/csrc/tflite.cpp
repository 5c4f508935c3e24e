// tflite.cpp -- reads a .tflite FlatBuffer into a ParsedModel and runs the
// constant preparation for every operator.  This is the host-side replacement of
// the proc-macro's front half (microflow-macros/src/lib.rs:46-151 and the
// Token*::new() constructors in microflow-macros/src/ops/*.rs); the generated
// flatbuffers bindings (23k lines upstream) are replaced by a bounds-checked
// cursor over the handful of tables the path reads.  Field ids are from
// microflow-macros/flatbuffers/tflite.fbs.
#include <cmath>
#include <cstring>

#include "mf_internal.hpp"

namespace mf {
namespace {

class Buf {
  public:
    Buf(const uint8_t *p, size_t n) : p_(p), n_(n) {}
    template <typename T> T at(size_t off) const {
        if (off + sizeof(T) > n_ || off + sizeof(T) < off)
            fail(MF_ERR_INVALID_MODEL, "invalid model, please provide a valid TensorFlow Lite model");
        T v;
        std::memcpy(&v, p_ + off, sizeof(T));
        return v;
    }
    const uint8_t *ptr(size_t off, size_t len) const {
        if (off + len > n_ || off + len < off)
            fail(MF_ERR_INVALID_MODEL, "invalid model, please provide a valid TensorFlow Lite model");
        return p_ + off;
    }

  private:
    const uint8_t *p_;
    size_t n_;
};

// a FlatBuffers table: position + vtable lookup
struct Table {
    const Buf *b = nullptr;
    size_t pos = 0;
    explicit operator bool() const { return b != nullptr; }
    size_t field(int id) const { // absolute offset of the field, 0 if absent
        if (!b) return 0;
        const int32_t soff = b->at<int32_t>(pos);
        const size_t vt = (size_t)((int64_t)pos - soff);
        const uint16_t vsize = b->at<uint16_t>(vt);
        const size_t slot = 4 + 2 * (size_t)id;
        if (slot + 2 > vsize) return 0;
        const uint16_t o = b->at<uint16_t>(vt + slot);
        return o ? pos + o : 0;
    }
    template <typename T> T scalar(int id, T dflt) const {
        const size_t f = field(id);
        return f ? b->at<T>(f) : dflt;
    }
    Table table(int id) const {
        const size_t f = field(id);
        if (!f) return {};
        return {b, f + b->at<uint32_t>(f)};
    }
};
struct Vec {
    const Buf *b = nullptr;
    size_t pos = 0; // points at the length word
    uint32_t size() const { return b ? b->at<uint32_t>(pos) : 0; }
    template <typename T> T get(uint32_t i) const { return b->at<T>(pos + 4 + sizeof(T) * (size_t)i); }
    Table table(uint32_t i) const {
        const size_t e = pos + 4 + 4 * (size_t)i;
        return {b, e + b->at<uint32_t>(e)};
    }
    const uint8_t *bytes(size_t len) const { return b->ptr(pos + 4, len); }
};
Vec vec(const Table &t, int id) {
    const size_t f = t.field(id);
    if (!f) return {};
    return {t.b, f + t.b->at<uint32_t>(f)};
}

enum { TT_INT32 = 2, TT_UINT8 = 3, TT_INT64 = 4, TT_INT8 = 9 };
enum { BUILTIN_PADV2 = 60, BUILTIN_MIRROR_PAD = 100 }; // the neighbours of PAD, refused by name

struct TensorInfo {
    std::vector<int> shape;
    int type = 0;
    std::vector<float> scale;
    std::vector<int64_t> zp;
    const uint8_t *data = nullptr;
    size_t data_len = 0;
    size_t elems() const { // dimensions are <= 2^24 each (read_tensor): cap the product well below size_t overflow
        size_t n = 1;
        for (int s : shape) {
            n *= (size_t)s;
            if (n > ((size_t)1 << 40)) fail(MF_ERR_INVALID_MODEL, "invalid model: tensor too large");
        }
        return n;
    }
};

// Tensor { shape:0 type:1 buffer:2 name:3 quantization:4 }
// QuantizationParameters { min:0 max:1 scale:2 zero_point:3 }   Buffer { data:0 }
TensorInfo read_tensor(const Vec &tensors, const Vec &buffers, int32_t index) {
    if (index < 0 || (uint32_t)index >= tensors.size())
        fail(MF_ERR_INVALID_MODEL, "invalid model: tensor index out of range");
    const Table t = tensors.table((uint32_t)index);
    TensorInfo ti;
    const Vec sh = vec(t, 0);
    if (sh.size() > 4) fail(MF_ERR_UNSUPPORTED, "unsupported tensor rank: " + std::to_string(sh.size()));
    for (uint32_t i = 0; i < sh.size(); ++i) {
        const int32_t d = sh.get<int32_t>(i);
        if (d <= 0 || d > (1 << 24)) fail(MF_ERR_INVALID_MODEL, "invalid model: bad tensor dimension");
        ti.shape.push_back(d);
    }
    ti.type = t.scalar<int8_t>(1, 0);
    const Table q = t.table(4);
    if (q) {
        const Vec sc = vec(q, 2), zp = vec(q, 3);
        for (uint32_t i = 0; i < sc.size(); ++i) ti.scale.push_back(sc.get<float>(i));
        for (uint32_t i = 0; i < zp.size(); ++i) ti.zp.push_back(zp.get<int64_t>(i));
    }
    const uint32_t bi = t.scalar<uint32_t>(2, 0);
    if (bi < buffers.size()) {
        const Vec d = vec(buffers.table(bi), 0);
        if (d.b) {
            ti.data_len = d.size();
            ti.data = d.bytes(ti.data_len);
        }
    }
    return ti;
}

// rank-1 shapes get a leading 1 (lib.rs:67-70, microflow-macros/src/tensor.rs:67-70)
void fix_rank1(TensorInfo &t) {
    if (t.shape.size() == 1) t.shape.insert(t.shape.begin(), 1);
}

void need_quant(const TensorInfo &t, const char *what) {
    if (t.scale.empty() || t.zp.empty())
        fail(MF_ERR_INVALID_MODEL, std::string("invalid model: ") + what + " has no quantization");
}

// The reference monomorphises every operator on its input tensor's type (i8 or u8, e.g.
// microflow-macros/src/ops/conv_2d.rs:58-83); a model whose tensors mix the two does not
// type-check there.  Here: every quantized tensor must have the model input's type.
void require_elem(const TensorInfo &t, const char *op, bool u8) {
    if (t.type != TT_INT8 && t.type != TT_UINT8)
        fail(MF_ERR_UNSUPPORTED, std::string(op) + " supports only INT8/UINT8 input tensors, got type " +
                                     std::to_string(t.type));
    if ((t.type == TT_UINT8) != u8)
        fail(MF_ERR_UNSUPPORTED, std::string(op) + ": tensor element type differs from the model input's (mixed INT8/UINT8)");
}
// zero points are i64 in the file and cast to T (microflow-macros/src/tensor.rs:81-88)
int zp_of(int64_t z, bool u8) { return u8 ? (int)(uint8_t)z : (int)(int8_t)z; }

int check_act(int a) { // microflow-macros/src/activation.rs:26-38
    if (a != MF_ACT_NONE && a != MF_ACT_RELU && a != MF_ACT_RELU6)
        fail(MF_ERR_UNSUPPORTED, "unsupported fused activation: " + std::to_string(a) +
                                     ". Supported activations are NONE, RELU, and RELU6");
    return a;
}
int check_pad(int p) {
    if (p != MF_PAD_SAME && p != MF_PAD_VALID) fail(MF_ERR_INVALID_MODEL, "invalid model: bad padding");
    return p;
}

void set_shapes(ParsedOp &op, const TensorInfo &in, const TensorInfo &out, bool u8) {
    op.in_rank = (int)in.shape.size();
    op.out_rank = (int)out.shape.size();
    for (int i = 0; i < op.in_rank; ++i) op.in_shape[i] = in.shape[i];
    for (int i = 0; i < op.out_rank; ++i) op.out_shape[i] = out.shape[i];
    op.in_elems = in.elems();
    op.out_elems = out.elems();
    if (!in.scale.empty()) op.in_scale = in.scale[0];
    if (!in.zp.empty()) op.in_zp = zp_of(in.zp[0], u8);
    if (!out.scale.empty()) op.out_scale = out.scale[0];
    if (!out.zp.empty()) op.out_zp = zp_of(out.zp[0], u8);
}

} // namespace

ParsedModel parse_tflite(const uint8_t *data, size_t len) {
    if (!data || len < 8) fail(MF_ERR_INVALID_MODEL, "invalid model, please provide a valid TensorFlow Lite model");
    const Buf buf(data, len);
    // Model { version:0 operator_codes:1 subgraphs:2 description:3 buffers:4 }
    const Table model{&buf, buf.at<uint32_t>(0)};
    const Vec opcodes = vec(model, 1), subgraphs = vec(model, 2), buffers = vec(model, 4);
    if (!opcodes.b || !subgraphs.b || !buffers.b || subgraphs.size() < 1)
        fail(MF_ERR_INVALID_MODEL, "invalid model, please provide a valid TensorFlow Lite model");
    // SubGraph { tensors:0 inputs:1 outputs:2 operators:3 } -- subgraph 0 only (lib.rs:62)
    const Table sg = subgraphs.table(0);
    const Vec tensors = vec(sg, 0), g_in = vec(sg, 1), g_out = vec(sg, 2), operators = vec(sg, 3);
    if (!tensors.b || !g_in.size() || !g_out.size() || !operators.b)
        fail(MF_ERR_INVALID_MODEL, "invalid model, please provide a valid TensorFlow Lite model");

    ParsedModel pm;
    { // model input (lib.rs:66-126)
        TensorInfo t = read_tensor(tensors, buffers, g_in.get<int32_t>(0));
        fix_rank1(t);
        if (t.type != TT_INT8 && t.type != TT_UINT8)
            fail(MF_ERR_UNSUPPORTED, "unsupported input tensor type: " + std::to_string(t.type) +
                                         ". Supported input types are INT8 and UINT8");
        if (t.shape.size() != 2 && t.shape.size() != 4)
            fail(MF_ERR_UNSUPPORTED, "unsupported input tensor rank: " + std::to_string(t.shape.size()) +
                                         ". Supported ranks are 2 and 4");
        need_quant(t, "model input");
        pm.u8 = t.type == TT_UINT8;
        pm.in_rank = (int)t.shape.size();
        for (int i = 0; i < pm.in_rank; ++i) pm.in_shape[i] = t.shape[i];
        pm.in_scale = t.scale[0];
        pm.in_zp = zp_of(t.zp[0], pm.u8);
        pm.in_elems = t.elems();
    }
    { // model output (lib.rs:153-183)
        TensorInfo t = read_tensor(tensors, buffers, g_out.get<int32_t>(0));
        fix_rank1(t);
        if (t.type != TT_INT8 && t.type != TT_UINT8)
            fail(MF_ERR_UNSUPPORTED, "unsupported output tensor type: " + std::to_string(t.type) +
                                         ". Supported output types are INT8 and UINT8");
        if ((t.type == TT_UINT8) != pm.u8)
            fail(MF_ERR_UNSUPPORTED, "model input and output element types differ (mixed INT8/UINT8)");
        if (t.shape.size() != 2 && t.shape.size() != 4)
            fail(MF_ERR_UNSUPPORTED, "unsupported output tensor rank: " + std::to_string(t.shape.size()) +
                                         ". Supported ranks are 2 and 4");
        need_quant(t, "model output");
        pm.out_rank = (int)t.shape.size();
        for (int i = 0; i < pm.out_rank; ++i) pm.out_shape[i] = t.shape[i];
        pm.out_scale = t.scale[0];
        pm.out_zp = zp_of(t.zp[0], pm.u8);
        pm.out_elems = t.elems();
    }
    pm.max_elems = pm.in_elems;
    // The macro threads ONE running value through the operators (`let input = op(input, ...)`,
    // lib.rs:130-151), so operator i consumes operator i-1's result whatever tensor indices the file
    // names; a shape disagreement is a Rust type error there.  Here it would make a kernel read its
    // input with the wrong per-inference stride, so the chain is checked: tensor index, or at least the
    // same shape, from the graph input through every operator to the graph output.
    int32_t prev_index = g_in.get<int32_t>(0);
    std::vector<int> prev_shape(pm.in_shape, pm.in_shape + pm.in_rank);
    // ... with skip edges (the joins, below): the output tensor index of every operator so far, and the last join -- the point up to
    // which an earlier skip tensor was alive
    std::vector<int32_t> out_index;
    int last_join = -1;
    // ... and with a side operator (one Conv2D on a skip edge, below): the one whose join has not come yet, or -1
    int pending_side = -1;
    // who reads tensor t behind operator `from`: joins -- ADDs and CONCATENATIONs -- (any input) and other operators (input 0)
    auto readers_behind = [&](int32_t t, uint32_t from, int &joins, int &others) {
        joins = others = 0;
        for (uint32_t k = from + 1; k < operators.size(); ++k) {
            const Table o = operators.table(k);
            const uint32_t c = o.scalar<uint32_t>(0, 0);
            const Vec in_k = vec(o, 1);
            if (c >= opcodes.size() || !in_k.size()) continue; // (refused when the walk reaches it)
            const int code_k = opcodes.table(c).scalar<int8_t>(0, 0);
            if (code_k == MF_OP_ADD) joins += in_k.get<int32_t>(0) == t || (in_k.size() > 1 && in_k.get<int32_t>(1) == t);
            else if (code_k == MF_OP_CONCATENATION) {
                bool reads = false;
                for (uint32_t j = 0; j < in_k.size(); ++j) reads = reads || in_k.get<int32_t>(j) == t;
                joins += reads;
            } else others += in_k.get<int32_t>(0) == t;
        }
    };
    // the non-linear graphs that stay refused keep the chain check's answer, with the reason behind it
    auto refuse_side = [](uint32_t oi, const std::string &why) {
        fail(MF_ERR_UNSUPPORTED, "operator " + std::to_string(oi) + " does not consume the previous operator's output (or the model "
                                 "input): only linear operator chains are supported (side operator: " + why + ")");
    };
    auto same_tensor = [](std::vector<int> a, std::vector<int> b) {
        if (a.size() == 1) a.insert(a.begin(), 1);
        if (b.size() == 1) b.insert(b.begin(), 1);
        return a == b;
    };

    // What the two joins share.  A join reads the running value (in either position) and ONE other tensor, matched by tensor index: an
    // earlier tensor of the chain or the pending side operator's output; at most one such tensor is alive at a time.  In order: the
    // operands (two, none constant, of the model's element type with per-tensor quantisation; `fused_act`: the kind takes no fused
    // activation and the file names one), which input is the running one, the skip source and the three liveness refusals; then the
    // kind's `own` checks and fields (it gets the second tensor; po.run_input, skip_src and the a_* / b_* fields are set by then, the
    // shapes not yet); then the shapes and what has to stay in memory up to here.  Every refusal carries the kind's prefix (`refuse`)
    auto parse_join = [&](ParsedOp &po, uint32_t oi, const Vec &ins, const TensorInfo &in, const TensorInfo &out, int32_t running_index, const char *name,
                          const auto &refuse, const char *arity, bool fused_act, const auto &own) {
        if (ins.size() < 2) refuse(arity);
        const int32_t ia = ins.get<int32_t>(0), ib = ins.get<int32_t>(1);
        const TensorInfo tb = read_tensor(tensors, buffers, ib);
        if (in.data_len || tb.data_len) refuse("a constant operand");
        if (ins.size() != 2) refuse(arity);
        for (const TensorInfo *t : {&in, &tb, &out}) {
            if ((t->type != TT_INT8 && t->type != TT_UINT8) || (t->type == TT_UINT8) != pm.u8) refuse("mixed element types");
            need_quant(*t, name);
            if (t->scale.size() != 1 || t->zp.size() != 1) refuse("per-channel quantisation on an operand");
            if (!(t->scale[0] > 0.0f) || !std::isfinite(t->scale[0]))
                fail(MF_ERR_INVALID_MODEL, std::string("invalid model: ") + name + " scales must be finite and positive");
        }
        if (fused_act) refuse("a fused activation");
        if (ia == ib) refuse("both inputs are the same tensor");
        if (ia != running_index && ib != running_index) refuse("neither input is the running value");
        po.run_input = ia == running_index ? 0 : 1;
        const int32_t is = po.run_input == 0 ? ib : ia;
        int src = -2;
        if (is == g_in.get<int32_t>(0)) src = -1;
        for (size_t j = 0; j < out_index.size(); ++j)
            if (out_index[j] == is) src = (int)j;
        if (src == -2) refuse("the other input is no earlier tensor of the chain");
        for (const ParsedOp &e : pm.ops)
            if (e.join() && e.skip_src == src) refuse("a fork tensor is used twice");
        // (a side operator's output: T and S count as one skip, alive from T's producer -- checked at the side operator -- to here)
        const bool via_side = src >= 0 && pm.ops[(size_t)src].side();
        if (pending_side >= 0 && src != pending_side) refuse("a side operator while another skip is alive");
        if (!via_side && src < last_join) refuse("two skip tensors alive at once (overlapping or nested skips)");
        po.skip_src = src;
        po.a_scale = in.scale[0], po.b_scale = tb.scale[0];
        po.a_zp = zp_of(in.zp[0], pm.u8), po.b_zp = zp_of(tb.zp[0], pm.u8);
        own(tb);
        set_shapes(po, po.run_input == 0 ? in : tb, out, pm.u8); // (in_scale / in_zp / in_elems: the running operand's)
        // what has to stay in memory up to here: the skip tensor itself or, through a side operator, its input T (Reshapes are
        // aliases: the operator that launches the tensor, or the model input); the side operator's output lives in a fork buffer too
        const int real = pm.launcher(via_side ? pm.ops[(size_t)src].side_src : src);
        const size_t kept = via_side ? pm.ops[(size_t)src].in_elems : po.skip_elems();
        if (real < 0) pm.input_skip = true;
        else if (kept > pm.max_fork_elems) pm.max_fork_elems = kept;
        if (via_side && po.skip_elems() > pm.max_fork_elems) pm.max_fork_elems = po.skip_elems();
        pending_side = -1;
        last_join = (int)oi;
    };

    for (uint32_t oi = 0; oi < operators.size(); ++oi) { // lib.rs:130-151
        // Operator { opcode_index:0 inputs:1 outputs:2 builtin_options_type:3 builtin_options:4 }
        const Table op = operators.table(oi);
        const uint32_t oc = op.scalar<uint32_t>(0, 0);
        if (oc >= opcodes.size()) fail(MF_ERR_INVALID_MODEL, "invalid model: opcode index out of range");
        // OperatorCode { deprecated_builtin_code:0 } is what the reference dispatches on
        const int code = opcodes.table(oc).scalar<int8_t>(0, 0);
        const Vec ins = vec(op, 1), outs = vec(op, 2);
        const Table opt = op.table(4);
        if (!ins.size() || !outs.size()) fail(MF_ERR_INVALID_MODEL, "invalid model: operator without tensors");
        TensorInfo in = read_tensor(tensors, buffers, ins.get<int32_t>(0));
        TensorInfo out = read_tensor(tensors, buffers, outs.get<int32_t>(0));
        const int32_t running_index = prev_index;
        ParsedOp po;
        po.kind = code;
        if (code != MF_OP_ADD && code != MF_OP_CONCATENATION) { // (a join checks its own inputs)
            // A side operator: ONE Conv2D on a skip edge.  Its input 0 is a tensor T of the chain, by index -- the model input or an
            // earlier operator's output -- that the main chain also continues from: either T is not the running value any more (the
            // side operator stands between the main operators or in front of its join), or it still is and a later operator reads
            // it as well (the side operator stands directly behind the fork).  Its output is read by exactly one later join and by
            // nothing else.  It does not become the running value: the chain bookkeeping passes over it
            const int32_t in0 = ins.get<int32_t>(0);
            if (pending_side >= 0 && in0 == out_index[(size_t)pending_side]) refuse_side(oi, "two or more operators on the skip edge");
            int t = in0 == g_in.get<int32_t>(0) ? -1 : -2;
            for (size_t j = 0; j < out_index.size(); ++j)
                if (out_index[j] == in0 && !pm.ops[j].side()) t = (int)j;
            int joins = 0, others = 0;
            bool side = false;
            if (t != -2 && in0 != prev_index) side = true;
            else if (t != -2) { // (of two operators that read the running value, the one no further operator reads is off the chain)
                readers_behind(in0, oi, joins, others);
                const bool read_again = others > 0;
                readers_behind(outs.get<int32_t>(0), oi, joins, others);
                side = read_again && others == 0;
            }
            if (side) {
                if (code != MF_OP_CONV_2D) refuse_side(oi, "a side operator that is not a Conv2D");
                readers_behind(outs.get<int32_t>(0), oi, joins, others);
                if (!joins && others == 1) refuse_side(oi, "two or more operators on the skip edge");
                if (!joins && !others) refuse_side(oi, "its output is never read");
                if (joins != 1 || others) refuse_side(oi, "its output is read by something other than one ADD");
                if (pending_side >= 0 || t < last_join) refuse_side(oi, "a side operator while another skip is alive");
                for (const TensorInfo *ti : {&in, &out})
                    if ((ti->type == TT_INT8 || ti->type == TT_UINT8) && (ti->type == TT_UINT8) != pm.u8) refuse_side(oi, "mixed element types");
                po.side_src = t;
                pending_side = (int)oi;
            } else if (in0 != prev_index && !same_tensor(in.shape, prev_shape)) {
                refuse_side(oi, "its input is no tensor of the chain");
            }
        }
        if (!po.side()) {
            prev_index = outs.get<int32_t>(0);
            prev_shape = out.shape;
        }

        switch (code) {
        case MF_OP_FULLY_CONNECTED: { // microflow-macros/src/ops/fully_connected.rs:66-98
            require_elem(in, "FullyConnected", pm.u8), require_elem(out, "FullyConnected", pm.u8);
            if (ins.size() < 3) fail(MF_ERR_INVALID_MODEL, "invalid model: FullyConnected needs 3 inputs");
            TensorInfo w = read_tensor(tensors, buffers, ins.get<int32_t>(1));
            TensorInfo b = read_tensor(tensors, buffers, ins.get<int32_t>(2));
            fix_rank1(in), fix_rank1(out), fix_rank1(w), fix_rank1(b);
            need_quant(in, "FullyConnected input"), need_quant(out, "FullyConnected output");
            need_quant(w, "FullyConnected weights"), need_quant(b, "FullyConnected bias");
            if (w.shape.size() != 2 || w.type != (pm.u8 ? TT_UINT8 : TT_INT8) || b.type != TT_INT32)
                fail(MF_ERR_UNSUPPORTED, "FullyConnected: unsupported weights/bias tensors");
            po.N = w.shape[0];
            po.K = w.shape[1];
            po.M = in.shape[0];
            if (in.elems() != (size_t)po.M * po.K || w.data_len < (size_t)po.N * po.K ||
                b.data_len < (size_t)po.N * 4)
                fail(MF_ERR_INVALID_MODEL, "invalid model: FullyConnected shapes do not agree");
            set_shapes(po, in, out, pm.u8);
            po.out_elems = (size_t)po.M * po.N;
            po.act = check_act(opt.scalar<int8_t>(0, 0)); // FullyConnectedOptions { act:0 }
            po.weights.assign((const int8_t *)w.data, (const int8_t *)w.data + (size_t)po.N * po.K);
            po.wzp.assign(1, zp_of(w.zp[0], pm.u8));
            std::vector<int32_t> bias(po.N);
            std::memcpy(bias.data(), b.data, (size_t)po.N * 4);
            po.c0.resize(po.N), po.c1.resize(1), po.c2.resize(po.N);
            h_preprocess_fc(in.scale[0], zp_of(in.zp[0], pm.u8), in.shape[1], po.weights.data(), pm.u8, po.K, po.N,
                            w.scale[0], zp_of(w.zp[0], pm.u8), bias.data(), b.scale[0], (int32_t)b.zp[0],
                            out.scale[0], po.c0.data(), po.c1.data(), po.c2.data(), &po.c3);
            break;
        }
        case MF_OP_CONV_2D:             // microflow-macros/src/ops/conv_2d.rs:58-83
        case MF_OP_DEPTHWISE_CONV_2D: { // microflow-macros/src/ops/depthwise_conv_2d.rs:62-89
            const bool dw = code == MF_OP_DEPTHWISE_CONV_2D;
            const char *nm = dw ? "DepthwiseConv2D" : "Conv2D";
            require_elem(in, nm, pm.u8), require_elem(out, nm, pm.u8);
            if (ins.size() < 3) fail(MF_ERR_INVALID_MODEL, std::string("invalid model: ") + nm + " needs 3 inputs");
            TensorInfo w = read_tensor(tensors, buffers, ins.get<int32_t>(1));
            TensorInfo b = read_tensor(tensors, buffers, ins.get<int32_t>(2));
            fix_rank1(b);
            need_quant(in, nm), need_quant(out, nm), need_quant(w, nm), need_quant(b, nm);
            if (in.shape.size() != 4 || out.shape.size() != 4 || w.shape.size() != 4 || w.type != (pm.u8 ? TT_UINT8 : TT_INT8) ||
                b.type != TT_INT32)
                fail(MF_ERR_UNSUPPORTED, std::string(nm) + ": unsupported tensors");
            if (in.shape[0] != 1 || out.shape[0] != 1) // src/ops/conv_2d.rs:40,49 hard-code batch 1
                fail(MF_ERR_UNSUPPORTED, std::string(nm) + ": tensor batch must be 1 (independent inferences are batched by the caller)");
            set_shapes(po, in, out, pm.u8);
            po.H = in.shape[1], po.W = in.shape[2], po.C = in.shape[3];
            po.KH = w.shape[1], po.KW = w.shape[2];
            po.OH = out.shape[1], po.OW = out.shape[2];
            // Conv2DOptions { padding:0 stride_w:1 stride_h:2 act:3 }
            // DepthwiseConv2DOptions { padding:0 stride_w:1 stride_h:2 depth_multiplier:3 act:4 }
            po.pad = check_pad(opt.scalar<int8_t>(0, 0));
            po.sw = opt.scalar<int32_t>(1, 0);
            po.sh = opt.scalar<int32_t>(2, 0);
            po.act = check_act(opt.scalar<int8_t>(dw ? 4 : 3, 0));
            if (po.sh <= 0 || po.sw <= 0) fail(MF_ERR_INVALID_MODEL, "invalid model: bad strides");
            if (dw) {
                if (w.shape[0] != 1) fail(MF_ERR_INVALID_MODEL, "invalid model: depthwise weights batch != 1");
                po.N = w.shape[3];
            } else {
                po.N = w.shape[0];
                if (w.shape[3] != po.C) fail(MF_ERR_INVALID_MODEL, "invalid model: Conv2D channel mismatch");
            }
            if (out.shape[3] != po.N) fail(MF_ERR_INVALID_MODEL, std::string("invalid model: ") + nm + " output channels");
            if (w.data_len < w.elems() || b.data_len < (size_t)po.N * 4)
                fail(MF_ERR_INVALID_MODEL, "invalid model: short weight buffer");
            po.weights.assign((const int8_t *)w.data, (const int8_t *)w.data + w.elems());
            for (int64_t z : w.zp) po.wzp.push_back(zp_of(z, pm.u8));
            std::vector<int32_t> bias(po.N);
            std::memcpy(bias.data(), b.data, (size_t)po.N * 4);
            std::vector<int32_t> bzp;
            for (int64_t z : b.zp) bzp.push_back((int32_t)z);
            po.c0.resize(po.N), po.c1.resize(w.scale.size());
            h_preprocess_conv(in.scale[0], po.N, bias.data(), b.scale.data(), (int)b.scale.size(), bzp.data(),
                              (int)bzp.size(), w.scale.data(), (int)w.scale.size(), out.scale[0], po.c0.data(),
                              po.c1.data());
            break;
        }
        case MF_OP_AVERAGE_POOL_2D:  // microflow-macros/src/ops/average_pool_2d.rs:47-66
        case MF_OP_MAX_POOL_2D: {    // (not in the reference: the same options table, checks and constants; include/microflow_amd.h)
            const char *nm = code == MF_OP_MAX_POOL_2D ? "MaxPool2D" : "AveragePool2D";
            require_elem(in, nm, pm.u8), require_elem(out, nm, pm.u8);
            need_quant(in, nm), need_quant(out, nm);
            if (in.shape.size() != 4 || out.shape.size() != 4)
                fail(MF_ERR_UNSUPPORTED, std::string(nm) + ": unsupported tensors");
            if (in.shape[0] != 1 || out.shape[0] != 1)
                fail(MF_ERR_UNSUPPORTED, std::string(nm) + ": tensor batch must be 1");
            set_shapes(po, in, out, pm.u8);
            po.H = in.shape[1], po.W = in.shape[2], po.C = in.shape[3], po.N = po.C;
            po.OH = out.shape[1], po.OW = out.shape[2];
            // Pool2DOptions { padding:0 stride_w:1 stride_h:2 filter_width:3 filter_height:4 act:5 }
            po.pad = check_pad(opt.scalar<int8_t>(0, 0));
            po.sw = opt.scalar<int32_t>(1, 0);
            po.sh = opt.scalar<int32_t>(2, 0);
            po.KW = opt.scalar<int32_t>(3, 0);
            po.KH = opt.scalar<int32_t>(4, 0);
            po.act = check_act(opt.scalar<int8_t>(5, 0));
            if (po.sh <= 0 || po.sw <= 0 || po.KH <= 0 || po.KW <= 0)
                fail(MF_ERR_INVALID_MODEL, "invalid model: bad pool geometry");
            if (out.shape[3] != po.C) fail(MF_ERR_INVALID_MODEL, "invalid model: pool channels");
            if (code == MF_OP_MAX_POOL_2D && (po.H <= 0 || po.W <= 0 || po.OH <= 0 || po.OW <= 0 ||
                                              h_pool_window_empty(po.H, po.W, po.KH, po.KW, po.sh, po.sw, po.pad == MF_PAD_SAME, po.OH, po.OW)))
                fail(MF_ERR_INVALID_MODEL, "invalid model: a MaxPool2D window has no in-bounds tap");
            po.c0.resize(1), po.c1.resize(1);
            h_preprocess_pool(in.scale[0], zp_of(in.zp[0], pm.u8), out.scale[0], zp_of(out.zp[0], pm.u8), po.c0.data(),
                              po.c1.data());
            break;
        }
        case MF_OP_SOFTMAX: { // microflow-macros/src/ops/softmax.rs:20-49
            require_elem(in, "Softmax", pm.u8), require_elem(out, "Softmax", pm.u8);
            fix_rank1(in), fix_rank1(out);
            need_quant(in, "Softmax"), need_quant(out, "Softmax");
            if (out.shape.size() != 2) fail(MF_ERR_UNSUPPORTED, "Softmax: output tensor must have rank 2");
            set_shapes(po, in, out, pm.u8);
            po.M = out.shape[0], po.N = out.shape[1];
            if (in.elems() != out.elems()) fail(MF_ERR_INVALID_MODEL, "invalid model: softmax shapes");
            break;
        }
        case MF_OP_RESHAPE: { // microflow-macros/src/ops/reshape.rs:33-60
            if (out.shape.size() != 2 && out.shape.size() != 4)
                fail(MF_ERR_UNSUPPORTED, "Reshape supports only output tensor ranks 2 and 4, got rank " +
                                             std::to_string(out.shape.size()));
            set_shapes(po, in, out, pm.u8);
            if (in.elems() != out.elems()) fail(MF_ERR_INVALID_MODEL, "invalid model: reshape changes size");
            break;
        }
        case MF_OP_ADD: { // not in the reference (lib.rs:148 answers "unsupported operator: 0"): the contract is include/microflow_amd.h's
            // The graphs that load are chains with skip edges: the ADD reads the running value (in either position) and ONE earlier
            // tensor of the chain, matched by tensor index; at most one such tensor is alive at a time.  Everything else keeps the
            // reference's answer, with the reason behind it
            auto refuse = [](const std::string &why) { fail(MF_ERR_UNSUPPORTED, "unsupported operator: 0 (ADD: " + why + ")"); };
            parse_join(po, oi, ins, in, out, running_index, "ADD", refuse, "it needs two inputs", false, [&](const TensorInfo &tb) {
                if (in.shape != tb.shape || in.shape != out.shape) refuse("differing shapes (no broadcasting)");
                if (in.shape.size() != 2 && in.shape.size() != 4) refuse("tensor rank must be 2 or 4");
                if (in.shape.size() == 4 && in.shape[0] != 1) refuse("tensor batch must be 1");
                po.act = check_act(opt.scalar<int8_t>(0, 0)); // AddOptions { act:0 pot_scale_int16:1 (ignored) }
                po.c0.resize(1), po.c1.resize(1);
                h_preprocess_add(po.a_scale, po.b_scale, out.scale[0], po.c0.data(), po.c1.data());
            });
            break;
        }
        case MF_OP_CONCATENATION: { // not in the reference (lib.rs:148 answers "unsupported operator: 2"): the contract is include/microflow_amd.h's
            // A second kind of join beside ADD, in the same graph form: it reads the running value (in either position) and ONE other
            // tensor -- an earlier tensor of the chain or the side operator's output -- along the last axis
            auto refuse = [](const std::string &why) { fail(MF_ERR_UNSUPPORTED, "unsupported operator: 2 (CONCATENATION: " + why + ")"); };
            if (ins.size() != 2) refuse("it needs exactly two inputs"); // (ahead of every other refusal, unlike ADD's)
            // ConcatenationOptions { axis:0 fused_activation_function:1 }
            const bool fused_act = opt.scalar<int8_t>(1, 0) != MF_ACT_NONE;
            parse_join(po, oi, ins, in, out, running_index, "CONCATENATION", refuse, "it needs exactly two inputs", fused_act, [&](const TensorInfo &tb) {
                const size_t rank = in.shape.size();
                if (rank < 2 || rank > 4 || tb.shape.size() != rank || out.shape.size() != rank) refuse("tensor rank must be 2 to 4, the same for all");
                int axis = opt.scalar<int32_t>(0, 0);
                if (axis < 0) axis += (int)rank;
                if (axis != (int)rank - 1) refuse("an axis other than the last");
                size_t rows = 1;
                for (size_t d = 0; d + 1 < rank; ++d) {
                    if (in.shape[d] != tb.shape[d]) refuse("the inputs differ in another dimension than the axis");
                    rows *= (size_t)in.shape[d];
                }
                if (rank > 2 && in.shape[0] != 1) refuse("tensor batch must be 1");
                const int Ca = in.shape[rank - 1], Cb = tb.shape[rank - 1];
                if (Ca <= 0 || Cb <= 0 || !rows) fail(MF_ERR_INVALID_MODEL, "invalid model: bad tensor dimension");
                for (size_t d = 0; d < rank; ++d)
                    if ((int64_t)out.shape[d] != (d + 1 < rank ? (int64_t)in.shape[d] : (int64_t)Ca + Cb))
                        fail(MF_ERR_INVALID_MODEL, "invalid model: CONCATENATION output shape is not the two inputs joined");
                po.act = MF_ACT_NONE;
                po.cat_rows = rows, po.cat_ca = Ca, po.cat_cb = Cb, po.N = Ca + Cb;
                po.c0.resize(1), po.c1.resize(1);
                h_preprocess_concatenation(po.a_scale, po.b_scale, out.scale[0], po.c0.data(), po.c1.data());
                const int out_zp = zp_of(out.zp[0], pm.u8);
                po.cat_copy_a = h_concat_identity(po.a_scale, po.a_zp, out.scale[0], out_zp, po.c0[0]);
                po.cat_copy_b = h_concat_identity(po.b_scale, po.b_zp, out.scale[0], out_zp, po.c1[0]);
            });
            break;
        }
        case MF_OP_PAD: { // not in the reference (lib.rs:148 answers "unsupported operator: 34"): the contract is include/microflow_amd.h's
            auto refuse = [](const std::string &why) { fail(MF_ERR_UNSUPPORTED, "unsupported operator: 34 (PAD: " + why + ")"); };
            if (ins.size() != 2) refuse("it needs an input and a paddings operand");
            for (const TensorInfo *t : {&in, &out}) {
                if ((t->type != TT_INT8 && t->type != TT_UINT8) || (t->type == TT_UINT8) != pm.u8) refuse("mixed element types");
                need_quant(*t, "PAD");
                if (t->scale.size() != 1 || t->zp.size() != 1) refuse("per-channel quantisation on an operand");
            }
            if (in.data_len) refuse("a constant operand");
            if (in.shape.size() != 4 || out.shape.size() != 4) refuse("tensor rank must be 4");
            if (in.shape[0] != 1) refuse("tensor batch must be 1");
            const TensorInfo pd = read_tensor(tensors, buffers, ins.get<int32_t>(1));
            if (!pd.data_len) refuse("the paddings operand is not constant");
            if (pd.type != TT_INT32 && pd.type != TT_INT64) refuse("the paddings operand must be INT32 or INT64");
            if (pd.shape != std::vector<int>{4, 2}) refuse("the paddings operand must have shape [4, 2]");
            const size_t esz = pd.type == TT_INT64 ? 8 : 4;
            if (pd.data_len < 8 * esz) fail(MF_ERR_INVALID_MODEL, "invalid model: short PAD paddings buffer");
            int64_t pv[8];
            for (int k = 0; k < 8; ++k) {
                if (esz == 8) {
                    std::memcpy(&pv[k], pd.data + 8 * k, 8);
                } else {
                    int32_t v;
                    std::memcpy(&v, pd.data + 4 * k, 4);
                    pv[k] = v;
                }
                if (pv[k] < 0) fail(MF_ERR_INVALID_MODEL, "invalid model: PAD with a negative pad");
                if (pv[k] > (1 << 24)) fail(MF_ERR_INVALID_MODEL, "invalid model: bad tensor dimension");
            }
            if (pv[0] || pv[1] || pv[6] || pv[7]) refuse("a batch or channel pad");
            if (std::memcmp(&in.scale[0], &out.scale[0], sizeof(float)) != 0 || zp_of(in.zp[0], pm.u8) != zp_of(out.zp[0], pm.u8))
                refuse("input and output quantisation differ");
            for (int d = 0; d < 4; ++d)
                if ((int64_t)out.shape[(size_t)d] != (int64_t)in.shape[(size_t)d] + pv[2 * d] + pv[2 * d + 1])
                    fail(MF_ERR_INVALID_MODEL, "invalid model: PAD output shape is not input + pads");
            set_shapes(po, in, out, pm.u8);
            po.H = in.shape[1], po.W = in.shape[2], po.C = in.shape[3], po.N = po.C;
            po.OH = out.shape[1], po.OW = out.shape[2];
            for (int k = 0; k < 4; ++k) po.pads[k] = (int)pv[2 + k]; // top, bottom, left, right
            break;
        }
        case MF_OP_MEAN: { // not in the reference: over axes {1, 2} it is the reference's average_pool_2d over the whole image
            // (include/microflow_amd.h), and is parsed into that operator: every rule that matches a global AveragePool2D sees one
            auto refuse = [](const std::string &why) { fail(MF_ERR_UNSUPPORTED, "unsupported operator: 40 (MEAN: " + why + ")"); };
            if (ins.size() != 2) refuse("it needs an input and an axes operand");
            require_elem(in, "MEAN", pm.u8), require_elem(out, "MEAN", pm.u8);
            need_quant(in, "MEAN"), need_quant(out, "MEAN");
            if (in.shape.size() != 4) refuse("tensor rank must be 4");
            if (in.shape[0] != 1) refuse("tensor batch must be 1");
            const TensorInfo ax = read_tensor(tensors, buffers, ins.get<int32_t>(1));
            if (!ax.data_len) refuse("the axes operand is not constant");
            if (ax.type != TT_INT32) refuse("the axes operand must be INT32");
            const size_t na = ax.elems();
            if (!na || ax.data_len < na * 4) fail(MF_ERR_INVALID_MODEL, "invalid model: short MEAN axes buffer");
            unsigned named = 0;
            for (size_t k = 0; k < na; ++k) {
                int32_t a;
                std::memcpy(&a, ax.data + 4 * k, 4);
                if (a < 0) a += 4;
                if (a != 1 && a != 2) refuse("axes other than {1, 2}");
                named |= 1u << a;
            }
            if (named != 6u) refuse("axes other than {1, 2}");
            const bool keep = opt.scalar<uint8_t>(0, 0) != 0; // ReducerOptions { keep_dims:0 }
            const int C = in.shape[3];
            if (out.shape != (keep ? std::vector<int>{1, 1, 1, C} : std::vector<int>{1, C}))
                fail(MF_ERR_INVALID_MODEL, "invalid model: MEAN output shape does not follow from the axes and keep_dims");
            set_shapes(po, in, out, pm.u8);
            po.kind = MF_OP_AVERAGE_POOL_2D, po.file_kind = MF_OP_MEAN;
            po.H = in.shape[1], po.W = in.shape[2], po.C = C, po.N = C;
            po.KH = po.H, po.KW = po.W, po.sh = po.sw = 1, po.pad = MF_PAD_VALID, po.act = MF_ACT_NONE;
            po.OH = po.OW = 1;
            po.c0.resize(1), po.c1.resize(1);
            h_preprocess_pool(in.scale[0], zp_of(in.zp[0], pm.u8), out.scale[0], zp_of(out.zp[0], pm.u8), po.c0.data(),
                              po.c1.data());
            break;
        }
        case BUILTIN_PADV2:
            fail(MF_ERR_UNSUPPORTED, "unsupported operator: 60 (PADV2: only PAD, whose fill is the tensor's zero point, is supported)");
        case BUILTIN_MIRROR_PAD:
            fail(MF_ERR_UNSUPPORTED, "unsupported operator: 100 (MIRROR_PAD: reflect / symmetric padding is not supported)");
        default:
            fail(MF_ERR_UNSUPPORTED, "unsupported operator: " + std::to_string(code)); // lib.rs:148
        }
        out_index.push_back(outs.get<int32_t>(0));
        if (po.out_elems > pm.max_elems) pm.max_elems = po.out_elems;
        if (po.in_elems > pm.max_elems) pm.max_elems = po.in_elems;
        pm.ops.push_back(std::move(po));
    }
    {
        std::vector<int> gout(pm.out_shape, pm.out_shape + pm.out_rank);
        if (!operators.size() || (prev_index != g_out.get<int32_t>(0) && !same_tensor(prev_shape, gout)))
            fail(MF_ERR_UNSUPPORTED, "the model output is not the last operator's output: only linear operator "
                                     "chains are supported");
    }
    return pm;
}

} // namespace mf
