// mf_internal.hpp -- internal declarations of libmicroflow_amd.so (not part of the ABI).
//
// Layering:
//   capi.cpp      extern "C" boundary (include/microflow_amd.h), error translation
//   model.cpp     .tflite -> ParsedModel -> prepared device ops -> launch sequence
//   model_groups.cpp   the grouping rules: which operators run as one launch (model_groups.hpp: ModelGroups, the owner of all three tiers)
//   tflite.cpp    minimal FlatBuffers reader for the ~10 TFLite tables the path needs
//   hostmath.cpp  f32 constant preparation in the reference's evaluation order
//   ops.hip       prepared operators: constant folding, kernel routing (one function per route), launches
//   fused.hip     fused groups of prepared operators as one launch: destroy / name / mode, f32 edges, the launch path
//   fused_pairs.hip, fused_heads.hip, fused_stages.hip   the groups' builders, by family (fused_impl.hpp: the group, shared helpers)
//   chain_partition.hip   the chain planner / autotuner
//   wimage.cpp    every operand layout the host builds for the kernels (host only: tests/test_wimage_host.py)
//   ops_impl.hpp  what ops.hip and the fused units share (OpImpl, DevBuf)
//   k_*.hip       the HIP kernels (gfx950), one file per family; k_common.hpp shared helpers
#pragma once
#include "mf_switches.hpp"
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/microflow_amd.h"
#include "windows_spec.hpp"

namespace mf {

struct Error {
    int code;
    std::string msg;
};
[[noreturn]] void fail(int code, const std::string &msg);
void set_last_error(const std::string &msg);

// ---- host numerics (hostmath.cpp) --------------------------------------
// All individually rounded f32 operations; this translation unit is compiled
// with -ffp-contract=off.
float h_roundf(float x);                              // round half away from zero
float h_expf(float x);                                // libm 0.2 (musl-derived) expf
void h_softmax_table(float in_scale, bool u8, float *table256); // expf over the 256 possible Softmax inputs
int8_t h_sat_i8(float x);                             // Rust `as i8`
int8_t h_quantize(float x, float scale, int8_t zp);   // src/quantize.rs:16-18
int h_quantize_t(float x, float scale, int zp, bool u8); // either element type
void h_preprocess_fc(float iscale, int izp, int in_shape1, const int8_t *w, bool u8, int K, int N,
                     float wscale, int wzp, const int32_t *bias, float bscale, int32_t bzp,
                     float oscale, float *c0, float *c1, int32_t *c2, int32_t *c3);
void h_preprocess_conv(float iscale, int n, const int32_t *bias, const float *bscale, int nbs,
                       const int32_t *bzp, int nbz, const float *fscale, int nfq, float oscale,
                       float *c0, float *c1);
void h_preprocess_pool(float iscale, int izp, float oscale, int ozp, float *c0, float *c1);
// true: some window of this (positive) pool geometry has no in-bounds tap -- MaxPool2D refuses it
bool h_pool_window_empty(int H, int W, int KH, int KW, int sh, int sw, bool same, int OH, int OW);
// ADD (not in the reference; include/microflow_amd.h states the contract): ca = sa / so, cb = sb / so, two f32 divisions
void h_preprocess_add(float sa, float sb, float so, float *ca, float *cb);
// CONCATENATION (not in the reference; include/microflow_amd.h states the contract): the same two divisions
void h_preprocess_concatenation(float sa, float sb, float so, float *ca, float *cb);
// ... and whether input i's slice is the identity of that contract: its scale bit-equal to the output's, equal zero points, c == 1.0f
bool h_concat_identity(float s_i, int z_i, float so, int zo, float c);
// ADD's gated form y = fma(cb, f32(ub), fma(ca, f32(ua), k1)) with k1 = zo - ca ka - cb kb (ua, ub: bytes 0 .. 255 whose values are
// ua - ka, ub - kb).  true, with *k1: the constants are finite and the form gives the text's byte -- through the same rounding and
// the clamp [lo, hi] -- for ALL 65 536 (ua, ub) pairs.  Host only, exhaustive
bool h_add_fma_form(float ca, float cb, int ka, int kb, int zo, int lo, int hi, float *k1);

// ---- single-fma requantisation: host search (epi_fma.cpp) -------------------
// y_u8(acc) = v_cvt_pk_u8_f32(v_fma_f32(S, bits_as_f32(0x4B400000 + acc + d), C))  -- k_common.hpp, epilogue mode 3
struct FmaForm {
    float S = 0, C = 0;
    int32_t d = 0;
    // at most ONE accumulator per channel is replaced by its neighbour before the fma (patch_delta = +-1; 0: none): the reference's
    // own roundings can put a single step one accumulator off every line (epi_fma.cpp)
    int64_t patch_acc = 0;
    int32_t patch_delta = 0;
};
struct FmaSearchStats {
    int steps = 0;            // steps of the reference staircase inside the reachable accumulator range
    int s_candidates = 0;     // f32 neighbours of S with a non-empty real-arithmetic window
    int s_rank = -1;          // which of them (by window width) gave the solution
    double best_width = 0;    // widest window
    long long pivots_tried = 0, exact_checks = 0;
};
// off: 128 (i8: the form works in the u8 domain, results are XOR-ed back) or 0 (u8); [lo, hi]: the clamp in T's domain;
// [amin, amax]: the accumulators this channel can produce (inside (-2^22, 2^22)).  false: no (S', C', d) reproduces the reference on it.
bool fma_form_search(float A, float S, int off, int lo, int hi, int64_t amin, int64_t amax, FmaForm &out, FmaSearchStats *stats = nullptr,
                     bool allow_patch = false);
int ref_form_eval(float A, float S, int off, int lo, int hi, int64_t acc); // the reference's tail, u8 domain
int fma_form_eval(const FmaForm &f, int64_t acc);                          // the device's instructions, emulated exactly
uint64_t fma_form_mismatches(float A, float S, int off, int lo, int hi, int64_t amin, int64_t amax, const FmaForm &f); // exhaustive, host

// ---- parsed model (tflite.cpp) -------------------------------------------
struct ParsedOp {
    int kind = 0;
    int in_rank = 0, in_shape[4] = {0, 0, 0, 0};
    int out_rank = 0, out_shape[4] = {0, 0, 0, 0};
    int KH = 0, KW = 0, sh = 0, sw = 0, pad = 0, act = 0;
    float in_scale = 0, out_scale = 0;
    int in_zp = 0, out_zp = 0;
    size_t in_elems = 0, out_elems = 0;
    // geometry
    int H = 0, W = 0, C = 0; // conv/dw/pool input
    int N = 0;               // conv filters / dw channels / fc outputs / softmax cols
    int M = 0, K = 0;        // fc rows / depth; softmax rows = M
    int OH = 0, OW = 0;
    std::vector<int8_t> weights; // fc [N][K]; conv [N][KH][KW][C]; dw [KH][KW][N] (raw bytes of T)
    std::vector<int> wzp;        // weight zero points (1 or per channel), values of T
    std::vector<float> c0, c1;
    std::vector<int32_t> c2;
    int32_t c3 = 0;
    // A join only: the tensor beside the running one.  skip_src: the operator whose output it is (-1: the model input; -2: no join);
    // run_input: which of the join's two inputs (0 = a, 1 = b) the running tensor is; (a_*, b_*): the operands' quantisation by
    // input position, zero points as values of T.  c0[0] = ca, c1[0] = cb
    int skip_src = -2, run_input = 0;
    float a_scale = 0, b_scale = 0;
    int a_zp = 0, b_zp = 0;
    // A join: an ADD or a CONCATENATION -- the two operators that read the running tensor AND one other (skip_src, run_input, a_*, b_*
    // as above, for either).  CONCATENATION only: rows (the product of all axes but the last), the two inputs' last axes by input
    // position, and whether each slice's requantisation is the identity (h_concat_identity); in_elems is the running operand's
    bool join() const { return kind == MF_OP_ADD || kind == MF_OP_CONCATENATION; }
    size_t cat_rows = 0;
    int cat_ca = 0, cat_cb = 0;
    bool cat_copy_a = false, cat_copy_b = false;
    size_t skip_elems() const { return kind == MF_OP_CONCATENATION ? cat_rows * (size_t)(run_input == 0 ? cat_cb : cat_ca) : in_elems; } // the other operand's
    // A side operator only (one Conv2D on a skip edge: it reads an earlier tensor T of the chain, not the running value, and one later
    // join reads its output beside the running value): the operator whose output T is (-1: the model input); -2: no side operator.
    // That join's skip_src is this operator's index.  in_scale / in_zp are T's
    int side_src = -2;
    bool side() const { return side_src != -2; }
    // PAD only: new rows / columns (top, bottom, left, right); H, W, C the input, OH, OW the output
    int pads[4] = {0, 0, 0, 0};
    // what mf_model_get_op reports as the kind: the file's.  A MEAN over {1, 2} is parsed into a global AveragePool2D (kind), so that
    // every rule that matches one sees it, and reports MF_OP_MEAN; -1: kind
    int file_kind = -1;
};
struct ParsedModel {
    bool u8 = false; // element type T of every quantized tensor: INT8 (false) or UINT8 (true)
    int in_rank = 0, in_shape[4] = {0, 0, 0, 0};
    int out_rank = 0, out_shape[4] = {0, 0, 0, 0};
    float in_scale = 0, out_scale = 0;
    int in_zp = 0, out_zp = 0;
    size_t in_elems = 0, out_elems = 0, max_elems = 0;
    size_t max_fork_elems = 0; // the largest tensor an operator produces for a later join (ADD, CONCATENATION) to read beside the running one (0: none)
    bool input_skip = false;   // some join reads the model input beside the running tensor
    std::vector<ParsedOp> ops;
    // the operator that launches tensor s of the chain (-1: the model input): the Reshapes (aliases) in front of it skipped, and the
    // side operators that stand between them in file order passed over
    int launcher(int s) const {
        while (s >= 0 && ops[(size_t)s].kind == MF_OP_RESHAPE)
            do --s;
            while (s >= 0 && ops[(size_t)s].side());
        return s;
    }
    // the operator that launches the tensor that has to stay in memory for join i (an ADD or a CONCATENATION): the one it reads beside the running one or, where
    // that is a side operator's output, the tensor T the side operator reads; -1: the model input
    int skip_real(size_t i) const {
        int s = ops[i].skip_src;
        if (s >= 0 && ops[(size_t)s].side()) s = ops[(size_t)s].side_src;
        return launcher(s);
    }
    // join i (an ADD or a CONCATENATION) reads a side operator's output: that operator's index, else -1
    int side_of_join(size_t i) const {
        const int s = ops[i].join() ? ops[i].skip_src : -2;
        return s >= 0 && ops[(size_t)s].side() ? s : -1;
    }
};
ParsedModel parse_tflite(const uint8_t *buf, size_t len);

// ---- prepared device operator (ops.hip; the fused groups: fused.hip) ------------------------------------
struct OpImpl; // device buffers + kernel routing
struct OpSpec {
    int kind = 0;
    // Element type T.  With u8 = true the zero points (izp, ozp, wzp) are u8 values, `weights`
    // are raw u8 bytes, c2/c3 come from the u8 preprocess; activations are exchanged with the
    // operator in the INTERNAL i8 domain (byte ^ 0x80) -- see kernels.hpp.
    bool u8 = false;
    int M = 0, K = 0, N = 0;
    int H = 0, W = 0, C = 0, KH = 0, KW = 0, sh = 1, sw = 1, pad = 0, OH = 0, OW = 0;
    int act = 0;
    int izp = 0;             // zero point of the running input tensor
    float in_scale = 0;      // softmax only
    float oscale = 0;
    int ozp = 0;
    const int8_t *weights = nullptr;
    const int *wzp = nullptr;
    int nq = 0;
    const float *c0 = nullptr;
    const float *c1 = nullptr;
    int nc1 = 0;
    const int32_t *c2 = nullptr;
    int32_t c3 = 0;
    float pool_c0 = 0, pool_c1 = 0;
    // a join (ADD, CONCATENATION): the operands' zero points (values of T) and the two constants, by input position
    int join_za = 0, join_zb = 0;
    float join_ca = 0, join_cb = 0;
    // ADD: elements per inference
    size_t add_elems = 0;
    // CONCATENATION: rows per inference, the inputs' last axes, whether a slice is copied (h_concat_identity)
    size_t cat_rows = 0;
    int cat_ca = 0, cat_cb = 0;
    bool cat_copy_a = false, cat_copy_b = false;
    // PAD only: new rows / columns (top, bottom, left, right) around the H x W x C image, each element izp; OH, OW the padded size.
    // (A convolution's spec carries SAME / VALID and nothing else: explicit pads exist only inside the PAD + convolution group)
    int pads[4] = {0, 0, 0, 0};
};
OpImpl *op_create(int device, const OpSpec &spec);
void op_destroy(OpImpl *op);
void op_run(OpImpl *op, const int8_t *d_in, size_t batch, int8_t *d_out, void *stream);
// an ADD: out = a + b over batch x elems bytes.  d_out may be exactly d_a or exactly d_b (in place); any other overlap is refused.
// a CONCATENATION: batch x rows rows of Ca + Cb bytes; the output overlaps neither input.
// external: a u8 operator exchanges real u8 bytes (the ABI's view, in the same launch), else the internal domain
void op_run2(OpImpl *op, const int8_t *d_a, const int8_t *d_b, size_t batch, int8_t *d_out, void *stream, bool external);
// the ABI's view: a u8 operator exchanges real u8 bytes (two extra byte passes)
void op_run_external(OpImpl *op, const int8_t *d_in, size_t batch, int8_t *d_out, void *stream);
size_t op_in_elems(const OpImpl *op);
size_t op_in2_elems(const OpImpl *op); // the second input of an ADD or a CONCATENATION; 0 otherwise
size_t op_out_elems(const OpImpl *op);
const char *op_kernel_name(const OpImpl *op);
int op_epilogue_mode(const OpImpl *op); // k_common.hpp epilogue mode (0 .. 3) of the operator's own launch; -1: no requantising epilogue of that kind
bool op_has_fma_epilogue(const OpImpl *op);
int op_fma_patches(const OpImpl *op); // patched accumulators of the operator's single-fma form (0 for most); -1: no such form // the single-fma form (mode 3) was found for every channel and confirmed on the device
void op_set_generic(OpImpl *op, bool generic);
// fuse the model-boundary quantize (f32 -> T) into this operator if it has an f32-input kernel
bool op_set_input_quant(OpImpl *op, float scale, int zp, bool u8);
bool op_accepts_f32(const OpImpl *op);
// ... and the mirror image: the model-boundary dequantize (T -> f32, the scale and zero point the operator stamped) inside this
// operator's launch if it has an f32-output kernel
bool op_set_output_dequant(OpImpl *op, float scale, int zp, bool u8);
bool op_emits_f32(const OpImpl *op);
// the operator's launch with one or both ends in f32: d_in is batch x in_elems floats (16-byte aligned) when in_f32, d_out
// batch x out_elems floats when out_f32; the other end as op_run's
void op_run_f32(OpImpl *op, const void *d_in, bool in_f32, size_t batch, void *d_out, bool out_f32, void *stream);
// kernel launches (and device-side fills and copies) this host thread has enqueued through the library so far; the model runtime adds
// its own device-to-device copies
unsigned long long &dev_launch_counter();
// fused DepthwiseConv2D 3x3 -> Conv2D 1x1 (borrows both operators' device buffers; nullptr when
// the pair has no fused kernel)
struct FusedImpl;
FusedImpl *fused_create(OpImpl *dw, OpImpl *pw);
FusedImpl *fused_block_create(OpImpl *expand, OpImpl *dw, OpImpl *pw, bool pair_grouped = false); // a 1x1 expand + depthwise 3x3 + 1x1 project block in one launch (k_block_band.hip), or nullptr; pair_grouped: the last two have a launch of their own
// a 1x1 Conv2D on a skip edge + the ADD that reads its result beside the running tensor as one shortcut_add_rt launch
// (k_side_join.hip), or nullptr: outside the class, the two run their own launches.  conv_first: the ADD's input a is the
// convolution's result.  fused_run2 runs it: d_t the convolution's input, d_run the running tensor; d_out may be exactly d_run
FusedImpl *fused_shortcut_add_create(OpImpl *conv, OpImpl *add, bool conv_first);
// ... and its sibling for a CONCATENATION join: a 1x1 Conv2D on a skip edge + the CONCATENATION of its result and the running tensor as
// one side_concat_rt launch (k_side_join.hip), or nullptr.  fused_run2 runs it; d_out overlaps neither input
FusedImpl *fused_side_concat_create(OpImpl *conv, OpImpl *cat, bool conv_first);
void fused_run2(FusedImpl *f, const int8_t *d_t, const int8_t *d_run, size_t batch, int8_t *d_out, void *stream);
// a PAD + the VALID Conv2D / DepthwiseConv2D on its output as ONE launch of the kernel the convolution, taken as an operator on the
// unpadded image with the PAD's top / left pads, gets from the run-time-geometry planners (conv_rows, conv_mm / dw_mm, dw_gemm, conv_gemm);
// nullptr: no planner accepts (or the class is excluded) and the two launches stay
FusedImpl *fused_pad_conv_create(OpImpl *pad, OpImpl *conv);
// the convolution `conv` (VALID, on the padded H x W) as an operator on the unpadded Hin x Win image whose windows start padt rows above
// and padl columns left of it, everything outside the image reading the input zero point; OH, OW stay.  It borrows conv's weights and
// constants (destroy it first), has a matrix-pipe / row kernel or does not exist (nullptr), and must only be run on 16-byte aligned pointers
OpImpl *op_create_padded_conv(const OpImpl *conv, int Hin, int Win, int padt, int padl);
FusedImpl *fused_conv_pool_create(OpImpl *conv, OpImpl *pool); // a Conv2D + the AveragePool2D (k_conv_pool.hip) or MaxPool2D (k_conv_maxpool.hip) with more than one output pixel on its output in one launch, or nullptr
// fused tail: AveragePool2D (1x1 output) -> Conv2D 1x1 (N <= 8) -> Softmax (one row of N)
FusedImpl *fused_tail_create(OpImpl *pool, OpImpl *conv, OpImpl *softmax);
// fused FullyConnected (row-wave kernel, one row per inference) -> Softmax over its outputs
FusedImpl *fused_fc_softmax_create(OpImpl *fc, OpImpl *softmax);
// consecutive FullyConnected operators (+ a Softmax over one row: sm, or nullptr) as one fc_chain launch (k_fc_rt.hip)
bool fused_fc_chain_fits(OpImpl *const *fcs, int n, OpImpl *sm);
FusedImpl *fused_fc_chain_create(OpImpl *const *fcs, int n, OpImpl *sm);
// the global AveragePool2D + the FullyConnected operators behind it (+ a Softmax over one row: sm, or nullptr) as one pool_fc_chain
// launch (k_pool_fc.hip; second level: a fc_rowwave_softmax group inside it stays for run_until pieces)
bool fused_pool_fc_fits(OpImpl *pool, OpImpl *const *fcs, int n, OpImpl *sm);
FusedImpl *fused_pool_fc_create(OpImpl *pool, OpImpl *const *fcs, int n, OpImpl *sm);
// a DepthwiseConv2D / Conv2D with one input channel + the FullyConnected behind it (+ a Softmax over one row: sm, or nullptr) as one
// conv1_fc_rt launch (k_conv1_fc.hip; second level: the operators and a fc_rowwave_softmax group inside it stay for run_until pieces)
bool fused_conv1_fc_fits(OpImpl *conv, OpImpl *fc, OpImpl *sm);
FusedImpl *fused_conv1_fc_create(OpImpl *conv, OpImpl *fc, OpImpl *sm);
// false: this launch cannot take the group's kernel on this input pointer (pool_fc_chain loads 16-byte words) and the operators run
// their own launches, as op_run decides for a single operator
bool fused_input_ok(const FusedImpl *f, const int8_t *d_in);
// false: at this batch the group's launch measured slower than the operators' own, which run instead (conv1_fc_rt)
bool fused_batch_ok(const FusedImpl *f, size_t batch);
// a run of identical depthwise + pointwise pair groups as one persistent kernel (borrows their device buffers:
// destroy it before them); nullptr when no stage kernel exists for the shape / count
FusedImpl *fused_stage_create(FusedImpl *const *pairs, int npairs);
// one-input-channel DepthwiseConv2D + the FullyConnected/Softmax group as one kernel (second level, like the stage)
FusedImpl *fused_dwfc_create(OpImpl *dw, FusedImpl *fc_softmax);
// the last depthwise + pointwise pair group (3x3x256) + the pool/head/softmax tail group as one kernel (second level)
FusedImpl *fused_pair_tail_create(FusedImpl *pair, FusedImpl *tail);
// ... and the pair group in front of that pair in the same launch (6x6x128 stride 2 -> 3x3x256 + the above), or nullptr
FusedImpl *fused_front_pair_tail_create(FusedImpl *front_pair, FusedImpl *pair_tail);
FusedImpl *fused_chain_create(FusedImpl *const *single_pair_chains, int n, int force_G = 0); // consecutive run-time-geometry pairs as one launch (k_chain.hip); force_G: images per step (0: the planner's)
bool fused_is_chain_single(const FusedImpl *f);
void fused_chain_partition(FusedImpl *const *single_pair_chains, int n, int *seg_len, bool *unfused, int *seg_G, bool autotune); // seg_G[i]: measured images per step of the chain starting at i (0: the planner's); autotune: time the candidates on the device instead of using the cost model
FusedImpl *fused_quad_create(FusedImpl *pair1, FusedImpl *pair2); // two consecutive pairs in one launch (k_quad.hip)
FusedImpl *fused_quad_stem_create(OpImpl *stem, FusedImpl *quad); // the one-input-channel stem + a quad in one launch, or nullptr
void fused_destroy(FusedImpl *f);
void fused_run(FusedImpl *f, const int8_t *d_in, size_t batch, int8_t *d_out, void *stream);
// the model boundary inside a group's launch (as op_set_input_quant / op_set_output_dequant): false when its kernel has no such instance
bool fused_set_input_quant(FusedImpl *f, float scale, int zp, bool u8);
bool fused_set_output_dequant(FusedImpl *f, float scale, int zp, bool u8);
bool fused_accepts_f32(const FusedImpl *f);
bool fused_emits_f32(const FusedImpl *f);
void fused_run_f32(FusedImpl *f, const void *d_in, bool in_f32, size_t batch, void *d_out, bool out_f32, void *stream);
const char *fused_kernel_name(const FusedImpl *f);
int fused_epilogue_mode(const FusedImpl *f); // epilogue mode of the launch (one for all its requantising operators); -1: none

// zp is a value of T; with u8 the int8 buffer is in the internal domain (byte ^ 0x80)
void dev_quantize(int device, const float *d_in, size_t n, float scale, int zp, bool u8, int8_t *d_out,
                  void *stream);
void dev_dequantize(int device, const int8_t *d_in, size_t n, float scale, int zp, bool u8, float *d_out,
                    void *stream);
void dev_dequantize_u8_raw(int device, const uint8_t *d_in, size_t n, float scale, int zp, float *d_out,
                           void *stream); // real u8 bytes in
void dev_xor80(int device, const int8_t *d_in, size_t n, int8_t *d_out, void *stream);
// windows [first, first + count) of a validated description (windows_spec.hpp) as a dense batch at d_dst (k_windows.hip); flip80:
// every byte ^ 0x80 on the way (a u8 model's internal domain).  The quantising form evaluates dev_quantize's arithmetic per element;
// `fast`: quant_div's 3-instruction division, only where dev_quant_div_fast said so for (scale, zp, u8)
void dev_window_gather(int device, const void *d_src, const mf_windows &w, const WindowsGeom &g, size_t first, size_t count, bool flip80,
                       int8_t *d_dst, void *stream);
void dev_window_gather_quantize(int device, const float *d_src, const mf_windows &w, const WindowsGeom &g, size_t first, size_t count,
                                float scale, int zp, bool u8, bool fast, bool flip80, int8_t *d_dst, void *stream);
bool dev_quant_div_fast(int device, float scale, int zp, bool u8); // verified on the device once per parameter set and process
void dev_synth_i8(int device, uint64_t seed, uint64_t first, size_t n, int8_t *d_out, void *stream);
uint64_t dev_checksum_i8(int device, const int8_t *d_in, size_t n, void *stream);
// exhaustive check of the 3-instruction boundary-quantisation division (k_common.hpp: quant_div): mismatching bytes
uint64_t dev_verify_quant_div(int device, float scale, float rcp, int zp, bool u8);
uint64_t dev_selftest_epilogue(int device, int mode, bool u8, bool have_as, float A, float S, int lo, int hi);
// one channel of the single-fma epilogue on the device, every accumulator of [amin, amax] (k_generic.hip verify_fma_form): mismatches
uint64_t dev_selftest_fma_epilogue(int device, float A, float S, bool u8, int64_t amin, int64_t amax, float S3, float C3, int pivot,
                                   int64_t patch_acc = 0, int patch_delta = 0);
uint64_t dev_selftest_cvt_pk(int device);
int dev_count();
void dev_require(int device); // throws MF_ERR_NO_DEVICE

// ---- model runtime (model.cpp) ----------------------------------------------
struct ModelImpl;
ModelImpl *model_create(const uint8_t *buf, size_t len);
void model_destroy(ModelImpl *m);
const ParsedModel &model_parsed(const ModelImpl *m);
const char *model_op_kernel(const ModelImpl *m, int i);
int model_op_epilogue_mode(const ModelImpl *m, int i); // of the launch that starts at operator i: the minimum over its operators
void model_prepare(ModelImpl *m, int device, size_t max_batch);
void model_set_stream(ModelImpl *m, void *stream);
void model_sync(ModelImpl *m);
void model_set_generic(ModelImpl *m, bool generic);
void model_set_fusion(ModelImpl *m, bool enabled);
// before model_prepare: measure the run-time-geometry chain candidates at creation (chain_partition.hip fused_chain_partition) instead of planning from the cost model
void model_set_autotune(ModelImpl *m, bool enabled);
// replay the device-resident launch sequence as a hipGraph (captured on the 2nd identical call)
void model_set_graph(ModelImpl *m, bool enabled);
uint64_t model_graph_launches(const ModelImpl *m);
uint64_t model_device_ops(const ModelImpl *m); // kernel launches and device-side copies enqueued so far (a graph replay counts as one)
// in_f32 or in_i8 (exactly one non-null); out_f32 or out_i8 (exactly one non-null)
void model_run(ModelImpl *m, const float *in_f32, const int8_t *in_i8, size_t batch,
               float *out_f32, int8_t *out_i8, int mem, int last_op);
// model_run over windows [first, first + count) of a source (include/microflow_amd.h, section 5): src_f32 or src_i8 (exactly one
// non-null), out_f32 or out_i8 (exactly one non-null).  Validates before it looks at the device.
void model_run_windows(ModelImpl *m, const float *src_f32, const int8_t *src_i8, const mf_windows *w, size_t first, size_t count,
                       float *out_f32, int8_t *out_i8, int mem);
void model_set_window_chunk(ModelImpl *m, size_t windows);
void model_time_device(ModelImpl *m, const int8_t *d_in, size_t batch, int8_t *d_out, int warmup,
                       int iters, float *avg_ms, float *per_op_ms);

} // namespace mf
