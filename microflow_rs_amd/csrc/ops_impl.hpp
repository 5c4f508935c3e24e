// ops_impl.hpp -- what the operator unit (ops.hip) and the fused-group units (fused*.hip, chain_partition.hip) share: the prepared operator
// itself, its device buffers, the wrapping integer arithmetic of the folded constants.  Internal to those units.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "mf_internal.hpp"

namespace mf {

#define MF_HIP(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            fail(e_ == hipErrorOutOfMemory ? MF_ERR_OOM : MF_ERR_HIP,                         \
                 std::string(#call) + ": " + hipGetErrorString(e_));                          \
    } while (0)

inline int32_t wrap_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
inline int32_t wrap_sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
inline int32_t wrap_mul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    void upload(const void *src, size_t bytes) {
        if (p) {
            (void)hipFree(p);
            p = nullptr;
        }
        if (!bytes) return;
        MF_HIP(hipMalloc(&p, bytes));
        MF_HIP(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    }
    template <typename T> const T *as() const { return (const T *)p; }
};

// activation + `as T` saturation as one clamp [lo, hi] in T's domain  (src/activation.rs:21-34)
inline void act_bounds(int act, float oscale, int ozp, bool u8, int &lo, int &hi) {
    lo = u8 ? 0 : -128;
    hi = u8 ? 255 : 127;
    if (act == MF_ACT_RELU || act == MF_ACT_RELU6) lo = ozp;        // max(y, zero_point)
    if (act == MF_ACT_RELU6) hi = h_quantize_t(6.0f, oscale, ozp, u8); // min(.., quantize(6.0))
    if (lo > hi) lo = hi; // min(max(y, lo), hi) == hi for every y when lo > hi
}

// the halves of a launch's boundary block (kernels.hpp: F32Edge).  `zp` is a value of T.  The entry's 3-instruction division is used
// only where it was verified for these parameters over all 2^32 inputs on the device (ops.hip: a few ms, once per parameter set)
void edge_set_in(k::F32Edge &e, int device, float scale, int zp, bool u8);
void edge_set_out(k::F32Edge &e, float scale, int zp, bool u8);

struct OpImpl {
    int device = 0;
    OpSpec s; // pointers inside are NOT valid after create
    size_t in_elems = 0, out_elems = 0;
    bool force_generic = false;
    bool accepts_f32 = false;  // op_set_input_quant succeeded: op_run_f32 may replace quantize + op_run
    bool emits_f32 = false;    // op_set_output_dequant succeeded: op_run_f32 may replace op_run + dequantize
    k::F32Edge edge{};         // ... the boundary parameters of the kernels that take them as one block (fc_rt)
    bool finite_consts = true; // A / S all finite (the shape-specialised and fused epilogues assume it)
    std::string generic_name, fast_name;
    enum Fast { NONE, DW_NHWC, DW_STEM, DW_STEM_RT, DW_C1, PW_MFMA, FC_ROWWAVE, FC_MFMA, POOL_C4, CONV1X1_ROW, DW_RT, PW_RT, CONV_ROWS, CONV_MM, FC_RT,
                CONV_GEMM, DW_GEMM, FC_SPARSE24, MAXPOOL_C4, ADD_C16, PAD_C4, CONCAT_C4 } fast = NONE;
    int *d_rowsum = nullptr; // FC_MFMA / FC_SPARSE24 with wzp != 0: per-row input sums
    size_t rowsum_cap = 0, rowsum_rows = 0; // (ints allocated; the row count the counter pairs currently sit behind)
    int8_t *d_ext = nullptr; // op_run_external on a u8 operator: input moved to the i8 domain
    size_t ext_cap = 0;
    // d_rowsum and d_ext are ONE scratch each per operator, while a handle may be launched on several streams: every use waits (on
    // the device) for the previous use's last reader and records the event again behind its own, so concurrent launches of these
    // two paths are serialised instead of racing; growing a buffer waits for the event on the host before the free.
    hipEvent_t scratch_ev = nullptr;
    bool scratch_used = false;
    // Under stream capture (mf_model_set_graph) the handshake is skipped: a captured wait on an event recorded outside the capture
    // is not legal, and an event recorded INTO the graph would leave later eager waits looking at a stale record.  The model runtime
    // captures one stream, on which the launches are ordered anyway, and a graph's buffers never grow (the eager pass before the
    // capture sized them).
    static bool capturing(hipStream_t s) {
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &st) != hipSuccess) (void)hipGetLastError();
        return st != hipStreamCaptureStatusNone;
    }
    void scratch_acquire(hipStream_t s, bool growing) {
        if (capturing(s)) {
            if (growing) fail(MF_ERR_HIP, "a scratch buffer would have to grow inside a stream capture");
            return;
        }
        if (!scratch_ev) MF_HIP(hipEventCreateWithFlags(&scratch_ev, hipEventDisableTiming));
        if (scratch_used) {
            if (growing) MF_HIP(hipEventSynchronize(scratch_ev));
            else MF_HIP(hipStreamWaitEvent(s, scratch_ev, 0));
        }
    }
    void scratch_release(hipStream_t s) {
        if (capturing(s)) return;
        if (!scratch_ev) MF_HIP(hipEventCreateWithFlags(&scratch_ev, hipEventDisableTiming));
        MF_HIP(hipEventRecord(scratch_ev, s));
        scratch_used = true;
    }

    DevBuf d_w, d_wzp, d_A, d_S, d_Kc, d_wprep, d_wsp, d_wblk, d_wrr, d_wiso, d_table;
    // host copies of d_w (i8 domain, as uploaded), d_A, d_S, d_Kc, d_wzp and of dw_c1_lds's packed taps: the fused groups
    // (fused_*.hip) build their own operand images from them.  Kept for the operator's lifetime.
    std::vector<int8_t> h_w;
    std::vector<float> h_A, h_S;
    std::vector<int32_t> h_Kc, h_wzp;
    std::vector<uint32_t> h_wpack;
    unsigned long q_launches = 0; // launches that drew a counter set from d_queue so far (atomic increments: k_common.hpp dq_slot)
    DevBuf d_queue; // zeroed counters: the dynamic step queue of the persistent kernels launched for this operator (k_common.hpp)
    k::DwC1Args dwc1{};
    k::ConvArgs conv{};
    k::PoolArgs pool{};
    k::AddArgs add{}, add_ext{}; // ADD in the internal domain (the model runtime) and on real bytes of T (mf_op_run2); the same for i8
    int cus = 0;                 // ... the device's CU count (add_c16's grid)
    bool add_fma = false;        // ... the gated form was admitted for these constants (hostmath.cpp: h_add_fma_form)
    k::ConcatArgs cat{}, cat_ext{}; // CONCATENATION in the internal domain and on real bytes of T (mf_op_run2); the same for i8
    size_t in2_elems = 0;        // ADD, CONCATENATION: the second input's elements per inference
    int cat_unit = 0;            // ... bytes per word of concat_c4 on 16-byte aligned pointers: 16, 8 or 4 (0: Ca or Cb is no multiple of 4)
    k::PadArgs padargs{};        // PAD (k_pad.hip)
    int pad_unit = 0;            // ... bytes per word of pad_c4: 4 or 16 (0: the shape has no word kernel)
    k::FcArgs fc{};
    k::SoftmaxArgs sm{};
    k::DwFastArgs dwf{};
    k::DwStemArgs stem{};
    k::DwStemRtArgs stemrt{};
    k::PwArgs pw{};
    // run-time-geometry kernels (k_rt.hip): shapes outside the tables of kernels.hpp
    k::DwRtArgs dwrt{};
    k::PwRtArgs pwrt{};
    k::FcRtArgs fcrt{};    // FullyConnected on the matrix pipe, any K and N (k_fc_rt.hip)
    bool fcrt_ok = false;  // ... its image and constants exist (also where the operator alone stays on fc_generic)
    DevBuf d_fcw, d_fcA, d_fcKc; // ... its weight image and constants padded to 16-column tiles
    DevBuf d_sp24;         // FC_SPARSE24: the compressed 2:4 weight image (k_fc_sparse.hip fc_sparse24_image)
    k::ConvRowsArgs crows{};
    k::ConvMmArgs cmm{};
    DevBuf d_tap;          // conv_mm_rt: tap offset table
    k::ConvGemmArgs cgm{}; // Conv2D of any C and N on the matrix pipe (k_conv_gemm.hip); tap table in d_tap, image in d_fcw,
    DevBuf d_cgm_mask;     // ... constants padded to 16-column tiles in d_rtA, d_rtS, d_rtKc, d_rtwzp; window-sum byte masks
    k::DwGemmArgs dwg{};   // DepthwiseConv2D of any C on the matrix pipe (k_dw_gemm.hip); operand A in d_wprep, constants as cgm's
    DevBuf d_crw, d_crm;   // conv_rows_lds: packed weights, tap masks
    bool rt_wz = false;    // non-zero weight zero points
    int magic_mode = 0;    // conv-like operators: epilogue mode the host proved usable (k_common.hpp: 0, 1 or 2)
    // ... and mode 3, the single-fma form: found per channel by the host search (epi_fma.cpp) AND confirmed on the device over every
    // reachable accumulator (k_generic.hip verify_fma_form).  The arrays hold C', S', Kc + pivot; the two-rounding constants stay
    // beside them (a fused launch uses mode 3 only if every operator in it has it).
    bool fma_ok = false;     // ... for every channel, with at most EPI_PATCH_MAX patched accumulators in all (fma_patch)
    k::EpiPatch fma_patch{}; // the channels whose line needs ONE accumulator replaced (epi_fma.cpp); n = 0: none
    bool fma_strict() const { return fma_ok && fma_patch.n == 0; } // what the kernels without patch support need
    DevBuf d_A3, d_S3, d_Kc3;
    std::vector<float> h_A3, h_S3;
    std::vector<int32_t> h_Kc3;
    int pw_group = 1;      // pixels presented as one row of the 1x1 product (K = 8 -> 2, K = 4 -> 4)
    DevBuf d_rtA, d_rtS, d_rtKc, d_rtwzp; // constants replicated per group member
};

} // namespace mf
