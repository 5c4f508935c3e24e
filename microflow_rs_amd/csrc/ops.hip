// ops.hip -- prepared operators: fold the reference's constants into the
// per-channel device arrays the kernels consume, pick a kernel for the shape,
// launch.  Host code only (HIP runtime API); the kernels are in k_*.hip, the
// weight layouts in wimage.cpp, the fused groups in fused.hip.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>

#include "ops_impl.hpp"
#include "wimage.hpp"

namespace mf {

int dev_count() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

void dev_require(int device) {
    const int n = dev_count();
    if (n <= 0)
        fail(MF_ERR_NO_DEVICE, "no HIP device available: libmicroflow_amd has no CPU fallback");
    if (device < 0 || device >= n)
        fail(MF_ERR_INVALID_ARG, "device index " + std::to_string(device) + " out of range (" +
                                     std::to_string(n) + " devices)");
    MF_HIP(hipSetDevice(device));
}

// layer-wise DepthwiseConv2D 3x3: taps on the matrix pipe (dwpw_mm's depthwise phase, k_fused_mm.hip) where that form is the
// faster one (the three large early layers), the v_dot4 kernel dw3x3_nhwc elsewhere: k::launch_dw_mm decides per shape
static bool dw_taps_on_matrix_pipe() { return true; }

namespace {

// T = u8: move the integer side to the i8 domain (every value and zero point minus 128);
// ozp, A, the clamp and the saturation stay in the u8 domain (kernels.hpp)
struct I8Domain {
    std::vector<int8_t> w;
    std::vector<int> wzp;
    void apply(OpSpec &s, size_t wbytes) { // `s` points into this object afterwards
        if (!s.u8) return;
        w.resize(wbytes);
        for (size_t i = 0; i < wbytes; ++i) w[i] = (int8_t)(s.weights[i] ^ (int8_t)0x80);
        wzp.resize((size_t)s.nq);
        for (int i = 0; i < s.nq; ++i) wzp[(size_t)i] = s.wzp[i] - 128;
        s.weights = w.data(), s.wzp = wzp.data();
        s.izp -= 128;
    }
};

// What the routes of a convolution-like operator share: the folded per-channel constants (the operator's host copies), the
// reachable accumulators, the epilogue mode the host proved usable and the clamp.
struct ConvCtx {
    const OpSpec &s; // in the i8 domain
    bool dw;
    const std::vector<float> &A, &S;
    const std::vector<int32_t> &Kc, &wzp;
    std::vector<int64_t> acc_bound_c;                     // per output channel: max |v - izp| * sum_taps |w - wzp|
    std::vector<std::pair<int64_t, int64_t>> acc_range_c; // per output channel: the exact interval of acc over all inputs
    int64_t acc_bound = 0;                                // the largest of acc_bound_c
    int magic = 0;                                        // k_common.hpp epilogue mode 0, 1 or 2
    int lo = 0, hi = 0, xr = 0;
    bool finite = true;   // A / S all finite
    bool wz = false;      // some weight zero point is not zero
    bool zero_wzp = true; // (for u8 these are the shifted zero points: the fast kernels need wzp_u8 == 128)
                          // ... and finite constants (their epilogue has no NaN test)
    bool same3x3 = false;
    int padt = 0, padl = 0; // where the window of output (0, 0) starts above / left of the image: SAME's (K - 1) / 2, VALID's 0 -- or the
                            // rows / columns of a PAD in front of the operator (op_create_padded_conv), which only the planners see
    bool rows_bytes_any_c = false; // conv_rows_plan_pads' bytes_any_c: the PAD + convolution group's inner operator only
    bool whole_range() const { return lo == (s.u8 ? 0 : -128) && hi == (s.u8 ? 255 : 127); } // the clamp is the element type's range
};

// per-channel A/S/Kc/wzp arrays for the conv-like operators
// Returns the worst-case |acc| over all inputs: max|v - izp| * max_c sum_taps |w - wzp|
// (acc = sum over ALL taps of (v' - izp)(w - wzp), the halo contributing 0).
int64_t fold_conv_constants(const OpSpec &s, bool depthwise, std::vector<float> &A,
                            std::vector<float> &S, std::vector<int32_t> &Kc,
                            std::vector<int32_t> &wzp, std::vector<int64_t> &acc_bound_per_channel,
                            std::vector<std::pair<int64_t, int64_t>> &acc_range_per_channel) {
    const int N = s.N;
    const int taps = s.KH * s.KW;
    int64_t max_wabs = 0;
    A.resize(N), S.resize(N), Kc.resize(N), wzp.resize(N);
    for (int c = 0; c < N; ++c) {
        volatile float a = (float)s.ozp + s.c0[c]; // f32(ozp) + c0[c], rounded once, as the reference does first
        A[c] = a;
        S[c] = s.c1[c < s.nc1 ? c : 0];            // constants.1.get(b).unwrap_or(constants.1[0])
        wzp[c] = s.wzp[c < s.nq ? c : 0];          // zero_point.get(b).unwrap_or(zero_point[0])
        int32_t wsum = 0;
        int32_t T;
        int64_t wabs = 0;
        // the exact interval of acc = sum_taps (v - izp)(w - wzp) over int8 v (a halo tap contributes 0, which lies inside every
        // tap's own interval): what the single-fma epilogue has to reproduce the reference on (epi_fma.cpp)
        const int64_t vlo = -128 - s.izp, vhi = 127 - s.izp;
        int64_t amin = 0, amax = 0;
        auto tap = [&](int w) {
            wsum = wrap_add(wsum, w);
            const int64_t dw_ = (int64_t)w - wzp[c];
            wabs += dw_ < 0 ? -dw_ : dw_;
            amin += std::min(std::min(vlo * dw_, vhi * dw_), (int64_t)0), amax += std::max(std::max(vlo * dw_, vhi * dw_), (int64_t)0);
        };
        if (depthwise) { // weights [KH][KW][N]
            for (int t = 0; t < taps; ++t) tap(s.weights[(size_t)t * N + c]);
            T = taps;
        } else { // filters [N][KH][KW][C]
            const int8_t *f = s.weights + (size_t)c * taps * s.C;
            for (int t = 0; t < taps * s.C; ++t) tap(f[t]);
            T = taps * s.C;
        }
        acc_range_per_channel.push_back({amin, amax});
        max_wabs = std::max(max_wabs, wabs);
        acc_bound_per_channel.push_back(wabs * std::max(127 - s.izp, s.izp + 128));
        // Kc = -izp * sum(w) + T * izp * wzp   (k2 and k3 of the reference with the halo == izp)
        Kc[c] = wrap_add(wrap_sub(0, wrap_mul(s.izp, wsum)), wrap_mul(wrap_mul(T, s.izp), wzp[c]));
    }
    const int64_t vdev = std::max(127 - s.izp, s.izp + 128); // max |v - izp| over int8 v
    return vdev * max_wabs;
}

bool all_finite(const std::vector<float> &v) {
    return std::all_of(v.begin(), v.end(), [](float x) { return std::isfinite(x); });
}
bool all_zero(const std::vector<int32_t> &v) {
    return std::all_of(v.begin(), v.end(), [](int32_t x) { return x == 0; });
}

// Epilogue mode 3: y = v_cvt_pk_u8_f32(v_fma_f32(S', bits(acc + pivot), C')).  Conditions: bit-pattern accumulators (mode >= 1),
// the clamp is the element type's whole range (the conversion's saturation IS the clamp), finite constants; then a solution
// for EVERY channel (host, exact: epi_fma.cpp) that the device confirms on every reachable accumulator.
void find_fma_form(OpImpl &op, const ConvCtx &c) {
    const OpSpec &s = c.s;
    const bool no_fma = switches().no_fma_epi; // tests / A-B: keep the two-rounding forms
    if (c.magic < 1 || no_fma || !c.whole_range() || !c.finite) return;
    std::vector<float> A3((size_t)s.N), S3((size_t)s.N);
    std::vector<int32_t> K3((size_t)s.N), piv((size_t)s.N), amn((size_t)s.N), amx((size_t)s.N), pP((size_t)s.N, 0), pR((size_t)s.N, 0);
    k::EpiPatch patch{};
    bool ok = true;
    int fail_c = -1;
    for (int ch = 0; ch < s.N && ok; ++ch) {
        FmaForm f;
        const auto &r = c.acc_range_c[(size_t)ch];
        ok = fma_form_search(c.A[(size_t)ch], c.S[(size_t)ch], s.u8 ? 0 : 128, c.lo, c.hi, r.first, r.second, f, nullptr, true);
        if (ok && f.patch_delta != 0) { // this channel's line needs one accumulator replaced by its neighbour
            if (patch.n == k::EPI_PATCH_MAX) ok = false; // (more than the kernels' patch list holds: the operator keeps the two-rounding form)
            else {
                const int32_t P = wrap_add(wrap_add(k::MF_MAGIC_I, (int32_t)f.patch_acc), f.d);
                patch.ch[patch.n] = ch, patch.P[patch.n] = P, patch.R[patch.n] = P + f.patch_delta, ++patch.n;
                pP[(size_t)ch] = P, pR[(size_t)ch] = P + f.patch_delta;
            }
        }
        if (!ok) fail_c = ch;
        A3[(size_t)ch] = f.C, S3[(size_t)ch] = f.S, piv[(size_t)ch] = f.d, K3[(size_t)ch] = wrap_add(c.Kc[(size_t)ch], f.d);
        amn[(size_t)ch] = (int32_t)r.first, amx[(size_t)ch] = (int32_t)r.second;
    }
    unsigned long long nbad = 0;
    if (ok) {
        op.d_A3.upload(A3.data(), A3.size() * 4), op.d_S3.upload(S3.data(), S3.size() * 4), op.d_Kc3.upload(K3.data(), K3.size() * 4);
        DevBuf d_piv, d_amn, d_amx, d_bad, d_pP, d_pR;
        const std::vector<unsigned long long> zero((size_t)s.N, 0ull);
        d_piv.upload(piv.data(), piv.size() * 4), d_amn.upload(amn.data(), amn.size() * 4), d_amx.upload(amx.data(), amx.size() * 4);
        d_pP.upload(pP.data(), pP.size() * 4), d_pR.upload(pR.data(), pR.size() * 4);
        d_bad.upload(zero.data(), zero.size() * 8);
        std::vector<unsigned long long> bad((size_t)s.N, ~0ull);
        if (k::verify_fma_form(op.d_A.as<float>(), op.d_S.as<float>(), op.d_A3.as<float>(), op.d_S3.as<float>(), d_piv.as<int>(),
                               d_amn.as<int>(), d_amx.as<int>(), d_pP.as<int>(), d_pR.as<int>(), s.N, (float)c.lo, (float)c.hi, s.u8,
                               (unsigned long long *)d_bad.p, nullptr))
            MF_HIP(hipMemcpy(bad.data(), d_bad.p, bad.size() * 8, hipMemcpyDeviceToHost));
        for (int ch = 0; ch < s.N; ++ch)
            if (bad[(size_t)ch]) nbad += bad[(size_t)ch], fail_c = ch;
        ok = nbad == 0;
        if (!ok) // the host's exact arithmetic and the device disagree: that is a bug in one of them, say so -- and do not use the form
            fprintf(stderr, "[microflow_amd] single-fma epilogue REJECTED by the device check (%llu accumulators differ, channel %d)\n", nbad, fail_c);
    }
    if (ok) op.fma_patch = patch;
    if (ok) op.fma_ok = true, op.h_A3 = A3, op.h_S3 = S3, op.h_Kc3 = K3;
    if (switches().debug_epi) {
        fprintf(stderr, "[epi] single-fma form: %s%s\n", ok ? ("all channels, " + std::to_string(patch.n) + " patched").c_str() : "no: channel ",
                ok ? "" : std::to_string(fail_c).c_str());
        if (ok && patch.n) {
            fprintf(stderr, "[epi]   patched channels:");
            for (int e = 0; e < patch.n; ++e) fprintf(stderr, " %d", patch.ch[e]);
            fprintf(stderr, "\n");
        }
    }
}

// Everything a convolution-like operator decides before it picks a kernel: the folded constants (uploaded, and kept on the host
// in the operator), the epilogue mode, the single-fma form, the generic kernel's argument block.
ConvCtx prepare_conv(OpImpl &op, const OpSpec &s, bool dw, int lo, int hi, int xr) {
    ConvCtx c{s, dw, op.h_A, op.h_S, op.h_Kc, op.h_wzp};
    c.lo = lo, c.hi = hi, c.xr = xr;
    // the fast kernels may convert the accumulator to f32 by bit pattern when it provably
    // stays below 2^22 in magnitude (requant_t<true> in k_common.hpp)
    const bool no_magic = switches().no_magic; // tests: force the convert form
    c.acc_bound = fold_conv_constants(s, dw, op.h_A, op.h_S, op.h_Kc, op.h_wzp, c.acc_bound_c, c.acc_range_c);
    c.finite = op.finite_consts = all_finite(c.A) && all_finite(c.S);
    c.wz = !all_zero(c.wzp);
    c.zero_wzp = !c.wz && c.finite;
    c.same3x3 = s.KH == 3 && s.KW == 3 && s.pad == MF_PAD_SAME && s.sh == s.sw &&
                s.OH == (s.H + s.sh - 1) / s.sh && s.OW == (s.W + s.sw - 1) / s.sw;
    c.padt = s.pad == MF_PAD_SAME ? (s.KH - 1) / 2 : 0, c.padl = s.pad == MF_PAD_SAME ? (s.KW - 1) / 2 : 0;
    c.magic = !no_magic && c.acc_bound < (1 << 22) ? 1 : 0;
    // mode 2 (k_common.hpp): the clamp is the element type's whole range (so a saturating pack can do it) and
    // |x| = |A + S * acc| stays below 2^15 for every input (so x + 128 fits the i16 the pack saturates from)
    const bool no_sat = switches().no_sat_pack; // tests: force the v_med3 form
    if (c.magic && !no_sat && c.whole_range() && c.finite) {
        double xmax = 0.0;
        for (int ch = 0; ch < s.N; ++ch)
            xmax = std::max(xmax, std::fabs((double)c.A[(size_t)ch]) + std::fabs((double)c.S[(size_t)ch]) * (double)c.acc_bound_c[(size_t)ch]);
        if (xmax < 30000.0) c.magic = 2;
    }
    if (switches().debug_epi) // which epilogue mode each operator gets, and why
        fprintf(stderr, "[epi] %s %dx%dx%d -> %d: |acc| < %lld, clamp [%d, %d] -> mode %d\n", dw ? "depthwise" : "conv", s.H, s.W, s.C, s.N,
                (long long)c.acc_bound, lo, hi, c.magic);
    op.magic_mode = c.magic;
    const size_t wbytes = dw ? (size_t)s.KH * s.KW * s.N : (size_t)s.N * s.KH * s.KW * s.C;
    op.h_w.assign(s.weights, s.weights + wbytes);
    op.d_w.upload(s.weights, wbytes);
    op.d_wzp.upload(c.wzp.data(), c.wzp.size() * 4);
    op.d_A.upload(c.A.data(), c.A.size() * 4);
    op.d_S.upload(c.S.data(), c.S.size() * 4);
    op.d_Kc.upload(c.Kc.data(), c.Kc.size() * 4);
    {
        const std::vector<int> zeros((size_t)k::DYNQ_INTS * k::DYNQ_RING, 0);
        op.d_queue.upload(zeros.data(), zeros.size() * sizeof(int));
    }
    find_fma_form(op, c);
    k::ConvArgs &a = op.conv;
    a.H = s.H, a.W = s.W, a.C = s.C, a.N = s.N, a.KH = s.KH, a.KW = s.KW, a.sh = s.sh, a.sw = s.sw;
    a.OH = s.OH, a.OW = s.OW, a.pad_same = s.pad == MF_PAD_SAME, a.izp = s.izp;
    a.lo_f = (float)lo, a.hi_f = (float)hi;
    a.w = op.d_w.as<int8_t>(), a.wzp = op.d_wzp.as<int>(), a.A = op.d_A.as<float>();
    a.S = op.d_S.as<float>(), a.Kc = op.d_Kc.as<int>();
    a.xr = xr;
    op.generic_name = dw ? "dwconv_generic" : "conv2d_generic";
    return c;
}

// ---- what every route writes into its kernel's argument block ----
// the clamp, the epilogue mode and the element domain ...
template <typename F> void epi_fields(F &f, const OpImpl &op, const ConvCtx &c) {
    f.lo_f = op.conv.lo_f, f.hi_f = op.conv.hi_f, f.magic = c.magic, f.xr = c.xr;
}
// ... and the input zero point in every byte of a dword, for the kernels that pad with it
template <typename F> void epi_fields_izp(F &f, const OpImpl &op, const ConvCtx &c) {
    f.izp4 = 0x01010101u * (uint32_t)(uint8_t)(int8_t)c.s.izp;
    epi_fields(f, op, c);
}
template <typename F> void step_queue(F &f, OpImpl &op) { f.queue = (int *)op.d_queue.p, f.qlaunch = &op.q_launches; }

struct ConstPtrs {
    const float *A, *S;
    const int *Kc, *wzp;
};
// the per-channel constants as the operator uploaded them
ConstPtrs channel_consts(const OpImpl &op) { return {op.conv.A, op.conv.S, op.conv.Kc, op.conv.wzp}; }
// The constants of the rows of a product whose rows are not the channels: `np` rows, of which the first `rows` take the constants
// of channel ch_of(row) and the rest are padding (zero).  One set per operator (d_rtA, d_rtS, d_rtKc, d_rtwzp).
template <typename M> ConstPtrs row_consts(OpImpl &op, const ConvCtx &c, size_t np, int rows, M ch_of) {
    std::vector<float> pA(np, 0.0f), pS(np, 0.0f);
    std::vector<int32_t> pK(np, 0), pZ(np, 0);
    for (int r = 0; r < rows; ++r) {
        const size_t ch = (size_t)ch_of(r);
        pA[(size_t)r] = c.A[ch], pS[(size_t)r] = c.S[ch], pK[(size_t)r] = c.Kc[ch], pZ[(size_t)r] = c.wzp[ch];
    }
    op.d_rtA.upload(pA.data(), np * 4), op.d_rtS.upload(pS.data(), np * 4);
    op.d_rtKc.upload(pK.data(), np * 4), op.d_rtwzp.upload(pZ.data(), np * 4);
    return {op.d_rtA.as<float>(), op.d_rtS.as<float>(), op.d_rtKc.as<int>(), op.d_rtwzp.as<int>()};
}

// ---- the routes of a convolution-like operator, in the order op_create tries them (create_conv) ----
// A route returns true when it took the operator.  Routes 1 - 5 are ONE else-if chain on their conditions: the first whose
// condition holds ends the chain, also where it then leaves the operator on the generic kernel (route_dw_c1).
// A *_plan call that fails may leave its argument block partly written; nothing reads the block of a route not taken.

// 1. a table shape of the 3x3 depthwise kernels (kernels.hpp)
bool route_dw_table(OpImpl &op, const ConvCtx &c) {
    const OpSpec &s = c.s;
    if (!(!switches().no_table && c.dw && c.zero_wzp && c.same3x3 && s.C == s.N && k::dw_fast_name(s.H, s.W, s.C, s.sh))) return false;
    op.fast = OpImpl::DW_NHWC;
    op.fast_name = k::dw_fast_name(s.H, s.W, s.C, s.sh);
    k::DwFastArgs &f = op.dwf;
    f.w = op.conv.w, f.A = op.conv.A, f.S = op.conv.S, f.Kc = op.conv.Kc;
    epi_fields_izp(f, op, c);
    f.wmm = nullptr, f.wsp = nullptr, f.wblk = nullptr;
    step_queue(f, op);
    if (s.C == 8 || s.C % 16 == 0) { // matrix-pipe form of the taps for the fused pair kernels
        const std::vector<int8_t> prep = wimage::build_dw_mm_weights(s.weights, s.C);
        op.d_wprep.upload(prep.data(), prep.size());
        f.wmm = op.d_wprep.p;
        const std::vector<int8_t> sp = wimage::build_dw_sp_weights(prep, s.C == 8 ? 1 : s.C / 16); // the sparse form of the same taps (k_quad.hip)
        if (!sp.empty()) {
            op.d_wsp.upload(sp.data(), sp.size());
            f.wsp = op.d_wsp.p;
        }
        if (s.sh == 1) { // the block form of the taps (k_quad.hip BlkPhase): stride 1 only
            const std::vector<int8_t> blk = wimage::build_dw_blk_weights(s.weights, s.C);
            op.d_wblk.upload(blk.data(), blk.size());
            f.wblk = op.d_wblk.p;
        }
        if (dw_taps_on_matrix_pipe() && k::dw_mm_name(s.H, s.W, s.C, s.sh)) op.fast_name = k::dw_mm_name(s.H, s.W, s.C, s.sh);
    }
    return true;
}

// 2. the one-input-channel 3x3 stem of a table shape
bool route_dw_stem(OpImpl &op, const ConvCtx &c) {
    const OpSpec &s = c.s;
    if (!(!switches().no_table && c.dw && c.zero_wzp && c.same3x3 && s.C == 1 && k::dw_stem_name(s.H, s.W, s.N, s.sh))) return false;
    op.fast = OpImpl::DW_STEM;
    op.fast_name = k::dw_stem_name(s.H, s.W, s.N, s.sh);
    k::DwStemArgs &f = op.stem;
    step_queue(f, op);
    wimage::build_stem_rows(s.weights, s.N, f.wrow);
    wimage::build_stem_mm(s.weights, s.N, &f.wmm[0][0], 2);
    for (int ch = 0; ch < 8; ++ch) f.A[ch] = c.A[ch], f.S[ch] = c.S[ch], f.Kc[ch] = c.Kc[ch];
    epi_fields_izp(f, op, c);
    return true;
}

// 3. a one-channel 3x3 stride-2 stem at any resolution: the taps as one MFMA per 256 output bytes (k_rt.hip)
bool route_dw_stem_rt(OpImpl &op, const ConvCtx &c) {
    const OpSpec &s = c.s;
    if (!(!switches().no_rt && !switches().no_stem_rt && c.dw && c.zero_wzp && c.same3x3 && s.C == 1 && s.sh == 2 &&
          k::dw_stem_rt_plan(op.stemrt, s.H, s.W, s.N, s.OH, s.OW)))
        return false;
    op.fast = OpImpl::DW_STEM_RT;
    op.fast_name = "dw3x3_stem_rt<" + std::to_string(s.N) + ">";
    k::DwStemRtArgs &f = op.stemrt;
    step_queue(f, op);
    wimage::build_stem_mm(s.weights, s.N, &f.wmm[0][0], 4);
    for (int ch = 0; ch < 8; ++ch) f.A[ch] = c.A[(size_t)(ch % s.N)], f.S[ch] = c.S[(size_t)(ch % s.N)], f.Kc[ch] = c.Kc[(size_t)(ch % s.N)];
    epi_fields_izp(f, op, c);
    return true;
}

// 4. one input channel, few output channels, any filter: LDS-staged direct kernel.  (Kept as it was: a shape that meets the
// condition but not dw_c1_supported still ends the chain of routes 1 - 5, so route 5 never sees it -- it is a depthwise.)
bool route_dw_c1(OpImpl &op, const ConvCtx &c) {
    const OpSpec &s = c.s;
    if (!(c.dw && c.zero_wzp && s.C == 1 && s.N <= 8)) return false;
    k::DwC1Args &f = op.dwc1;
    f.H = s.H, f.W = s.W, f.N = s.N, f.KH = s.KH, f.KW = s.KW, f.sh = s.sh, f.sw = s.sw;
    f.OH = s.OH, f.OW = s.OW, f.pad_same = s.pad == MF_PAD_SAME, f.izp = s.izp;
    f.A = op.conv.A, f.S = op.conv.S, f.Kc = op.conv.Kc;
    epi_fields(f, op, c);
    f.KG = (s.KW + 3) / 4;
    // a window row is read as KG + 1 aligned dwords starting at (row start & ~3)
    f.TWP = ((((s.OW - 1) * s.sw + 3) & ~3) + 4 * (f.KG + 1) + 3) & ~3;
    if (k::dw_c1_supported(f)) {
        op.h_wpack = wimage::build_dw_c1_pack(s.weights, s.KH, s.KW, s.N, f.KG);
        op.d_wprep.upload(op.h_wpack.data(), op.h_wpack.size() * 4);
        f.wpack = op.d_wprep.as<uint32_t>();
        op.fast = OpImpl::DW_C1;
        op.fast_name = "dw_c1_lds";
    }
    return true;
}

// 5. a table shape of the 1x1 convolution on the matrix pipe
bool route_pw_mfma(OpImpl &op, const ConvCtx &c) {
    const OpSpec &s = c.s;
    if (!(!switches().no_table && !c.dw && c.zero_wzp && s.KH == 1 && s.KW == 1 && s.sh == 1 && s.sw == 1 &&
          s.OH == s.H && s.OW == s.W && k::pw_name(s.C, s.N) &&
          (s.C != 8 || ((s.H * s.W) % 2 == 0))))
        return false;
    op.fast = OpImpl::PW_MFMA;
    op.fast_name = k::pw_name(s.C, s.N);
    const std::vector<int8_t> prep = wimage::build_pw_weights(s.weights, s.C, s.N);
    op.d_wprep.upload(prep.data(), prep.size());
    k::PwArgs &f = op.pw;
    f.wprep = op.d_wprep.p, f.A = op.conv.A, f.S = op.conv.S, f.Kc = op.conv.Kc;
    epi_fields(f, op, c);
    f.wrr = nullptr, f.wiso = nullptr;
    if ((s.C == 8 || s.C == 16 || s.C == 32) && (s.C == 8 ? 2 * s.N : s.N) % 16 == 0) {
        const std::vector<int8_t> rr = wimage::build_pw_rr_weights(s.weights, s.C, s.N);
        op.d_wrr.upload(rr.data(), rr.size());
        f.wrr = op.d_wrr.p;
    }
    if (s.C == 8 && s.N % 16 == 0) { // the isolating operands behind a block-form depthwise
        const std::vector<int8_t> iso = wimage::build_pw_iso_weights(s.weights, s.N);
        op.d_wiso.upload(iso.data(), iso.size());
        f.wiso = op.d_wiso.p;
    }
    return true;
}

// Shapes outside the tables: the run-time-geometry kernels (k_rt.hip and later), with or without weight zero points.  Each of
// these routes looks only at an operator no earlier route took (route_conv_rows: see there).
bool rt_candidate(const OpImpl &op, const ConvCtx &c) {
    const bool no_rt = switches().no_rt; // tests / A-B: shape-generic kernels instead
    return op.fast == OpImpl::NONE && !no_rt && c.finite;
}

// 6. 3x3 SAME depthwise, one output per channel
bool route_dw_rt(OpImpl &op, const ConvCtx &c) {
    const OpSpec &s = c.s;
    if (!(rt_candidate(op, c) && c.dw && c.same3x3 && s.C == s.N && k::dw_rt_plan(op.dwrt, s.H, s.W, s.C, s.sh, s.OH, s.OW))) return false;
    op.fast = OpImpl::DW_RT;
    op.rt_wz = c.wz;
    op.fast_name = std::string("dw3x3_rt<") + std::to_string(s.sh) + (op.rt_wz ? ",wzp>" : ">");
    k::DwFastArgs &f = op.dwrt.dw;
    f.w = op.conv.w, f.A = op.conv.A, f.S = op.conv.S, f.Kc = op.conv.Kc, f.wmm = nullptr;
    epi_fields_izp(f, op, c);
    step_queue(f, op);
    op.dwrt.wzp = op.conv.wzp;
    if (!op.rt_wz && (s.C % 16 == 0 || s.C == 8)) { // matrix-pipe form of the taps: what the fused chain kernel (k_chain.hip) multiplies
        const std::vector<int8_t> prep = wimage::build_dw_mm_weights(s.weights, s.C);
        op.d_wprep.upload(prep.data(), prep.size());
        f.wmm = op.d_wprep.p;
    }
    return true;
}

// 7. 1x1 stride-1 convolution of any K and N
bool route_pw_rt(OpImpl &op, const ConvCtx &c) {
    const OpSpec &s = c.s;
    if (!(rt_candidate(op, c) && !c.dw && s.KH == 1 && s.KW == 1 && s.sh == 1 && s.sw == 1 && s.OH == s.H && s.OW == s.W)) return false;
    const bool wz = c.wz;
    // K not a multiple of 16: `group` consecutive pixels form one row of the product (K = 8, 24, 40 ...: 2; K = 4, 12, 20 ...: 4)
    int group = s.C % 16 == 0 ? 1 : (s.C % 8 == 0 ? 2 : (s.C % 4 == 0 ? 4 : 0));
    // weights in registers (zero weight zero points, N * group <= 256): more pixels per row while the 64-deep k
    // step has room, so that the MFMA's k span is used and a row's output is a long contiguous run
    if (s.N % 4 != 0) group = 0; // packed dword results: N in whole fours (a 2-output head runs conv1x1_rowwave)
    bool reg = group >= 1 && !wz && s.N * group <= 256 && s.C * group <= 512;
    // (... but not past 64 output bytes per row: one wave then stores whole rows, 1 KiB contiguous per store
    // instruction, instead of two waves storing half lines -- MF_PW_RT_NCAP: tuning)
    const int ncap = switches().pw_rt_ncap;
    if (reg)
        while (s.C * group * 2 <= 64 && s.N * group * 2 <= std::max(ncap, s.N)) group *= 2;
    if (!(group >= 1 && !(wz && group > 1) && (reg || k::pw_rt_supported(s.C * group, s.N * group, wz)))) return false;
    op.fast = OpImpl::PW_RT;
    op.rt_wz = wz, op.pw_group = group;
    op.fast_name = "pw_rt<" + std::to_string(s.C) + "," + std::to_string(s.N) + (wz ? ",wzp>" : ">");
    const int NTg = (s.N * group + 15) / 16;
    const int TB = reg ? (NTg < 4 ? NTg : 4) : 0;
    const int NBLK = reg ? (NTg + TB - 1) / TB : 0;            // <= 4 because N * group <= 256
    const int NSPLIT = NBLK <= 1 ? 1 : (NBLK == 2 ? 2 : 4);
    const std::vector<int8_t> prep = reg ? wimage::build_pw_rt_reg_weights(s.weights, s.C, s.N, group, TB, NSPLIT)
                                         : wimage::build_pw_rt_weights(s.weights, s.C, s.N, group, wz);
    op.d_wprep.upload(prep.data(), prep.size());
    k::PwRtArgs &f = op.pwrt;
    f.wprep = op.d_wprep.p;
    f.K = s.C * group, f.N = s.N * group, f.KS = (f.K + 63) / 64, f.NT = (f.N + 15) / 16;
    f.patch_pitch = (f.N + 15) & ~15;
    f.TB = TB, f.NSPLIT = NSPLIT;
    epi_fields(f, op, c);
    // group > 1: the constants of row gi * N + n are channel n's
    const ConstPtrs p = group == 1 ? channel_consts(op) : row_consts(op, c, (size_t)f.N, f.N, [&](int r) { return r % s.N; });
    f.A = p.A, f.S = p.S, f.Kc = p.Kc, f.wzp = p.wzp;
    return true;
}

// 8. few input channels (a first convolution; a one-channel depthwise with more than 8 outputs): window rows as dwords.
// The one route that may REPLACE an earlier one: a one-channel depthwise keeps dw_c1_lds only where the one-launch speech kernel
// builds on it, k_dwfc.hip (measured on the 96x96 stem: dw_c1_lds 1.22 ms, conv_rows_lds 0.70 ms; MF_DW_C1=lds forces the old
// kernel).  Steps aside for conv1x1_rowwave.  One input channel with image rows that are not whole dwords (W % 4 != 0: audio features):
// the same route, launched as conv_rows_bytes (49x13 -> 8: dw_c1_lds 0.090 ms, dw_rows_lds<bytes> 0.065 ms per 16 384 images).
bool route_conv_rows(OpImpl &op, const ConvCtx &c) {
    const OpSpec &s = c.s;
    const bool c1_lds = switches().dw_c1_lds, no_rt = switches().no_rt;
    const bool rows_for_c1 = !c1_lds && !k::dwfc_supported(s.H, s.W, s.KH, s.KW, s.sh, s.sw, s.OH, s.OW, s.N, 4);
    if (!((op.fast == OpImpl::NONE || (op.fast == OpImpl::DW_C1 && rows_for_c1)) && !no_rt && c.finite &&
          (!c.dw || s.C == 1) && !(s.KH == 1 && s.KW == 1 && !c.dw && k::conv1x1_rowwave_supported(op.conv)) &&
          k::conv_rows_plan_pads(op.crows, s.H, s.W, s.C, s.N, s.KH, s.KW, s.sh, s.sw, s.OH, s.OW, c.padt, c.padl, c.rows_bytes_any_c)))
        return false;
    k::ConvRowsArgs &f = op.crows;
    const std::vector<uint32_t> wp = wimage::build_conv_rows_pack(s.weights, c.dw, s.KH, s.KW, s.C, s.N, f.KG, f.NP);
    const std::vector<uint32_t> mk = wimage::build_conv_rows_mask(s.KW * s.C, f.KG);
    op.d_crw.upload(wp.data(), wp.size() * 4), op.d_crm.upload(mk.data(), mk.size() * 4);
    f.wpack = op.d_crw.as<uint32_t>(), f.mask = op.d_crm.as<uint32_t>();
    const ConstPtrs p = channel_consts(op);
    f.A = p.A, f.S = p.S, f.Kc = p.Kc, f.wzp = p.wzp;
    epi_fields_izp(f, op, c);
    op.fast = OpImpl::CONV_ROWS;
    op.rt_wz = c.wz;
    // (rows that are not whole dwords: the conv_rows_bytes launch, k::ConvRowsArgs::BYTES())
    op.fast_name = std::string(c.dw ? "dw_rows_lds" : "conv_rows_lds") + (f.BYTES() ? (op.rt_wz ? "<bytes,wzp>" : "<bytes>") : (op.rt_wz ? "<wzp>" : ""));
    return true;
}

// conv_mm_rt's argument block once its plan exists (routes 9 and 11)
void conv_mm_fields(OpImpl &op, const ConvCtx &c, const std::vector<int8_t> &prep, const std::vector<int> &tap) {
    k::ConvMmArgs &f = op.cmm;
    op.d_wprep.upload(prep.data(), prep.size());
    op.d_tap.upload(tap.data(), tap.size() * sizeof(int));
    f.wprep = op.d_wprep.p, f.tap_off = op.d_tap.as<int>();
    const ConstPtrs p = channel_consts(op);
    f.A = p.A, f.S = p.S, f.Kc = p.Kc, f.wzp = p.wzp;
    epi_fields_izp(f, op, c);
    op.fast = OpImpl::CONV_MM;
}

// 9. any other DepthwiseConv2D with C % 16 == 0 and one output per channel -- a filter other than 3x3, VALID padding, unequal
// strides -- : conv_mm_rt in its depthwise mode, taps of a 16-channel group on the matrix pipe against block-diagonal weights
bool route_dw_mm(OpImpl &op, const ConvCtx &c) {
    const OpSpec &s = c.s;
    if (!(rt_candidate(op, c) && c.dw && s.C == s.N && s.C % 16 == 0 && !c.wz)) return false;
    std::vector<int> tap;
    if (!k::conv_mm_plan_pads(op.cmm, tap, s.H, s.W, s.C, s.N, s.KH, s.KW, s.sh, s.sw, s.OH, s.OW, c.padt, c.padl, false, true)) return false;
    conv_mm_fields(op, c, wimage::build_dw_mm_rt_weights(s.weights, s.KH, s.KW, s.C, op.cmm.KS), tap);
    op.rt_wz = false;
    op.fast_name = "dw_mm_rt<" + std::to_string(s.KH) + "x" + std::to_string(s.KW) + ">";
    return true;
}

// 10. every other DepthwiseConv2D with one output per channel and whole-dword image rows -- C % 16 != 0, filter zero points, 3x3
// SAME shapes dw3x3_rt rejects -- : the same block-diagonal product, operand B read at its natural alignment (k_dw_gemm.hip)
bool dw_gemm_candidate(const OpImpl &op, const ConvCtx &c) { // (also of route 13's one-channel case)
    return op.fast == OpImpl::NONE && c.dw && !switches().no_rt && !switches().no_dw_gemm && c.finite;
}
bool route_dw_gemm(OpImpl &op, const ConvCtx &c) {
    const OpSpec &s = c.s;
    k::DwGemmArgs &f = op.dwg;
    if (!(dw_gemm_candidate(op, c) && s.C == s.N && s.C >= 2)) return false;
    if (!k::dw_gemm_plan_pads(f, s.H, s.W, s.C, s.KH, s.KW, s.sh, s.sw, s.OH, s.OW, c.padt, c.padl)) return false;
    const bool wz = c.wz;
    const std::vector<int8_t> prep = wimage::build_dw_mm_rt_weights(s.weights, s.KH, s.KW, s.C, f.KS, f.P);
    op.d_wprep.upload(prep.data(), prep.size());
    f.wprep = op.d_wprep.p;
    // the constants of each row's channel
    const ConstPtrs p = row_consts(op, c, (size_t)f.NBLK * 16, f.P > 1 ? f.P * s.C : s.C, [&](int r) { return r % s.C; });
    f.A = p.A, f.S = p.S, f.Kc = p.Kc, f.wzp = p.wzp;
    epi_fields_izp(f, op, c);
    op.fast = OpImpl::DW_GEMM;
    op.rt_wz = wz;
    op.fast_name = "dw_gemm_rt<" + std::to_string(s.KH) + "x" + std::to_string(s.KW) + (wz ? ",wzp>" : ">");
    if (switches().verbose)
        fprintf(stderr, "[microflow_amd] dw_gemm_rt %dx%dx%d %dx%d: %d k steps, %d channel groups of %d pixels, %s %d x %d rows, %d B LDS\n", s.H,
                s.W, s.C, s.KH, s.KW, f.KS, f.NBLK, f.P, f.NBANDS > 1 ? "bands of" : "images per step:", f.NBANDS > 1 ? f.BH : f.G, f.RB, f.lds);
    return true;
}

// 11. any other Conv2D with C % 16 == 0: MFMA product over K = KH KW C with the image staged in LDS.  Steps aside for
// conv1x1_rowwave.
bool route_conv_mm(OpImpl &op, const ConvCtx &c) {
    const OpSpec &s = c.s;
    if (!(rt_candidate(op, c) && !c.dw && !(s.KH == 1 && s.KW == 1 && k::conv1x1_rowwave_supported(op.conv)))) return false;
    const bool wz = c.wz;
    std::vector<int> tap;
    if (!k::conv_mm_plan_pads(op.cmm, tap, s.H, s.W, s.C, s.N, s.KH, s.KW, s.sh, s.sw, s.OH, s.OW, c.padt, c.padl, wz)) return false;
    const int Ktot = s.KH * s.KW * s.C;
    std::vector<int8_t> prep = wimage::build_pw_rt_reg_weights(s.weights, Ktot, s.N, 1, op.cmm.TB, op.cmm.NBLK); // [N][KH][KW][C] IS [N][K]
    if (wz) { // + a tile of ones over the real k-bytes
        const size_t base_sz = prep.size();
        prep.resize(base_sz + (size_t)op.cmm.KS * 1024, 0);
        wimage::fill_ones_tile(prep.data() + base_sz, Ktot, op.cmm.KS);
    }
    conv_mm_fields(op, c, prep, tap);
    op.rt_wz = wz;
    op.fast_name = std::string("conv_mm_rt") + (wz ? "<wzp>" : "");
    return true;
}

// 12. few outputs: one wavefront per pixel
bool route_conv1x1_row(OpImpl &op, const ConvCtx &c) {
    if (!(op.fast == OpImpl::NONE && !c.dw && k::conv1x1_rowwave_supported(op.conv))) return false;
    op.fast = OpImpl::CONV1X1_ROW, op.fast_name = "conv1x1_rowwave";
    return true;
}

// 13. every other Conv2D with whole-dword image rows: the MFMA product over K' = KH x (KW C rounded up to 16), the weights
// resident in LDS in N slices (k_conv_gemm.hip).  Also a one-channel DepthwiseConv2D with more outputs than the C = 1 kernels
// above take: the reference reads channel 0 for every output (depthwise_conv_2d.rs:67), so it IS this Conv2D with C = 1 and the
// filters [N][KH][KW][1] (the filter zero points and Kc are per output channel in both).  (conv1x1_rowwave came first: route 12.)
bool route_conv_gemm(OpImpl &op, const ConvCtx &c) {
    const OpSpec &s = c.s;
    const bool dw_c1 = dw_gemm_candidate(op, c) && s.C == 1 && s.N > 1;
    if (!((rt_candidate(op, c) && !switches().no_conv_gemm && !c.dw) || dw_c1)) return false;
    const bool wz = c.wz;
    std::vector<int> tap;
    std::vector<uint32_t> mask;
    std::vector<int8_t> wt;
    if (dw_c1) {
        const int T = s.KH * s.KW;
        wt.resize((size_t)s.N * T);
        for (int n = 0; n < s.N; ++n)
            for (int t = 0; t < T; ++t) wt[(size_t)n * T + t] = s.weights[(size_t)t * s.N + n];
    }
    k::ConvGemmArgs &f = op.cgm;
    if (!k::conv_gemm_plan_pads(f, tap, mask, s.H, s.W, s.C, s.N, s.KH, s.KW, s.sh, s.sw, s.OH, s.OW, c.padt, c.padl, wz)) return false;
    const std::vector<int8_t> img = k::conv_gemm_weight_image(dw_c1 ? wt.data() : s.weights, f);
    op.d_fcw.upload(img.data(), img.size());
    op.d_tap.upload(tap.data(), tap.size() * sizeof(int));
    op.d_cgm_mask.upload(mask.data(), mask.size() * 4);
    f.wimg = op.d_fcw.p, f.tap = op.d_tap.as<int>(), f.kmask = op.d_cgm_mask.as<uint32_t>();
    const ConstPtrs p = row_consts(op, c, (size_t)f.NT * 16, s.N, [](int n) { return n; }); // padded to 16-column tiles
    f.A = p.A, f.S = p.S, f.Kc = p.Kc, f.wzp = p.wzp;
    epi_fields_izp(f, op, c);
    op.fast = OpImpl::CONV_GEMM;
    op.rt_wz = wz;
    op.fast_name = std::string("conv_gemm_rt") + (c.dw ? (wz ? "<dw,wzp>" : "<dw>") : (wz ? "<wzp>" : ""));
    if (switches().verbose)
        fprintf(stderr, "[microflow_amd] conv_gemm_rt %dx%dx%d -> %d %dx%d: K' %d (%d k steps), %d tiles in %d slice(s) of %d, %s %d x %d rows, %d B LDS\n",
                s.H, s.W, s.C, s.N, s.KH, s.KW, s.KH * f.KWCP, f.KS, f.NT, f.NSL, f.NTS, f.NBANDS > 1 ? "bands of" : "images per step:",
                f.NBANDS > 1 ? f.BH : f.G, f.RB, f.lds);
    return true;
}

using Route = bool (*)(OpImpl &, const ConvCtx &);
// The order is the contract: every shape keeps the kernel it had.
const Route TABLE_ROUTES[] = {route_dw_table, route_dw_stem, route_dw_stem_rt, route_dw_c1, route_pw_mfma}; // the first whose condition holds
const Route RT_ROUTES[] = {route_dw_rt, route_pw_rt, route_conv_rows, route_dw_mm, route_dw_gemm, route_conv_mm, route_conv1x1_row,
                           route_conv_gemm}; // each one, in turn

void create_conv(OpImpl &op, OpSpec &s, I8Domain &dom, int lo, int hi, int xr) {
    const bool dw = s.kind == MF_OP_DEPTHWISE_CONV_2D;
    if (s.H <= 0 || s.W <= 0 || s.C <= 0 || s.N <= 0 || s.KH <= 0 || s.KW <= 0 || s.OH <= 0 ||
        s.OW <= 0 || s.sh <= 0 || s.sw <= 0 || s.nq <= 0 || s.nc1 <= 0 || !s.weights || !s.wzp ||
        !s.c0 || !s.c1)
        fail(MF_ERR_INVALID_ARG, "conv: bad arguments");
    if (s.pad == MF_PAD_VALID &&
        ((s.OH - 1) * s.sh + s.KH > s.H || (s.OW - 1) * s.sw + s.KW > s.W))
        fail(MF_ERR_INVALID_ARG, "conv: VALID view leaves the input (the reference would panic, src/tensor.rs:223)");
    op.in_elems = (size_t)s.H * s.W * s.C;
    op.out_elems = (size_t)s.OH * s.OW * s.N;
    dom.apply(s, dw ? (size_t)s.KH * s.KW * s.N : (size_t)s.N * s.KH * s.KW * s.C);
    const ConvCtx c = prepare_conv(op, s, dw, lo, hi, xr);
    for (Route r : TABLE_ROUTES)
        if (r(op, c)) break;
    for (Route r : RT_ROUTES) r(op, c);
    if (op.fma_ok) { // the single-fma constants beside the two-rounding ones, in the blocks of the kernels that have the form
        op.dwf.A3 = op.pw.A3 = op.d_A3.as<float>(), op.dwf.S3 = op.pw.S3 = op.d_S3.as<float>();
        op.dwf.Kc3 = op.pw.Kc3 = op.d_Kc3.as<int>();
        op.dwf.npatch3 = op.pw.npatch3 = op.fma_patch.n;
        if (op.fast == OpImpl::DW_STEM && op.fma_strict()) {
            for (int ch = 0; ch < 8; ++ch) op.stem.A3[ch] = op.h_A3[(size_t)ch], op.stem.S3[ch] = op.h_S3[(size_t)ch], op.stem.Kc3[ch] = op.h_Kc3[(size_t)ch];
            op.stem.fma_ok = 1;
        }
    }
    if (switches().verbose)
        fprintf(stderr, "[microflow_amd] %s %dx%dx%d -> %d: kernel %s, worst-case |acc| %lld%s\n",
                dw ? "depthwise_conv_2d" : "conv_2d", s.H, s.W, s.C, s.N,
                op.fast != OpImpl::NONE ? op.fast_name.c_str() : op.generic_name.c_str(),
                (long long)c.acc_bound, op.fast == OpImpl::NONE || !c.magic ? "" : c.magic == 2 ? " (bit-pattern int->f32, saturating pack)" : " (bit-pattern int->f32)");
}

void create_pool(OpImpl &op, const OpSpec &s, int lo, int hi, int xr) {
    const bool mx = s.kind == MF_OP_MAX_POOL_2D;
    const std::string nm = mx ? "max_pool_2d" : "average_pool_2d";
    if (s.H <= 0 || s.W <= 0 || s.C <= 0 || s.KH <= 0 || s.KW <= 0 || s.OH <= 0 || s.OW <= 0 ||
        s.sh <= 0 || s.sw <= 0)
        fail(MF_ERR_INVALID_ARG, nm + ": bad arguments");
    if (mx && h_pool_window_empty(s.H, s.W, s.KH, s.KW, s.sh, s.sw, s.pad == MF_PAD_SAME, s.OH, s.OW))
        fail(MF_ERR_INVALID_ARG, nm + ": a window has no in-bounds tap");
    if (s.pad == MF_PAD_VALID &&
        ((s.OH - 1) * s.sh + s.KH > s.H || (s.OW - 1) * s.sw + s.KW > s.W))
        fail(MF_ERR_INVALID_ARG, nm + ": VALID view leaves the input");
    op.in_elems = (size_t)s.H * s.W * s.C;
    op.out_elems = (size_t)s.OH * s.OW * s.C;
    k::PoolArgs &a = op.pool;
    a.H = s.H, a.W = s.W, a.C = s.C, a.KH = s.KH, a.KW = s.KW, a.sh = s.sh, a.sw = s.sw;
    a.OH = s.OH, a.OW = s.OW, a.pad_same = s.pad == MF_PAD_SAME;
    a.c0 = s.pool_c0, a.c1 = s.pool_c1, a.lo = lo, a.hi = hi;
    a.bias = s.u8 ? 128 : 0, a.xr = xr;
    a.sat_lo = s.u8 ? 0.0f : -128.0f, a.sat_hi = s.u8 ? 255.0f : 127.0f;
    op.generic_name = mx ? "maxpool_generic" : "avgpool_generic";
    // 4 channels per thread, dword loads
    if (s.C % 4 == 0) op.fast = mx ? OpImpl::MAXPOOL_C4 : OpImpl::POOL_C4, op.fast_name = mx ? "maxpool_c4" : "avgpool_c4";
}

void create_fc(OpImpl &op, OpSpec &s, I8Domain &dom, int lo, int hi, int xr) {
    if (s.M <= 0 || s.K <= 0 || s.N <= 0 || !s.weights || !s.c0 || !s.c2)
        fail(MF_ERR_INVALID_ARG, "fully_connected: bad arguments");
    const int beta = s.u8 ? 128 : 0;
    op.in_elems = (size_t)s.M * s.K;
    op.out_elems = (size_t)s.M * s.N;
    const int wzp_t = s.wzp ? s.wzp[0] : 0; // in T's domain
    if (!s.wzp) s.nq = 0;
    dom.apply(s, (size_t)s.N * s.K);
    std::vector<float> A(s.N);
    std::vector<int32_t> Kc(s.N);
    for (int j = 0; j < s.N; ++j) {
        volatile float a = (float)s.ozp + s.c0[j];
        A[j] = a;
        Kc[j] = wrap_sub(s.c3, s.c2[j]); // acc = x0 - x1 - c2[j] + c3
        if (s.u8) {
            // with x = x' + 128, w = w' + 128:  x0 - x1 = sum x'w' - (wzp - 128) sum x'
            //                                   + 128 sum_k w'[j][k] + K 128 (128 - wzp)
            int32_t ws = 0;
            for (int k = 0; k < s.K; ++k) ws = wrap_add(ws, s.weights[(size_t)j * s.K + k]);
            Kc[j] = wrap_add(Kc[j], wrap_add(wrap_mul(beta, ws),
                                             wrap_mul(wrap_mul(s.K, beta), beta - wzp_t)));
        }
    }
    op.h_w.assign(s.weights, s.weights + (size_t)s.N * s.K);
    op.h_A = A, op.h_Kc = Kc; // (a fused group builds its own padded copies where the operator has no fc_rt image: fused.hip conv1_fc)
    op.d_w.upload(s.weights, (size_t)s.N * s.K);
    op.d_A.upload(A.data(), A.size() * 4);
    op.d_Kc.upload(Kc.data(), Kc.size() * 4);
    k::FcArgs &a = op.fc;
    a.K = s.K, a.N = s.N, a.wzp = wzp_t - beta, a.S = s.c1[0];
    a.lo_f = (float)lo, a.hi_f = (float)hi, a.xr = xr;
    a.w = op.d_w.as<int8_t>(), a.A = op.d_A.as<float>(), a.Kc = op.d_Kc.as<int>();
    op.generic_name = "fc_generic";
    const bool finite = all_finite(A) && std::isfinite(a.S);
    if (!finite) {
        // degenerate constants: the generic kernel reproduces Rust's NaN -> 0 cast
    } else if (s.K % 16 == 0 && s.K >= 256 && (s.N == 1 || s.N == 2 || s.N == 4 || s.N == 8)) {
        op.fast = OpImpl::FC_ROWWAVE;
        op.fast_name = "fc_rowwave<" + std::to_string(s.N) + ">";
    } else if (s.N % 128 == 0 && s.K % 128 == 0) {
        // dense contraction: int8 MFMA GEMM whenever the batch supplies whole 128-row tiles; weights with at most two non-zero
        // bytes in every aligned group of four along K (judged on the stored i8 bytes) on the sparse matrix instruction
        op.fast = OpImpl::FC_MFMA;
        op.fast_name = "fc_mfma";
        if (!switches().no_fc_sparse && k::fc_sparse24_eligible(s.weights, s.N, s.K)) {
            const std::vector<int8_t> img = k::fc_sparse24_image(s.weights, s.N, s.K);
            op.d_sp24.upload(img.data(), img.size());
            op.fast = OpImpl::FC_SPARSE24;
            op.fast_name = a.wzp ? "fc_sparse24<wzp>" : "fc_sparse24";
        }
    }
    if (finite && (op.fast == OpImpl::NONE || op.fast == OpImpl::FC_ROWWAVE) && k::fc_rt_plan(op.fcrt, s.K, s.N)) {
        // every other shape: the int8 matrix pipe with the (sliced) weight image resident in LDS.  The image and constants are
        // built for every such operator: a fused FullyConnected chain (fc_chain) takes them from its members.  (A row-wave shape
        // gets them too and keeps its kernel: behind a global pool it is a layer of pool_fc_chain, fused.hip.)
        k::FcRtArgs &f = op.fcrt;
        const std::vector<int8_t> img = k::fc_rt_weight_image(s.weights, s.K, s.N);
        std::vector<float> pA((size_t)f.NT * 16, 0.0f);
        std::vector<int32_t> pK((size_t)f.NT * 16, 0);
        // epilogue mode (k_common.hpp): |acc| <= 128 sum_k |w - wzp| + |Kc| in the i8 domain, exactly, over every input
        int64_t bound = 0;
        double xmax = 0.0;
        for (int j = 0; j < s.N; ++j) {
            int64_t b = std::abs((int64_t)Kc[(size_t)j]);
            for (int k = 0; k < s.K; ++k) b += 128 * std::abs((int64_t)s.weights[(size_t)j * s.K + k] - a.wzp);
            bound = std::max(bound, b);
            xmax = std::max(xmax, std::fabs((double)A[(size_t)j]) + std::fabs((double)a.S) * (double)b);
            pA[(size_t)j] = A[(size_t)j], pK[(size_t)j] = Kc[(size_t)j];
        }
        int magic = !switches().no_magic && bound < (1 << 22) ? 1 : 0;
        if (magic && !switches().no_sat_pack && lo == (s.u8 ? 0 : -128) && hi == (s.u8 ? 255 : 127) && xmax < 30000.0) magic = 2;
        if (switches().debug_epi)
            fprintf(stderr, "[epi] fully_connected %dx%d -> %d: |acc| <= %lld -> mode %d\n", s.M, s.K, s.N, (long long)bound, magic);
        op.d_fcw.upload(img.data(), img.size());
        op.d_fcA.upload(pA.data(), pA.size() * 4);
        op.d_fcKc.upload(pK.data(), pK.size() * 4);
        f.wimg = op.d_fcw.p, f.A = op.d_fcA.as<float>(), f.Kc = op.d_fcKc.as<int>();
        f.S = a.S, f.lo_f = a.lo_f, f.hi_f = a.hi_f, f.wzp = a.wzp, f.magic = magic, f.xr = xr;
        op.fcrt_ok = true;
        // (At most one 16 x 16 weight tile of work per row -- sine.tflite's 1 -> 16 -> 16 -> 1 -- stays on fc_generic when it
        // runs alone, which moves the same bytes without the staging latency: fc_rt was 11 % slower on sine at 65 536 rows,
        // scripts/time_fc_rt.py.  In a chain those layers run inside fc_chain.)
        if (op.fast == OpImpl::NONE && (long long)s.K * s.N > 256 && !switches().no_fc_rt) {
            op.fast = OpImpl::FC_RT;
            op.fast_name = a.wzp ? "fc_rt<wzp>" : "fc_rt";
        }
    }
}

void create_softmax(OpImpl &op, const OpSpec &s, int xr) {
    if (s.M <= 0 || s.N <= 0) fail(MF_ERR_INVALID_ARG, "softmax: bad arguments");
    op.in_elems = op.out_elems = (size_t)s.M * s.N;
    // exp table over the 256 possible int8 inputs: expf(f32(q) * input.scale[0])
    // (src/ops/softmax.rs:20-21), libm's algorithm evaluated on the host
    // (entry = stored byte + 128, which is q + 128 for i8 and q itself for u8)
    std::vector<float> table(256);
    h_softmax_table(s.in_scale, s.u8, table.data());
    op.d_table.upload(table.data(), 256 * 4);
    k::SoftmaxArgs &a = op.sm;
    a.rows = s.M, a.cols = s.N, a.oscale = s.oscale, a.ozp_f = (float)s.ozp;
    a.exp_table = op.d_table.as<float>();
    a.sat_lo = s.u8 ? 0.0f : -128.0f, a.sat_hi = s.u8 ? 255.0f : 127.0f, a.xr = xr;
    op.generic_name = "softmax_table";
}

// ADD: no weights; the constants of both domains the operator is run in (kernels.hpp: AddArgs)
void create_add(OpImpl &op, const OpSpec &s, int lo, int hi) {
    if (!s.add_elems) fail(MF_ERR_INVALID_ARG, "add: bad arguments");
    op.in_elems = op.in2_elems = op.out_elems = s.add_elems;
    k::AddArgs &a = op.add;
    const int off = s.u8 ? 0 : 128;
    a.ca = s.join_ca, a.cb = s.join_cb, a.ka = (float)(off + s.join_za), a.kb = (float)(off + s.join_zb);
    a.zo_f = (float)s.ozp, a.lo_f = (float)lo, a.hi_f = (float)hi; // (act_bounds: [lo, hi] lies inside T's range)
    op.add_fma = h_add_fma_form(a.ca, a.cb, off + s.join_za, off + s.join_zb, s.ozp, lo, hi, &a.k1);
    a.xin4 = 0x80808080u, a.xout4 = s.u8 ? 0x80808080u : 0u;
    op.add_ext = a;
    if (s.u8) op.add_ext.xin4 = op.add_ext.xout4 = 0u; // real u8 bytes
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, op.device) != hipSuccess) (void)hipGetLastError(), cus = 0;
    op.cus = cus;
    op.generic_name = "add_generic";
    op.fast = OpImpl::ADD_C16, op.fast_name = op.add_fma ? "add_c16<fma>" : "add_c16"; // taken where all three pointers are 16-byte aligned
}

// CONCATENATION: no weights; the constants of both domains the operator is run in (kernels.hpp: ConcatArgs).  No activation: the
// clamp is T's range
void create_concat(OpImpl &op, const OpSpec &s) {
    if (!s.cat_rows || s.cat_ca <= 0 || s.cat_cb <= 0 || (long long)s.cat_ca + s.cat_cb > 0x7fffffffll) fail(MF_ERR_INVALID_ARG, "concatenation: bad arguments");
    if (s.cat_rows > (~(size_t)0 >> 2) / ((size_t)s.cat_ca + (size_t)s.cat_cb)) fail(MF_ERR_INVALID_ARG, "concatenation: bad arguments");
    op.in_elems = s.cat_rows * (size_t)s.cat_ca, op.in2_elems = s.cat_rows * (size_t)s.cat_cb;
    op.out_elems = op.in_elems + op.in2_elems;
    k::ConcatArgs &a = op.cat;
    const int off = s.u8 ? 0 : 128;
    a.ca = s.join_ca, a.cb = s.join_cb, a.ka = (float)(off + s.join_za), a.kb = (float)(off + s.join_zb);
    a.zo_f = (float)s.ozp, a.lo_f = s.u8 ? 0.0f : -128.0f, a.hi_f = s.u8 ? 255.0f : 127.0f;
    a.xin4 = 0x80808080u, a.xout4 = s.u8 ? 0x80808080u : 0u;
    a.Ca = s.cat_ca, a.Cb = s.cat_cb, a.copy_a = s.cat_copy_a, a.copy_b = s.cat_copy_b;
    op.cat_ext = a;
    if (s.u8) op.cat_ext.xin4 = op.cat_ext.xout4 = 0u; // real u8 bytes
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, op.device) != hipSuccess) (void)hipGetLastError(), cus = 0;
    op.cus = cus;
    op.generic_name = "concat_generic";
    // the widest word that divides both slices; the pointers may narrow it at run time (op_run2)
    const int both = s.cat_ca | s.cat_cb;
    op.cat_unit = both % 16 == 0 ? 16 : both % 8 == 0 ? 8 : both % 4 == 0 ? 4 : 0;
    if (op.cat_unit) op.fast = OpImpl::CONCAT_C4, op.fast_name = op.cat_unit == 16 ? "concat_c4<v16>" : op.cat_unit == 8 ? "concat_c4<v8>" : "concat_c4";
}

// PAD: no weights, no constants; the fill byte is the input zero point as the kernels see stored bytes (u8: the internal domain)
void create_pad(OpImpl &op, const OpSpec &s) {
    const int t = s.pads[0], b = s.pads[1], l = s.pads[2], r = s.pads[3];
    if (s.H <= 0 || s.W <= 0 || s.C <= 0 || t < 0 || b < 0 || l < 0 || r < 0) fail(MF_ERR_INVALID_ARG, "pad: bad arguments");
    const long long OH = (long long)s.H + t + b, OW = (long long)s.W + l + r;
    if (OH != s.OH || OW != s.OW || OW * s.C > 0x7fffffffll || OH > 0x7fffffffll) fail(MF_ERR_INVALID_ARG, "pad: the output shape is not input + pads");
    if (s.izp < (s.u8 ? 0 : -128) || s.izp > (s.u8 ? 255 : 127)) fail(MF_ERR_INVALID_ARG, "pad: the zero point is no value of T");
    op.in_elems = (size_t)s.H * s.W * s.C;
    op.out_elems = (size_t)OH * (size_t)OW * s.C;
    k::PadArgs &a = op.padargs;
    a.H = s.H, a.OH = (int)OH, a.top = t, a.in_row = s.W * s.C, a.out_row = (int)OW * s.C, a.lp = l * s.C;
    a.fill4 = 0x01010101u * (uint32_t)(uint8_t)(s.u8 ? s.izp ^ 0x80 : s.izp);
    op.generic_name = "pad_generic";
    // whole words in every row segment: dwords with C % 4 == 0; 16 bytes where the image row and both fills are multiples of 16
    if (s.C % 4 == 0) {
        op.pad_unit = (a.in_row % 16 == 0 && a.lp % 16 == 0 && a.out_row % 16 == 0) ? 16 : 4;
        op.fast = OpImpl::PAD_C4, op.fast_name = op.pad_unit == 16 ? "pad_c4<v16>" : "pad_c4";
    }
}

} // namespace

OpImpl *op_create_padded_conv(const OpImpl *conv, int Hin, int Win, int padt, int padl) {
    const OpSpec &q = conv->s;
    const bool dw = q.kind == MF_OP_DEPTHWISE_CONV_2D;
    if ((q.kind != MF_OP_CONV_2D && !dw) || q.pad != MF_PAD_VALID || Hin <= 0 || Win <= 0 || padt < 0 || padl < 0 || Hin + padt > q.H ||
        Win + padl > q.W || conv->h_w.empty())
        return nullptr;
    MF_HIP(hipSetDevice(conv->device));
    std::unique_ptr<OpImpl> op(new OpImpl);
    op->device = conv->device;
    op->s = q;
    op->s.H = Hin, op->s.W = Win;
    op->s.weights = conv->h_w.data(); // (i8 domain, as uploaded: what the image builders read; cleared again below)
    op->in_elems = (size_t)Hin * Win * q.C, op->out_elems = conv->out_elems;
    op->h_A = conv->h_A, op->h_S = conv->h_S, op->h_Kc = conv->h_Kc, op->h_wzp = conv->h_wzp;
    op->finite_consts = conv->finite_consts, op->magic_mode = conv->magic_mode;
    op->conv = conv->conv; // the borrowed device arrays (w, wzp, A, S, Kc), the clamp, the input zero point
    op->conv.H = Hin, op->conv.W = Win;
    op->generic_name = "(none)";
    ConvCtx c{op->s, dw, op->h_A, op->h_S, op->h_Kc, op->h_wzp};
    c.lo = (int)conv->conv.lo_f, c.hi = (int)conv->conv.hi_f, c.xr = conv->conv.xr;
    c.magic = conv->magic_mode, c.finite = conv->finite_consts;
    c.wz = !all_zero(c.wzp), c.zero_wzp = !c.wz && c.finite;
    c.padt = padt, c.padl = padl, c.rows_bytes_any_c = true;
    // the run-time-geometry routes that take a window placement, in create_conv's order; the two-rounding epilogue (no single-fma form)
    for (Route r : {route_conv_rows, route_dw_mm, route_dw_gemm, route_conv_mm, route_conv_gemm}) r(*op, c);
    op->s.weights = nullptr, op->s.wzp = nullptr, op->s.c0 = op->s.c1 = nullptr, op->s.c2 = nullptr;
    if (op->fast == OpImpl::NONE) return nullptr;
    return op.release();
}

OpImpl *op_create(int device, const OpSpec &spec) {
    dev_require(device);
    std::unique_ptr<OpImpl> op(new OpImpl);
    op->device = device;
    OpSpec s = spec;
    I8Domain dom; // (outlives the creators: `s` points into it for a u8 operator)
    const int xr = s.u8 ? 0x80 : 0;
    int lo, hi;
    act_bounds(s.act, s.oscale, s.ozp, s.u8, lo, hi);

    switch (s.kind) {
    case MF_OP_CONV_2D:
    case MF_OP_DEPTHWISE_CONV_2D: create_conv(*op, s, dom, lo, hi, xr); break;
    case MF_OP_AVERAGE_POOL_2D:
    case MF_OP_MAX_POOL_2D: create_pool(*op, s, lo, hi, xr); break;
    case MF_OP_FULLY_CONNECTED: create_fc(*op, s, dom, lo, hi, xr); break;
    case MF_OP_SOFTMAX: create_softmax(*op, s, xr); break;
    case MF_OP_ADD: create_add(*op, s, lo, hi); break;
    case MF_OP_CONCATENATION: create_concat(*op, s); break;
    case MF_OP_PAD: create_pad(*op, s); break;
    default: fail(MF_ERR_UNSUPPORTED, "unsupported operator kind " + std::to_string(s.kind));
    }
    op->s = s;
    // the spec's host pointers die with the caller
    op->s.weights = nullptr, op->s.wzp = nullptr, op->s.c0 = op->s.c1 = nullptr, op->s.c2 = nullptr;
    return op.release();
}

void op_destroy(OpImpl *op) {
    if (!op) return;
    (void)hipSetDevice(op->device);
    if (op->scratch_ev) {
        (void)hipEventSynchronize(op->scratch_ev);
        (void)hipEventDestroy(op->scratch_ev);
    }
    if (op->d_rowsum) (void)hipFree(op->d_rowsum);
    if (op->d_ext) (void)hipFree(op->d_ext);
    delete op;
}

size_t op_in_elems(const OpImpl *op) { return op->in_elems; }
size_t op_in2_elems(const OpImpl *op) { return op->in2_elems; }
size_t op_out_elems(const OpImpl *op) { return op->out_elems; }
const char *op_kernel_name(const OpImpl *op) {
    return (op->fast != OpImpl::NONE && !op->force_generic) ? op->fast_name.c_str()
                                                             : op->generic_name.c_str();
}
void op_set_generic(OpImpl *op, bool g) { op->force_generic = g; }
// the layer-wise kernels that have the single-fma epilogue (k_common.hpp mode 3): the matrix-pipe depthwise, the MFMA pointwise, the stem
static bool op_runs_fma(const OpImpl *op) {
    if (!op->fma_strict()) return false; // (the layer-wise kernels have no patch support)
    const OpSpec &sp = op->s;
    const bool stem_valu = switches().stem_valu;
    return (op->fast == OpImpl::DW_NHWC && dw_taps_on_matrix_pipe() && op->dwf.wmm && k::dw_mm_name(sp.H, sp.W, sp.C, sp.sh)) ||
           op->fast == OpImpl::PW_MFMA || (op->fast == OpImpl::DW_STEM && !stem_valu);
}
int op_epilogue_mode(const OpImpl *op) { // of the operator's own (layer-wise) launch; -1: not a convolution-like operator
    if (op->s.kind != MF_OP_CONV_2D && op->s.kind != MF_OP_DEPTHWISE_CONV_2D) return -1;
    return op_runs_fma(op) ? 3 : op->magic_mode;
}
bool op_has_fma_epilogue(const OpImpl *op) { return op->fma_ok; }
int op_fma_patches(const OpImpl *op) { return op->fma_ok ? op->fma_patch.n : -1; }

void op_run(OpImpl *op, const int8_t *d_in, size_t batch, int8_t *d_out, void *stream) {
    if (!batch) return;
    if (!d_in || !d_out) fail(MF_ERR_INVALID_ARG, "op_run: null device pointer");
    if (op->s.kind == MF_OP_ADD) fail(MF_ERR_INVALID_ARG, "op_run: an ADD has two inputs (mf_op_run2)");
    if (op->s.kind == MF_OP_CONCATENATION) fail(MF_ERR_INVALID_ARG, "op_run: a CONCATENATION has two inputs (mf_op_run2)");
    hipStream_t s = (hipStream_t)stream;
    const OpSpec &sp = op->s;
    // the fast kernels move 4- and 16-byte words (vector loads, LDS-DMA, packed stores): buffers that are not 16-byte
    // aligned -- an offset into a larger allocation handed to mf_op_run -- take the byte-wise shape-generic kernels
    const bool aligned = (((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0;
    const bool fast = op->fast != OpImpl::NONE && !op->force_generic && aligned;
    bool done = false;
    if (fast) {
        if (batch > 0x7fffffffull / 4) fail(MF_ERR_INVALID_ARG, "batch too large for one launch");
        switch (op->fast) {
        case OpImpl::DW_NHWC: {
            k::DwFastArgs f3 = op->dwf;
            const bool fma = op_runs_fma(op) && f3.use_fma();
            done = (dw_taps_on_matrix_pipe() && k::launch_dw_mm(sp.H, sp.W, sp.C, sp.sh, d_in, d_out, fma ? f3 : op->dwf, (int)batch, s)) ||
                   k::launch_dw_fast(sp.H, sp.W, sp.C, sp.sh, d_in, d_out, op->dwf, (int)batch, s);
            break;
        }
        case OpImpl::DW_STEM: {
            k::DwStemArgs f3 = op->stem;
            const bool fma = op_runs_fma(op) && f3.use_fma();
            done = k::launch_dw_stem(sp.H, sp.W, sp.N, sp.sh, d_in, d_out, fma ? f3 : op->stem, (int)batch, s);
            break;
        }
        case OpImpl::DW_STEM_RT:
            k::launch_dw_stem_rt(d_in, d_out, op->stemrt, (int)batch, s);
            done = true;
            break;
        case OpImpl::CONV1X1_ROW:
            k::launch_conv1x1_rowwave(d_in, d_out, op->conv, batch, s);
            done = true;
            break;
        case OpImpl::POOL_C4:
            k::launch_avgpool_c4(d_in, d_out, op->pool, batch, s);
            done = true;
            break;
        case OpImpl::MAXPOOL_C4:
            k::launch_maxpool_c4(d_in, d_out, op->pool, batch, s);
            done = true;
            break;
        case OpImpl::PAD_C4:
            k::launch_pad_c4(d_in, d_out, op->padargs, batch, op->pad_unit, s);
            done = true;
            break;
        case OpImpl::DW_C1:
            k::launch_dw_c1(d_in, d_out, op->dwc1, batch, s);
            done = true;
            break;
        case OpImpl::PW_MFMA: {
            k::PwArgs f3 = op->pw;
            const bool fma = op_runs_fma(op) && f3.use_fma();
            done = k::launch_pw(sp.C, sp.N, d_in, d_out, fma ? f3 : op->pw, (long long)batch * sp.H * sp.W, s);
            break;
        }
        case OpImpl::CONV_MM:
            if (op->cmm.dwise) k::launch_dw_mm(d_in, d_out, op->cmm, (int)batch, s);
            else k::launch_conv_mm(d_in, d_out, op->cmm, op->rt_wz, (int)batch, s);
            done = true;
            break;
        case OpImpl::CONV_ROWS:
            k::launch_conv_rows(d_in, d_out, op->crows, op->rt_wz, (int)batch, s);
            done = true;
            break;
        case OpImpl::CONV_GEMM:
            k::launch_conv_gemm(d_in, d_out, op->cgm, op->rt_wz, (int)batch, s);
            done = true;
            break;
        case OpImpl::DW_GEMM:
            k::launch_dw_gemm(d_in, d_out, op->dwg, op->rt_wz, (int)batch, s);
            done = true;
            break;
        case OpImpl::DW_RT:
            k::launch_dw_rt(d_in, d_out, op->dwrt, sp.sh, op->rt_wz, (int)batch, s);
            done = true;
            break;
        case OpImpl::PW_RT: {
            // `pw_group` pixels are one row of the product; the few pixels left over when the pixel count is not a
            // multiple of it go through the shape-generic kernel as one short 1 x rem image
            const long long npix = (long long)batch * sp.H * sp.W, full = npix / op->pw_group * op->pw_group;
            if (full) k::launch_pw_rt(d_in, d_out, op->pwrt, op->rt_wz, full / op->pw_group, s);
            if (npix > full) {
                k::ConvArgs t = op->conv;
                t.H = t.OH = 1, t.W = t.OW = (int)(npix - full);
                k::launch_conv2d_generic(d_in + full * sp.C, d_out + full * sp.N, t, 1, s);
            }
            done = true;
            break;
        }
        case OpImpl::FC_ROWWAVE:
            done = k::launch_fc_rowwave(d_in, d_out, op->fc, batch * sp.M, s);
            break;
        case OpImpl::FC_RT:
            k::launch_fc_rt(d_in, d_out, op->fcrt, (long long)(batch * sp.M), s);
            done = true;
            break;
        case OpImpl::FC_MFMA:
        case OpImpl::FC_SPARSE24: {
            const size_t rows = batch * sp.M;
            if (!k::fc_mfma_supported(rows, sp.N, sp.K)) break; // fewer than 64 rows: generic kernel
            const bool sparse = op->fast == OpImpl::FC_SPARSE24;
            k::FcGemmArgs g{};
            g.w = sparse ? op->d_sp24.as<int8_t>() : op->fc.w, g.A = op->fc.A, g.Kc = op->fc.Kc, g.wzp = op->fc.wzp, g.S = op->fc.S;
            g.lo_f = op->fc.lo_f, g.hi_f = op->fc.hi_f, g.M = (int)rows, g.N = sp.N, g.K = sp.K;
            g.xr4 = 0x01010101u * (uint32_t)op->fc.xr;
            g.rowsum = nullptr, g.rs_sums = nullptr, g.rs_sync = nullptr;
            // the weight-zero-point term needs sum_k x[m][k]: formed by the GEMM launch itself (its prologue) where the shape
            // allows, else by a pre-pass launch; either way in the operator's one row-sum scratch (+ the row tiles' counter pairs
            // behind it), whose uses the event handshake serialises across streams
            // (fc_sparse24 always takes the pre-pass)
            const bool inlaunch = op->fc.wzp != 0 && !sparse && k::fc_mfma_rowsum_prologue(rows, sp.N);
            const bool prepass = op->fc.wzp != 0 && (inlaunch || sparse || k::fc_mfma_rowsum_prepass());
            if (prepass) {
                const size_t ntm = (rows + 255) / 256, need = rows + 2 * ntm;
                op->scratch_acquire(s, op->rowsum_cap < need);
                if (op->rowsum_cap < need) {
                    if (op->d_rowsum) (void)hipFree(op->d_rowsum);
                    op->d_rowsum = nullptr, op->rowsum_cap = 0;
                    MF_HIP(hipMalloc((void **)&op->d_rowsum, need * sizeof(int)));
                    MF_HIP(hipMemset(op->d_rowsum, 0, need * sizeof(int))); // (the counter pairs start at zero and every launch leaves them so)
                    op->rowsum_cap = need;
                    op->rowsum_rows = 0;
                }
                if (inlaunch && op->rowsum_rows != rows) { // the counters sit behind the sums of THIS row count
                    if (op->rowsum_rows) {
                        MF_HIP(hipMemsetAsync(op->d_rowsum, 0, op->rowsum_cap * sizeof(int), s));
                        ++k::launches_enqueued; // (a device-side fill)
                    }
                    op->rowsum_rows = rows;
                }
                if (inlaunch) g.rs_sums = op->d_rowsum, g.rs_sync = op->d_rowsum + rows;
                else k::launch_fc_rowsum(d_in, op->d_rowsum, rows, sp.K, s), g.rowsum = op->d_rowsum;
            }
            if (sparse) k::launch_fc_sparse24(d_in, d_out, g, s);
            else k::launch_fc_mfma(d_in, d_out, g, s);
            if (prepass) op->scratch_release(s);
            done = true;
            break;
        }
        default: break;
        }
    }
    if (!done) {
        switch (sp.kind) {
        case MF_OP_CONV_2D: k::launch_conv2d_generic(d_in, d_out, op->conv, batch, s); break;
        case MF_OP_DEPTHWISE_CONV_2D: k::launch_dwconv_generic(d_in, d_out, op->conv, batch, s); break;
        case MF_OP_AVERAGE_POOL_2D: k::launch_avgpool_generic(d_in, d_out, op->pool, batch, s); break;
        case MF_OP_MAX_POOL_2D: k::launch_maxpool_generic(d_in, d_out, op->pool, batch, s); break;
        case MF_OP_FULLY_CONNECTED: k::launch_fc_generic(d_in, d_out, op->fc, batch * sp.M, s); break;
        case MF_OP_SOFTMAX: k::launch_softmax(d_in, d_out, op->sm, batch, s); break;
        case MF_OP_PAD: k::launch_pad_generic(d_in, d_out, op->padargs, batch, s); break;
        default: fail(MF_ERR_UNSUPPORTED, "op_run: bad kind");
        }
    }
    MF_HIP(hipGetLastError());
}

// ADD.  The output may be exactly one of the inputs; add_c16 where all three pointers are 16-byte aligned, else the byte-wise kernel
// CONCATENATION.  The output overlaps neither input; concat_c4 on the widest word (16, 8, 4 bytes) that divides Ca, Cb and all three
// pointers, else the byte-wise kernel
static void run_concat(OpImpl *op, const int8_t *d_a, const int8_t *d_b, size_t batch, int8_t *d_out, void *stream, bool external) {
    if (!batch) return;
    if (!d_a || !d_b || !d_out) fail(MF_ERR_INVALID_ARG, "op_run2: null device pointer");
    if (batch > (~(size_t)0 >> 1) / op->out_elems) fail(MF_ERR_INVALID_ARG, "batch too large");
    const uintptr_t o = (uintptr_t)d_out, a = (uintptr_t)d_a, b = (uintptr_t)d_b;
    const size_t na = batch * op->in_elems, nb = batch * op->in2_elems, no = batch * op->out_elems;
    if ((a < o + no && o < a + na) || (b < o + no && o < b + nb)) fail(MF_ERR_INVALID_ARG, "op_run2: the output overlaps an input");
    if (external) MF_HIP(hipSetDevice(op->device));
    hipStream_t s = (hipStream_t)stream;
    const k::ConcatArgs &p = external ? op->cat_ext : op->cat;
    const size_t rows = batch * op->s.cat_rows;
    const uintptr_t bits = a | b | o;
    int unit = op->force_generic ? 0 : op->cat_unit;
    while (unit && (bits & (uintptr_t)(unit - 1))) unit = unit > 4 ? unit / 2 : 0;
    if (unit) k::launch_concat_c4(d_a, d_b, d_out, p, rows, unit, op->cus, s);
    else k::launch_concat_generic(d_a, d_b, d_out, p, rows, s);
    MF_HIP(hipGetLastError());
}

void op_run2(OpImpl *op, const int8_t *d_a, const int8_t *d_b, size_t batch, int8_t *d_out, void *stream, bool external) {
    if (op->s.kind == MF_OP_CONCATENATION) return run_concat(op, d_a, d_b, batch, d_out, stream, external);
    if (op->s.kind != MF_OP_ADD) fail(MF_ERR_INVALID_ARG, "op_run2: the operator has one input (mf_op_run)");
    if (!batch) return;
    if (!d_a || !d_b || !d_out) fail(MF_ERR_INVALID_ARG, "op_run2: null device pointer");
    if (batch > (~(size_t)0 >> 1) / op->in_elems) fail(MF_ERR_INVALID_ARG, "batch too large");
    const size_t n = batch * op->in_elems;
    const uintptr_t o = (uintptr_t)d_out;
    for (const int8_t *in : {d_a, d_b}) {
        const uintptr_t i = (uintptr_t)in;
        if (i != o && i < o + n && o < i + n) fail(MF_ERR_INVALID_ARG, "op_run2: the output partly overlaps an input");
    }
    if (external) MF_HIP(hipSetDevice(op->device));
    hipStream_t s = (hipStream_t)stream;
    const k::AddArgs &a = external ? op->add_ext : op->add;
    const bool aligned = (((uintptr_t)d_a | (uintptr_t)d_b | o) & 15) == 0;
    if (aligned && !op->force_generic) k::launch_add_c16(d_a, d_b, d_out, a, n, op->cus, op->add_fma, s);
    else k::launch_add_generic(d_a, d_b, d_out, a, n, s);
    MF_HIP(hipGetLastError());
}

// The C ABI's mf_op_run: a u8 operator takes and returns real u8 bytes.
void op_run_external(OpImpl *op, const int8_t *d_in, size_t batch, int8_t *d_out, void *stream) {
    if (op->s.kind == MF_OP_ADD) fail(MF_ERR_INVALID_ARG, "op_run: an ADD has two inputs (mf_op_run2)");
    if (op->s.kind == MF_OP_CONCATENATION) fail(MF_ERR_INVALID_ARG, "op_run: a CONCATENATION has two inputs (mf_op_run2)");
    MF_HIP(hipSetDevice(op->device)); // the operator's buffers and kernels live on its device
    if (!op->s.u8) return op_run(op, d_in, batch, d_out, stream);
    if (!batch) return;
    if (!d_in || !d_out) fail(MF_ERR_INVALID_ARG, "op_run: null device pointer");
    hipStream_t s = (hipStream_t)stream;
    const size_t n_in = batch * op->in_elems;
    // (two scratch buffers may be in play -- d_ext here, d_rowsum inside op_run for an FC with a weight zero point -- behind one
    // event: op_run's own acquire then waits for nothing new, its release is superseded by the one below)
    op->scratch_acquire(s, op->ext_cap < n_in);
    if (op->ext_cap < n_in) {
        if (op->d_ext) (void)hipFree(op->d_ext);
        op->d_ext = nullptr, op->ext_cap = 0;
        MF_HIP(hipMalloc((void **)&op->d_ext, n_in + 256));
        op->ext_cap = n_in;
    }
    k::launch_xor80(d_in, op->d_ext, n_in, s);
    op_run(op, op->d_ext, batch, d_out, stream);
    op->scratch_release(s); // op_run's kernels were the last readers of d_ext
    k::launch_xor80(d_out, d_out, batch * op->out_elems, s);
    MF_HIP(hipGetLastError());
}

// Boundary quantisation fused into the first operator (M::predict on f32 input): only the stem
// kernel has an f32-input variant.  `zp` is a value of T.
// quant_div (k_common.hpp): true when the fast form gives the same byte as the true division for EVERY float input
static bool quant_div_verified(int device, float scale, float rcp, float zp_f, float sat_lo, float sat_hi) {
    const bool off = switches().no_fast_quant_div;
    if (off || !std::isfinite(scale) || !std::isfinite(rcp) || scale == 0.0f) return false;
    static std::mutex mu;
    static std::map<std::array<uint32_t, 4>, bool> cache;
    uint32_t kb[4];
    memcpy(&kb[0], &scale, 4), memcpy(&kb[1], &zp_f, 4), memcpy(&kb[2], &sat_lo, 4), memcpy(&kb[3], &sat_hi, 4);
    const std::array<uint32_t, 4> key{kb[0], kb[1], kb[2], kb[3]};
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    MF_HIP(hipSetDevice(device));
    const unsigned long long bad = k::verify_quant_div(scale, rcp, zp_f, sat_lo, sat_hi, nullptr);
    if (bad == ~0ull) return false; // the check itself could not run: keep the true division now, try again next time
    const bool ok = bad == 0;
    if (switches().verbose) fprintf(stderr, "[microflow_amd] boundary quantisation: 3-instruction division %s for scale %g\n", ok ? "verified" : "REJECTED", (double)scale);
    cache[key] = ok;
    return ok;
}
void edge_set_in(k::F32Edge &e, int device, float scale, int zp, bool u8) {
    e.in_scale = scale, e.in_zp_f = (float)zp;
    e.in_sat_lo = u8 ? 0.0f : -128.0f, e.in_sat_hi = u8 ? 255.0f : 127.0f;
    e.in_xr4 = u8 ? 0x80808080u : 0u;
    e.in_rcp = (float)(1.0 / (double)scale);
    e.in_fast = quant_div_verified(device, scale, e.in_rcp, e.in_zp_f, e.in_sat_lo, e.in_sat_hi) ? 1 : 0;
}
void edge_set_out(k::F32Edge &e, float scale, int zp, bool u8) {
    // f32(q) - f32(zp) with q = stored + 128: both small integers, so the shift moves to zp exactly (as dev_dequantize)
    e.out_scale = scale, e.out_zp_f = (float)(zp - (u8 ? 128 : 0));
}
thread_local unsigned long long k::launches_enqueued = 0;
unsigned long long &dev_launch_counter() { return k::launches_enqueued; }

bool op_set_input_quant(OpImpl *op, float scale, int zp, bool u8) {
    if (!(scale == scale)) return false;
    // fc_rt_f32 (k_fc_f32.hip), dw3x3_stem_rt_f32 and conv_rows_lds_f32 (k_rt.hip).  conv_rows_lds takes the floats only where a step is
    // one image (G == 1: more than 4096 dwords of image): with several small images per step its predict measured slower than the separate
    // pass (28x28x1, G = 8, +4 %), and conv_gemm_rt has no f32 instance for the same reason (224x224x3 in row bands, +12 %)
    // (conv_rows_bytes has no f32 instance: a float4 of its input is not a tile dword)
    const bool conv_rows_one_image = op->fast == OpImpl::CONV_ROWS && op->crows.G == 1 && !op->crows.BYTES();
    if ((op->fast == OpImpl::FC_RT || op->fast == OpImpl::DW_STEM_RT || conv_rows_one_image) && !switches().no_f32_boundary) {
        edge_set_in(op->edge, op->device, scale, zp, u8);
        op->accepts_f32 = true;
        return true;
    }
    if (op->fast != OpImpl::DW_STEM) return false;
    k::DwStemArgs &f = op->stem;
    f.in_scale = scale, f.in_zp_f = (float)zp;
    f.in_sat_lo = u8 ? 0.0f : -128.0f, f.in_sat_hi = u8 ? 255.0f : 127.0f;
    f.in_xr4 = u8 ? 0x80808080u : 0u;
    // the 3-instruction division of the boundary quantisation, if it is exact for these parameters (checked over all
    // 2^32 inputs on the device, a few ms, once per parameter set and process)
    f.in_rcp = (float)(1.0 / (double)scale);
    f.in_fast = quant_div_verified(op->device, scale, f.in_rcp, f.in_zp_f, f.in_sat_lo, f.in_sat_hi) ? 1 : 0;
    op->accepts_f32 = true;
    return true;
}
bool op_accepts_f32(const OpImpl *op) { return op->accepts_f32 && !op->force_generic; }
bool op_set_output_dequant(OpImpl *op, float scale, int zp, bool u8) {
    if (op->fast != OpImpl::FC_RT || switches().no_f32_boundary) return false;
    edge_set_out(op->edge, scale, zp, u8);
    op->emits_f32 = true;
    return true;
}
bool op_emits_f32(const OpImpl *op) { return op->emits_f32 && !op->force_generic; }
void op_run_f32(OpImpl *op, const void *d_in, bool in_f32, size_t batch, void *d_out, bool out_f32, void *stream) {
    if (!batch) return;
    if (!in_f32 && !out_f32) return op_run(op, (const int8_t *)d_in, batch, (int8_t *)d_out, stream);
    if (in_f32 && !op_accepts_f32(op)) fail(MF_ERR_UNSUPPORTED, "operator has no f32-input kernel");
    if (out_f32 && !op_emits_f32(op)) fail(MF_ERR_UNSUPPORTED, "operator has no f32-output kernel");
    if (!d_in || !d_out) fail(MF_ERR_INVALID_ARG, "op_run_f32: null device pointer");
    if ((in_f32 && ((uintptr_t)d_in & 15)) || (out_f32 && ((uintptr_t)d_out & 3))) fail(MF_ERR_INVALID_ARG, "op_run_f32: unaligned device pointer");
    if (batch > 0x7fffffffull / 4) fail(MF_ERR_INVALID_ARG, "batch too large for one launch");
    const OpSpec &sp = op->s;
    if (op->fast == OpImpl::DW_STEM_RT) { // (entry only: op_set_output_dequant refuses this kernel)
        MF_HIP(hipSetDevice(op->device));
        k::launch_dw_stem_rt((const int8_t *)d_in, (int8_t *)d_out, op->stemrt, (int)batch, (hipStream_t)stream, &op->edge);
        MF_HIP(hipGetLastError());
        return;
    }
    if (op->fast == OpImpl::CONV_ROWS) { // (entry only, as the stem)
        MF_HIP(hipSetDevice(op->device));
        k::launch_conv_rows((const int8_t *)d_in, (int8_t *)d_out, op->crows, op->rt_wz, (int)batch, (hipStream_t)stream, &op->edge);
        MF_HIP(hipGetLastError());
        return;
    }
    if (op->fast == OpImpl::FC_RT) {
        MF_HIP(hipSetDevice(op->device));
        k::launch_fc_rt_f32(d_in, d_out, op->fcrt, op->edge, (in_f32 ? k::EDGE_IN : 0) | (out_f32 ? k::EDGE_OUT : 0), (long long)(batch * sp.M),
                            (hipStream_t)stream);
        MF_HIP(hipGetLastError());
        return;
    }
    // (never the single-fma epilogue here: that form runs its kernel in round-toward-zero, and this kernel's boundary quantisation
    // needs round-to-nearest)
    if (!k::launch_dw_stem(sp.H, sp.W, sp.N, sp.sh, (const int8_t *)d_in, (int8_t *)d_out, op->stem, (int)batch,
                           (hipStream_t)stream, true))
        fail(MF_ERR_UNSUPPORTED, "f32 stem kernel missing");
    MF_HIP(hipGetLastError());
}

void dev_quantize(int device, const float *d_in, size_t n, float scale, int zp, bool u8, int8_t *d_out,
                  void *stream) {
    dev_require(device);
    if (!n) return;
    k::launch_quantize(d_in, d_out, n, scale, (float)zp, u8, (hipStream_t)stream);
    MF_HIP(hipGetLastError());
}
void dev_dequantize(int device, const int8_t *d_in, size_t n, float scale, int zp, bool u8, float *d_out,
                    void *stream) {
    dev_require(device);
    if (!n) return;
    // f32(q) - f32(zp) with q = stored + 128: both small integers, so the shift moves to zp exactly
    k::launch_dequantize(d_in, d_out, n, scale, (float)(zp - (u8 ? 128 : 0)), false, (hipStream_t)stream);
    MF_HIP(hipGetLastError());
}
void dev_dequantize_u8_raw(int device, const uint8_t *d_in, size_t n, float scale, int zp, float *d_out,
                           void *stream) {
    dev_require(device);
    if (!n) return;
    k::launch_dequantize((const int8_t *)d_in, d_out, n, scale, (float)zp, true, (hipStream_t)stream);
    MF_HIP(hipGetLastError());
}
void dev_xor80(int device, const int8_t *d_in, size_t n, int8_t *d_out, void *stream) {
    dev_require(device);
    if (!n) return;
    k::launch_xor80(d_in, d_out, n, (hipStream_t)stream);
    MF_HIP(hipGetLastError());
}
// the kernel's view of a validated description: windows [first, first + count)
static k::WinArgs win_args(const mf_windows &w, const WindowsGeom &g, size_t first, size_t count) {
    k::WinArgs a{};
    const size_t E = w.win_rows * w.win_row_elems;
    if (E > 0x7fffffffull) fail(MF_ERR_INVALID_ARG, "invalid window description: win_rows * win_row_elems is 2^31 or more");
    if (count > ~(size_t)0 / E) fail(MF_ERR_INVALID_ARG, "invalid window description: count * input_elems overflows");
    a.src_stride = w.n_sources > 1 ? w.src_stride : 0, a.src_pitch = w.src_pitch;
    a.hop_row_stride = w.hop_rows * w.src_pitch, a.hop_elems = w.hop_elems;
    a.ny = g.ny, a.nx = g.nx, a.first = first, a.total = count * E;
    a.E = (uint32_t)E, a.WE = (uint32_t)w.win_row_elems, a.WR = (uint32_t)w.win_rows;
    if (w.src_pitch == w.win_row_elems) a.WE = a.E, a.WR = 1; // the window's rows lie back to back: one run
    a.narrow = (first + count <= 0xffffffffull && a.total <= 0xffffffffull && g.nx <= 0xffffffffull && g.ny <= 0xffffffffull) ? 1 : 0;
    return a;
}
void dev_window_gather(int device, const void *d_src, const mf_windows &w, const WindowsGeom &g, size_t first, size_t count, bool flip80,
                       int8_t *d_dst, void *stream) {
    dev_require(device);
    if (!count) return;
    k::WinArgs a = win_args(w, g, first, count);
    a.xr4 = flip80 ? 0x80808080u : 0u;
    k::launch_window_gather(d_src, d_dst, a, (hipStream_t)stream);
    MF_HIP(hipGetLastError());
}
bool dev_quant_div_fast(int device, float scale, int zp, bool u8) {
    dev_require(device);
    return quant_div_verified(device, scale, (float)(1.0 / (double)scale), (float)zp, u8 ? 0.0f : -128.0f, u8 ? 255.0f : 127.0f);
}
void dev_window_gather_quantize(int device, const float *d_src, const mf_windows &w, const WindowsGeom &g, size_t first, size_t count,
                                float scale, int zp, bool u8, bool fast, bool flip80, int8_t *d_dst, void *stream) {
    dev_require(device);
    if (!count) return;
    k::WinArgs a = win_args(w, g, first, count);
    a.xr4 = flip80 ? 0x80808080u : 0u;
    a.scale = scale, a.rcp = (float)(1.0 / (double)scale), a.zp_f = (float)zp;
    a.sat_lo = u8 ? 0.0f : -128.0f, a.sat_hi = u8 ? 255.0f : 127.0f;
    a.fast = fast ? 1 : 0;
    k::launch_window_gather_quantize(d_src, d_dst, a, (hipStream_t)stream);
    MF_HIP(hipGetLastError());
}
void dev_synth_i8(int device, uint64_t seed, uint64_t first, size_t n, int8_t *d_out, void *stream) {
    dev_require(device);
    if (!n) return;
    k::launch_synth(d_out, n, seed, first, (hipStream_t)stream);
    MF_HIP(hipGetLastError());
}
uint64_t dev_selftest_epilogue(int device, int mode, bool u8, bool have_as, float A, float S, int lo, int hi) {
    dev_require(device);
    if (mode == 3 && !have_as && !u8) { // negative control of the rounding check: plain round-to-nearest-even (must mismatch)
        const unsigned long long r3 = k::selftest_rounding(3, false, (float)lo, (float)hi, nullptr);
        if (r3 == ~0ull) fail(MF_ERR_HIP, "selftest kernel could not run");
        return r3;
    }
    if ((mode != 1 && mode != 2) || lo > hi || lo < (u8 ? 0 : -128) || hi > (u8 ? 255 : 127))
        fail(MF_ERR_INVALID_ARG, "selftest: mode 1 or 2 and a clamp inside the element type's range");
    if (mode == 2 && (lo != (u8 ? 0 : -128) || hi != (u8 ? 255 : 127)))
        fail(MF_ERR_INVALID_ARG, "selftest: the saturating pack (mode 2) is only ever used with the whole range as clamp");
    const unsigned long long r = have_as ? k::selftest_requant(mode, u8, A, S, (float)lo, (float)hi, nullptr)
                                         : k::selftest_rounding(mode, u8, (float)lo, (float)hi, nullptr);
    if (r == ~0ull) fail(MF_ERR_HIP, "selftest kernel could not run");
    return r;
}
uint64_t dev_selftest_fma_epilogue(int device, float A, float S, bool u8, int64_t amin, int64_t amax, float S3, float C3, int pivot,
                                   int64_t patch_acc, int patch_delta) {
    dev_require(device);
    MF_HIP(hipSetDevice(device));
    DevBuf dA, dS, dC3, dS3, dpiv, dmn, dmx, dbad, dpP, dpR;
    const int32_t mn = (int32_t)amin, mx = (int32_t)amax, pP = patch_delta ? k::MF_MAGIC_I + (int32_t)patch_acc + pivot : 0, pR = pP + patch_delta;
    const unsigned long long zero = 0;
    dpP.upload(&pP, 4), dpR.upload(&pR, 4);
    dA.upload(&A, 4), dS.upload(&S, 4), dC3.upload(&C3, 4), dS3.upload(&S3, 4), dpiv.upload(&pivot, 4), dmn.upload(&mn, 4), dmx.upload(&mx, 4);
    dbad.upload(&zero, 8);
    unsigned long long bad = ~0ull;
    if (!k::verify_fma_form(dA.as<float>(), dS.as<float>(), dC3.as<float>(), dS3.as<float>(), dpiv.as<int>(), dmn.as<int>(), dmx.as<int>(), dpP.as<int>(), dpR.as<int>(), 1,
                            u8 ? 0.0f : -128.0f, u8 ? 255.0f : 127.0f, u8, (unsigned long long *)dbad.p, nullptr))
        fail(MF_ERR_HIP, "selftest kernel could not run");
    MF_HIP(hipMemcpy(&bad, dbad.p, 8, hipMemcpyDeviceToHost));
    return (uint64_t)bad;
}
uint64_t dev_selftest_cvt_pk(int device) {
    dev_require(device);
    MF_HIP(hipSetDevice(device));
    const unsigned long long r = k::selftest_cvt_pk(nullptr);
    if (r == ~0ull) fail(MF_ERR_HIP, "selftest kernel could not run");
    return (uint64_t)r;
}
uint64_t dev_verify_quant_div(int device, float scale, float rcp, int zp, bool u8) {
    dev_require(device);
    MF_HIP(hipSetDevice(device));
    return k::verify_quant_div(scale, rcp, (float)zp, u8 ? 0.0f : -128.0f, u8 ? 255.0f : 127.0f, nullptr);
}
uint64_t dev_checksum_i8(int device, const int8_t *d_in, size_t n, void *stream) {
    dev_require(device);
    unsigned long long *d_res = nullptr, h = 0;
    MF_HIP(hipMalloc((void **)&d_res, 8));
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(d_res, 0, 8, s);
    if (e == hipSuccess && n) {
        k::launch_checksum(d_in, n, d_res, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h, d_res, 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_res);
    if (e != hipSuccess) fail(MF_ERR_HIP, std::string("checksum: ") + hipGetErrorString(e));
    return (uint64_t)h;
}

} // namespace mf
