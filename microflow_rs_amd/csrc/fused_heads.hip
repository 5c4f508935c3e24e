// fused_heads.hip -- the groups at a network's classifier end: pool + head + Softmax, FullyConnected (+ Softmax) runs, a global pool
// or a one-input-channel convolution in front of them; and the Conv2D + AveragePool2D stage.  Host code only; the kernels are in k_*.hip.
#include "fused_impl.hpp"

namespace mf {

FusedImpl *fused_tail_create(OpImpl *pool, OpImpl *conv, OpImpl *sm) {
    if (!pool || !conv || !sm) return nullptr;
    const OpSpec &p = pool->s, &c = conv->s, &m = sm->s;
    if (p.u8 != c.u8 || c.u8 != m.u8) return nullptr;
    if (!conv->finite_consts || !std::isfinite(p.pool_c0) || !std::isfinite(p.pool_c1)) return nullptr;
    if (p.kind != MF_OP_AVERAGE_POOL_2D || c.kind != MF_OP_CONV_2D || m.kind != MF_OP_SOFTMAX) return nullptr;
    if (p.OH != 1 || p.OW != 1) return nullptr;                       // one pooling window
    if (c.KH != 1 || c.KW != 1 || c.H != 1 || c.W != 1 || c.OH != 1 || c.OW != 1 || c.C != p.C) return nullptr;
    if (m.M != 1 || m.N != c.N) return nullptr;                       // softmax over the head's N values
    // the in-range taps of the single window
    int shy, shx;
    pool_window_shift(p, shy, shx);
    std::vector<int> taps;
    for (int ky = 0; ky < p.KH; ++ky)
        for (int kx = 0; kx < p.KW; ++kx) {
            const int iy = ky - shy, ix = kx - shx;
            if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) taps.push_back((iy * p.W + ix) * p.C);
        }
    if (!k::tail_supported(p.C, c.N, (int)taps.size())) return nullptr;
    std::unique_ptr<FusedImpl> f = make_group(FusedImpl::TAIL, pool, conv, sm, "tail_pool_head_softmax<" + std::to_string(c.N) + ">");
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
    return f.release();
}

// FullyConnected (one row per inference, the few-outputs row-wave kernel) -> [Reshape] -> Softmax
// over exactly those outputs
FusedImpl *fused_fc_softmax_create(OpImpl *fc, OpImpl *sm) {
    if (!fc || fc->fast != OpImpl::FC_ROWWAVE || fc->s.M != 1 || fc->s.N < 2 || !softmax_over_row(sm, fc->s.N, fc->s.u8, fc->device)) return nullptr;
    return make_group(FusedImpl::FCSM, fc, sm, nullptr, "fc_rowwave_softmax<" + std::to_string(fc->s.N) + ">").release();
}

// Consecutive FullyConnected operators (each reading the previous one's [M][N] output) + optionally a Softmax over one row, as
// one fc_chain launch; nullptr when a member has no fc_rt image or the layers' images and tiles do not fit the LDS budget
static bool fc_chain_args(OpImpl *const *fcs, int n, OpImpl *sm, k::FcChainArgs &a) {
    if (switches().no_fc_chain || n < 2 || n > k::FC_CHAIN_MAX || !fcs[0]) return false;
    // any M, the first layer's (a [M][N] activation matrix per inference)
    if (!fc_layers_fill(fcs, n, a, fcs[0]->s.M, fcs[0]->s.u8, fcs[0]->device)) return false;
    for (int l = 0; l < n; ++l)
        if (fcs[l]->fast == OpImpl::FC_ROWWAVE) return false; // (a few-outputs layer keeps its row-wave kernel, or the FCSM group)
    if (sm) {
        if (fcs[0]->s.M != 1 || !softmax_over_row(sm, fcs[n - 1]->s.N, fcs[0]->s.u8, fcs[0]->device)) return false;
        a.softmax = 1, a.sm = sm->sm;
    }
    return k::fc_chain_plan(a);
}
bool fused_fc_chain_fits(OpImpl *const *fcs, int n, OpImpl *sm) {
    k::FcChainArgs a;
    return fc_chain_args(fcs, n, sm, a);
}
FusedImpl *fused_fc_chain_create(OpImpl *const *fcs, int n, OpImpl *sm) {
    k::FcChainArgs a;
    if (!fc_chain_args(fcs, n, sm, a)) return nullptr;
    std::unique_ptr<FusedImpl> f = make_group(FusedImpl::FCCHAIN, fcs[0], fcs[n - 1], sm, "fc_chain<" + std::to_string(n) + (sm ? ">+sm" : ">"));
    f->fcchain.args = a, f->fcchain.M = fcs[0]->s.M, f->epi_mode = a.magic;
    return f.release();
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
    // the in-range taps of the single window must be the whole image
    int shy, shx;
    pool_window_shift(p, shy, shx);
    if (p.KH - 1 - shy < p.H - 1 || p.KW - 1 - shx < p.W - 1) return false;
    a = k::PoolFcArgs{};
    k::FcChainArgs &c = a.c;
    // one row per inference (the pooled pixel), the pool's element type and device
    if (!fc_layers_fill(fcs, n, c, 1, p.u8, pool->device) || fcs[0]->s.K != p.C) return false;
    if (sm) {
        if (!softmax_over_row(sm, fcs[n - 1]->s.N, p.u8, pool->device)) return false;
        c.softmax = 1, c.sm = sm->sm;
    }
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
    std::unique_ptr<FusedImpl> f = make_group(FusedImpl::POOLFC, pool, fcs[n - 1], sm, "pool_fc_chain<" + std::to_string(n) + (sm ? ">+sm" : ">"));
    f->poolfc = a, f->epi_mode = a.c.magic;
    return f.release();
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
        if (!softmax_over_row(sm, q.N, d.u8, cv->device)) return false;
        a.softmax = 1, a.sm = sm->sm;
    }
    a.A = cv->conv.A, a.S = cv->conv.S, a.Kc = cv->conv.Kc, a.lo_f = cv->conv.lo_f, a.hi_f = cv->conv.hi_f;
    a.izp4 = 0x01010101u * (uint32_t)(uint8_t)(int8_t)d.izp;
    a.magic = std::min(cv->magic_mode, 2), a.xr = g.xr; // (the convolution's mode; the FullyConnected's few bytes take mode 0)
    if (cv->conv.xr != g.xr) return false;
    return k::conv1_fc_plan(a);
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
    std::unique_ptr<FusedImpl> f = make_group(FusedImpl::CONV1FC, conv, fc, sm,
                                              std::string("conv1_fc_rt<") + (dw ? "dw," : "conv,") + std::to_string(d.KH) + "x" + std::to_string(d.KW) + "," +
                                                  std::to_string(d.N) + (sm ? ">+sm" : ">"));
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
    f->conv1fc.args = a, f->epi_mode = a.magic;
    // The routing rule of DESIGN 4.2d, by measurement (profiles/r10/time_conv1_fc.txt): where the FullyConnected has its own fc_rt launch,
    // conv1_fc_rt beat the three launches at batch 4096 (one step per workgroup: 1.13 - 1.55x) and lost at 65 536 (0.82 - 1.01x), so such
    // a group takes batches up to 4096 only; where the FullyConnected alone runs fc_generic it won at both (2.3 - 3.1x) and takes any
    f->conv1fc.max_batch = fc->fcrt_ok ? 4096 : 0;
    return f.release();
}

// A Conv2D directly followed by an AveragePool2D with more than one output pixel on exactly its output, as one conv_pool_rt launch
// (k_conv_pool.hip) -- or by a MaxPool2D, as one conv_maxpool_rt launch (k_conv_maxpool.hip: the same kernel text, plan and
// conditions; its own name and its own measured exclusions): the convolution's bytes stay in LDS. Same device and element type, finite constants, neither forced generic, and
// what k::conv_pool_plan accepts.  The weight image, the tables and the padded constants are the group's own, built from the
// convolution's host copies: alone it may run conv_rows_lds, conv_mm_rt or pw_rt, which keep other images.
FusedImpl *fused_conv_pool_create(OpImpl *conv, OpImpl *pool) {
    if (switches().no_conv_pool || !conv || !pool || conv->force_generic || pool->force_generic) return nullptr;
    const OpSpec &d = conv->s, &q = pool->s;
    const bool mx = q.kind == MF_OP_MAX_POOL_2D;
    if (d.kind != MF_OP_CONV_2D || (q.kind != MF_OP_AVERAGE_POOL_2D && !mx) || conv->device != pool->device || d.u8 != q.u8) return nullptr;
    if (q.H != d.OH || q.W != d.OW || q.C != d.N) return nullptr; // on exactly the convolution's output
    if (!conv->finite_consts || !std::isfinite(q.pool_c0) || !std::isfinite(q.pool_c1)) return nullptr;
    if (conv->h_w.size() != (size_t)d.N * d.KH * d.KW * d.C || conv->h_A.size() != (size_t)d.N || conv->h_S.size() != (size_t)d.N ||
        conv->h_Kc.size() != (size_t)d.N || conv->h_wzp.size() != (size_t)d.N)
        return nullptr;
    const bool wz = std::any_of(conv->h_wzp.begin(), conv->h_wzp.end(), [](int32_t z) { return z != 0; });
    std::unique_ptr<FusedImpl> f = make_group(FusedImpl::CONVPOOL, conv, pool, nullptr, "");
    k::ConvPoolArgs &a = f->convpool.args;
    std::vector<int> tap;
    std::vector<uint32_t> mask;
    if (!k::conv_pool_plan(a, tap, mask, d.H, d.W, d.C, d.N, d.KH, d.KW, d.sh, d.sw, d.OH, d.OW, d.pad == MF_PAD_SAME, wz, q.KH, q.KW, q.sh, q.sw, q.OH, q.OW,
                           q.pad == MF_PAD_SAME))
        return nullptr;
    // Classes measured NOT faster than the two launches they replace by more than the spread of the repeats (profiles/r14/time_conv_pool.txt,
    // DESIGN 4.17) keep those launches:
    //   one input channel -- a 16-byte operand holds KW real bytes, and conv_rows_lds, which such a convolution runs alone, pads nothing:
    //   28x28x1 -> 6 5x5 ran x0.52, 96x96x1 -> 8 3x3 x0.19, 12x12x1 -> 8 5x5 x0.86;
    //   a plan beyond half a CU's LDS -- one workgroup per CU is one wave per SIMD, and a 16-pixel chunk is bound by instruction issue:
    //   64x64x4 -> 64 in bands x0.67, 48x48x8 -> 96 in bands x0.76, 32x32x32 -> 64 (one image, 126 KiB) x0.74;
    //   fewer than 16 output channels (half a matrix tile is padding: x0.44 - x0.94 over C = 3 .. 12, 3x3 and 5x5), or fewer than 2400
    //   real multiply-adds per output pixel, KH KW C N (the chunk's cost is the same, the launches it replaces are cheap: the sweep's
    //   x0.66 - x1.08, none clearing its spread; from 2400 on x1.14 - x2.81, all clearing it).
    const bool slow = d.C == 1 || a.lds > 80 * 1024 || d.N < 16 || (long long)d.KH * d.KW * d.C * d.N < 2400;
    // With a MaxPool2D behind the convolution the classes were measured anew (profiles/r17/time_conv_maxpool_all.txt and
    // time_conv_maxpool_sweep.txt) and fall the same way, since phase A is the same and the two launches the group replaces
    // differ by the pool alone: C = 1 x0.51 / x0.19 / x0.86; beyond 80 KiB x0.68 / x0.76 / x0.75; N = 8 x0.44 - x0.95; below 2400
    // multiply-adds per output pixel x0.66 - x1.10 with one shape of eleven clearing its spread (16x16x8 -> 32 3x3, 2304: x1.10 against
    // 8.1 %, while 16x16x4 -> 64 at the same 2304 does not: x1.07 against 10.6 %); from 2400 on x1.15 - x2.82, all clearing it.
    if (slow && !switches().conv_pool_all) return nullptr;
    k::ConvGemmArgs wg{}; // (what conv_gemm_weight_image reads: the filter and its padded row)
    wg.N = d.N, wg.C = d.C, wg.KH = d.KH, wg.KW = d.KW, wg.KWCP = a.KWCP;
    const std::vector<int8_t> img = k::conv_gemm_weight_image(conv->h_w.data(), wg);
    if (img.size() != (size_t)a.NT * a.KS * 1024) return nullptr;
    a.wimg = keep(*f, img.data(), img.size());
    a.tap = (const int *)keep(*f, tap.data(), tap.size() * sizeof(int));
    a.kmask = (const uint32_t *)keep(*f, mask.data(), mask.size() * 4);
    const size_t np = (size_t)a.NT * 16; // a lane fetches the constants of its four channels whether or not they are below N
    auto padded = [&](const auto &src) {
        auto h = src;
        h.resize(np, 0);
        return keep(*f, h.data(), np * 4);
    };
    a.A = (const float *)padded(conv->h_A), a.S = (const float *)padded(conv->h_S);
    a.Kc = (const int *)padded(conv->h_Kc), a.wzp = (const int *)padded(conv->h_wzp);
    a.izp4 = 0x01010101u * (uint32_t)(uint8_t)(int8_t)d.izp;
    a.lo_f = conv->conv.lo_f, a.hi_f = conv->conv.hi_f;
    a.magic = std::min(conv->magic_mode, 2), a.xr = conv->conv.xr;
    a.pool = pool->pool;
    if (pool->pool.xr != a.xr) return nullptr;
    f->convpool.wz = wz, f->convpool.mx = mx;
    f->epi_mode = a.magic;
    f->name = std::string(mx ? "conv_maxpool_rt<" : "conv_pool_rt<") + std::to_string(d.H) + "x" + std::to_string(d.W) + "x" + std::to_string(d.C) + "-" + std::to_string(d.N) + ";" + std::to_string(d.KH) + "x" +
              std::to_string(d.KW) + (d.sh != 1 || d.sw != 1 ? "s" + std::to_string(d.sh) : "") + ";p" + std::to_string(q.KH) + "x" + std::to_string(q.KW) +
              (q.sh != 1 || q.sw != 1 ? "s" + std::to_string(q.sh) : "") +
              (a.NB == 1 ? ";G" + std::to_string(a.G) : ";PB" + std::to_string(a.PB) + ";NB" + std::to_string(a.NB)) + ">";
    if (switches().chain_verbose)
        fprintf(stderr, "[microflow_amd] conv + pool group %s: %d k steps, %d tiles, tile %d rows x %d B, Y %d B per image (%d B per pixel), lds %d B, mode %d\n",
                f->name.c_str(), a.KS, a.NT, a.RB, a.ROW, a.YIMG, a.NP, a.lds, a.magic);
    return f.release();
}

// A PAD directly followed by a VALID Conv2D / DepthwiseConv2D on exactly its output, as ONE launch of the kernel the convolution gets from
// the run-time-geometry planners when it is taken as an operator on the unpadded image with the PAD's top / left rows and columns as its
// window placement (ops.hip op_create_padded_conv).  Those kernels fill every tile byte outside the image with the input zero
// point, which is the PAD's fill: the same bytes as PAD, then the VALID convolution.  Same device and element type, finite constants,
// neither forced generic, a filter larger than 1 x 1 (a 1x1 convolution has no window to place).  nullptr: the two launches stay
FusedImpl *fused_pad_conv_create(OpImpl *pad, OpImpl *conv) {
    if (switches().no_pad_conv || !pad || !conv || pad->force_generic || conv->force_generic) return nullptr;
    const OpSpec &p = pad->s, &d = conv->s;
    const bool dw = d.kind == MF_OP_DEPTHWISE_CONV_2D;
    if (p.kind != MF_OP_PAD || (d.kind != MF_OP_CONV_2D && !dw) || d.pad != MF_PAD_VALID || pad->device != conv->device || p.u8 != d.u8) return nullptr;
    if (d.H != p.OH || d.W != p.OW || d.C != p.C) return nullptr; // on exactly the PAD's output
    if (d.KH == 1 && d.KW == 1) return nullptr;
    if (!conv->finite_consts) return nullptr;
    // the PAD's fill is the byte the kernels put outside the image: the convolution's input zero point (it is, where the model's
    // quantisation is consistent; where not, the two launches compute what the file says)
    if ((pad->padargs.fill4 & 0xffu) != (uint32_t)(uint8_t)(int8_t)conv->conv.izp) return nullptr;
    std::shared_ptr<OpImpl> inner(op_create_padded_conv(conv, p.H, p.W, p.pads[0], p.pads[2]), op_destroy);
    if (!inner) return nullptr;
    std::unique_ptr<FusedImpl> f = make_group(FusedImpl::PADCONV, pad, conv, nullptr, "pad+" + inner->fast_name);
    f->padconv = inner;
    f->epi_mode = conv->magic_mode;
    return f.release();
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
    std::unique_ptr<FusedImpl> f = make_group(FusedImpl::DWFC, dw, fc, sm, k::dwfc_name());
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

// A 1x1 Conv2D on a skip edge and the join -- an ADD or a CONCATENATION -- that reads its result beside
// the running tensor, as one side_join_rt launch (k_side_join.hip) under the name shortcut_add_rt or side_concat_rt.  The class:
// KH = KW = 1, strides (1,1) or (2,2), C and N in whole sixteens inside k::shortcut_add_supported -- for a CONCATENATION the running
// slice in whole sixteens too -- filter zero points all zero in the i8 domain, finite constants on both, neither forced generic.
// Everything else keeps its two launches.  Operand A is the group's own, built from the convolution's host copy -- alone a stride-2
// 1x1 runs conv_mm_rt, which keeps another image; the constants, the clamp and the epilogue mode (0 to 2) are the convolution's own, as
// pw_rt takes them (ops.hip: epi_fields); the join's block is the operator's internal-domain one.
bool shortcut_add_class(const OpSpec &d, bool zero_wzp, bool finite) {
    return d.kind == MF_OP_CONV_2D && d.KH == 1 && d.KW == 1 && d.sh == d.sw && (d.sh == 1 || d.sh == 2) && zero_wzp && finite &&
           d.OH == (d.H + d.sh - 1) / d.sh && d.OW == (d.W + d.sw - 1) / d.sw && k::shortcut_add_supported(d.C, d.N);
}
bool side_concat_class(const OpSpec &d, int run_channels, bool zero_wzp, bool finite) {
    return shortcut_add_class(d, zero_wzp, finite) && k::side_concat_supported(d.C, d.N, run_channels);
}
// What the two creators share: every check that does not depend on the join's own geometry, the group, and the convolution's part of
// its argument block.  CR: the running tensor's channels at a CONCATENATION (an ADD's class does not ask).  nullptr: outside the class
static std::unique_ptr<FusedImpl> side_join_group(FusedImpl::Kind kind, OpImpl *conv, OpImpl *join, bool conv_first, int CR) {
    const bool add = kind == FusedImpl::SHORTCUT;
    if ((add ? switches().no_shortcut_add : switches().no_side_concat) || !conv || !join || conv->force_generic || join->force_generic) return nullptr;
    const OpSpec &d = conv->s, &q = join->s;
    if (q.kind != (add ? MF_OP_ADD : MF_OP_CONCATENATION) || conv->device != join->device || d.u8 != q.u8) return nullptr;
    const bool zero_wzp = std::all_of(conv->h_wzp.begin(), conv->h_wzp.end(), [](int32_t z) { return z == 0; });
    if (!(add ? shortcut_add_class(d, zero_wzp, conv->finite_consts) : side_concat_class(d, CR, zero_wzp, conv->finite_consts))) return nullptr;
    if (conv->h_w.size() != (size_t)d.N * d.C || !std::isfinite(q.join_ca) || !std::isfinite(q.join_cb)) return nullptr;
    std::unique_ptr<FusedImpl> f = make_group(kind, conv, join, nullptr, "");
    k::SideConvArgs &a = add ? f->shortcut.conv : f->sideconcat.conv;
    const int NT = d.N / 16, TB = NT < 4 ? NT : 4, NBLK = (NT + TB - 1) / TB, NSPLIT = NBLK <= 1 ? 1 : (NBLK == 2 ? 2 : 4);
    const std::vector<int8_t> prep = wimage::build_pw_rt_reg_weights(conv->h_w.data(), d.C, d.N, 1, TB, NSPLIT); // [N][1][1][C], i8 domain
    a.pw.wprep = keep(*f, prep.data(), prep.size());
    a.pw.A = conv->conv.A, a.pw.S = conv->conv.S, a.pw.Kc = conv->conv.Kc, a.pw.wzp = conv->conv.wzp;
    a.pw.lo_f = conv->conv.lo_f, a.pw.hi_f = conv->conv.hi_f;
    a.pw.K = d.C, a.pw.N = d.N, a.pw.KS = (d.C + 63) / 64, a.pw.NT = NT, a.pw.patch_pitch = d.N;
    a.pw.TB = TB, a.pw.NSPLIT = NSPLIT;
    a.pw.magic = std::min(conv->magic_mode, 2), a.pw.xr = conv->conv.xr;
    a.H = d.H, a.W = d.W, a.OH = d.OH, a.OW = d.OW, a.sh = d.sh, a.sw = d.sw;
    a.conv_first = conv_first ? 1 : 0;
    f->epi_mode = a.pw.magic;
    f->name = std::string(add ? "shortcut_add_rt<" : "side_concat_rt<") + std::to_string(d.C) + "," + std::to_string(d.N) + (add ? "" : "," + std::to_string(CR)) +
              (d.sh == 2 ? ",s2>" : ">");
    return f;
}
FusedImpl *fused_shortcut_add_create(OpImpl *conv, OpImpl *add, bool conv_first) {
    std::unique_ptr<FusedImpl> f = side_join_group(FusedImpl::SHORTCUT, conv, add, conv_first, 0);
    if (!f || add->s.add_elems != (size_t)conv->s.OH * conv->s.OW * conv->s.N) return nullptr; // on exactly the convolution's output
    f->shortcut.add = add->add;
    return f.release();
}
FusedImpl *fused_side_concat_create(OpImpl *conv, OpImpl *cat, bool conv_first) {
    const int CR = !cat ? 0 : conv_first ? cat->s.cat_cb : cat->s.cat_ca;
    std::unique_ptr<FusedImpl> f = side_join_group(FusedImpl::SIDECONCAT, conv, cat, conv_first, CR);
    if (!f) return nullptr;
    // on exactly the convolution's output: its pixels are the join's rows, its channels the join's slice for that input
    const OpSpec &d = conv->s, &q = cat->s;
    if (q.cat_rows != (size_t)d.OH * d.OW || (conv_first ? q.cat_ca : q.cat_cb) != d.N) return nullptr;
    f->sideconcat.cat = cat->cat, f->sideconcat.CR = CR;
    return f.release();
}

} // namespace mf
