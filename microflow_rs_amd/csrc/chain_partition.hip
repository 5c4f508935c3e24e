// chain_partition.hip -- the planner that cuts a run of run-time-geometry pairs (single-pair chain groups, fused_pairs.hip) into
// chain_rt launches, by cost model or by measurement.  Host code only.
#include <cstdio>

#include "fused_impl.hpp"

namespace mf {

// How to run `n` consecutive single-pair chain groups: seg_len[i] = number of pairs of the chain that starts at pair i (0: pair i is
// inside a chain that started earlier); unfused[i] = pair i is cheapest as two separate operator launches.  Dynamic programme over the
// planner's cost estimates (k_chain.hip: chain_plan / chain_unfused_us_per_image).
namespace {
// The partition by MEASUREMENT (the default when a device is there, i.e. always: operators are created on one): every plannable
// candidate "pairs i .. i + len - 1 as one chain_rt launch", and every pair as its two separate operators, is run on scratch tensors
// at a batch that fills the chip for dozens of steps, and the dynamic programme takes the times.  The cost model's errors were
// 0.7 - 1.5x on single pairs and 1.0 - 1.3x on chains (profiles/r04/chain_calib.txt) -- larger than the differences it decides
// between -- and every kernel change moved them.  ~0.1 - 0.3 s per model at creation; MF_CHAIN_AUTOTUNE=0 goes back to the estimates.
struct ChainTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t st = nullptr; // a private NON-BLOCKING stream: the timing neither waits for nor stalls the caller's other streams
    DevBuf a, b, c;
    size_t cap = 0;
    bool ok = false;
    explicit ChainTimer(size_t bytes) {
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); st = nullptr; return; }
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return;
        for (DevBuf *d : {&a, &b, &c}) {
            if (hipMalloc(&d->p, bytes) != hipSuccess) { (void)hipGetLastError(); return; }
            (void)hipMemsetAsync(d->p, 0, bytes, st);
        }
        cap = bytes, ok = hipStreamSynchronize(st) == hipSuccess;
    }
    ~ChainTimer() {
        if (st) (void)hipStreamSynchronize(st);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (st) (void)hipStreamDestroy(st);
    }
    template <typename F> double us(F &&launch) { // best of five after a warm-up; < 0: failed (a throwing launch counts as failed)
        try {
            launch();
            double best = -1;
            for (int r = 0; r < 5; ++r) {
                if (hipEventRecord(e0, st) != hipSuccess) return -1;
                launch();
                if (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) return -1;
                float ms = 0;
                if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return -1;
                best = best < 0 || ms * 1e3 < best ? ms * 1e3 : best;
            }
            return best;
        } catch (const Error &) {
            (void)hipGetLastError();
            failed = true;
            return -1;
        }
    }
    bool failed = false; // a launch threw: the caller drops every measurement and plans from the estimates
};
} // namespace

void fused_chain_partition(FusedImpl *const *groups, int n, int *seg_len, bool *unfused, int *seg_G, bool autotune_opt) {
    auto member = [&](int i) -> const std::pair<OpImpl *, OpImpl *> & { return groups[i]->chain.members[0]; };
    std::vector<k::ChainGeom> geo((size_t)n);
    for (int i = 0; i < n; ++i) geo[(size_t)i] = chain_geom(member(i).first, member(i).second);
    // pairs i .. i + len - 1 can be ONE chain at all: the same element type, and C >= 16 unless alone (a superpixel pair's output
    // tensor is not in the next pair's units: chain_geom)
    auto candidate = [&](int i, int len) {
        for (int j = i; j < i + len; ++j)
            if (member(j).first->s.u8 != member(i).first->s.u8 || (len != 1 && member(j).first->s.C < 16)) return false;
        return true;
    };
    // A forced plan (MF_CHAIN_PLAN, read NOW: one process prepares the same model under many plans) replaces both the dynamic
    // programme and the timing.  Every segment is made by the functions autotune installs its winners with -- fused_chain_create,
    // chain_create + swap -- behind the same chain_plan feasibility checks, so that the switch can install nothing autotune could
    // not; a segment that cannot be made fails the preparation (a test must never pass on the planner's plan after all).
    if (switches().dev) {
        const Switches now = switches_parse();
        if (now.chain_plan_set) {
            if (!now.chain_plan_error.empty()) fail(MF_ERR_INVALID_ARG, "MF_CHAIN_PLAN: " + now.chain_plan_error);
            const bool verbose = switches().chain_verbose;
            for (int i = 0; i < n; ++i) seg_len[i] = 0, unfused[i] = false;
            if (seg_G) for (int i = 0; i < n; ++i) seg_G[i] = 0;
            int i = 0;
            for (size_t e = 0; e < now.chain_plan.size(); ++e) {
                const ChainPlanSeg &sp = now.chain_plan[e];
                const int len = std::max(sp.len, 1);
                const std::string what = "MF_CHAIN_PLAN segment " + std::to_string(e) + " (" + std::to_string(sp.len) + ":" + std::to_string(sp.G) + ":" +
                                         std::to_string(sp.dbuf) + ", pairs " + std::to_string(i) + ".." + std::to_string(i + len - 1) + " of " + std::to_string(n) + ")";
                if (i + len > n) fail(MF_ERR_UNSUPPORTED, what + ": past the end of the run");
                seg_len[i] = len;
                const k::ChainArgs *made = nullptr;
                std::unique_ptr<FusedImpl> trial;
                if (sp.len == 0) {
                    unfused[i] = true;
                } else if (sp.len == 1) {
                    if (sp.G > 0 || sp.dbuf >= 0) {
                        trial = chain_create(&member(i), 1, sp.G, sp.dbuf);
                        if (!trial) fail(MF_ERR_UNSUPPORTED, what + ": no such plan");
                        if (sp.dbuf >= 0 && trial->chain.args.dbuf != sp.dbuf) fail(MF_ERR_UNSUPPORTED, what + ": the input tile does not fit twice");
                        std::swap(*groups[i], *trial);
                    }
                    made = &groups[i]->chain.args;
                } else {
                    if (!seg_G) fail(MF_ERR_UNSUPPORTED, what + ": the caller takes no images per step");
                    trial.reset(fused_chain_create(groups + i, len, sp.G)); // (the caller makes the same one again from seg_G)
                    if (!trial) fail(MF_ERR_UNSUPPORTED, what + ": no such plan");
                    seg_G[i] = sp.G;
                    made = &trial->chain.args;
                }
                if (verbose) {
                    if (made) fprintf(stderr, "[microflow_amd] chain plan forced: pairs %d..%d G %d dbuf %d nwave %d lds %d\n", i, i + len - 1, made->G, made->dbuf, made->nwave, made->lds_bytes);
                    else fprintf(stderr, "[microflow_amd] chain plan forced: pair %d unfused\n", i);
                }
                i += len;
            }
            if (i != n) fail(MF_ERR_UNSUPPORTED, "MF_CHAIN_PLAN covers " + std::to_string(i) + " pairs of a run of " + std::to_string(n));
            return;
        }
    }
    const bool force_fuse = switches().chain_force; // tests: never prefer the unfused operators
    const double INF = 1e30;
    std::vector<double> best((size_t)n + 1, INF);
    std::vector<int> choice((size_t)n + 1, 1);
    std::vector<char> choice_unf((size_t)n + 1, 0);
    best[(size_t)n] = 0;
    std::vector<k::ChainPair> tab((size_t)k::CHAIN_MAX);
    // measuring is the CALLER's choice (mf_model_set_autotune; off by default: model creation is then deterministic, allocates no
    // scratch and launches nothing); MF_CHAIN_AUTOTUNE=1 / =0 overrides it for scripts
    const int env_tune = switches().chain_autotune;
    bool autotune = env_tune < 0 ? autotune_opt : env_tune != 0;
    const bool verbose_t = switches().chain_verbose;
    const bool tune_g = switches().chain_tune_g;
    // measured[i][len]: microseconds per image of the candidate (< 0: not measured); measured_unf[i]: of the pair's two operators
    std::vector<std::vector<double>> measured((size_t)n, std::vector<double>((size_t)k::CHAIN_MAX + 1, -1.0));
    std::vector<double> measured_unf((size_t)n, -1.0);
    const size_t CAP = (size_t)512 << 20; // upper limit of a scratch tensor: dozens of steps per workgroup also for 2 KB images
    auto tensor_bytes = [&](int i, int len) { // the largest tensor any operator of pairs i .. i + len - 1 touches, per image
        size_t m = 0;
        for (int j = i; j < i + len; ++j) {
            const OpSpec &d = member(j).first->s, &q = member(j).second->s;
            m = std::max(m, std::max((size_t)d.H * d.W * d.C, std::max((size_t)d.OH * d.OW * d.N, (size_t)q.OH * q.OW * q.N)));
        }
        return m;
    };
    auto batch_of = [&](size_t tb) { return std::min<size_t>(CAP / std::max<size_t>(tb, 1), 262144) & ~(size_t)63; };
    if (autotune && n >= 1) {
        size_t need = 0; // the scratch the largest candidate needs (not a fixed 512 MB)
        for (int i = 0; i < n; ++i)
            for (int len = 1; len <= n - i && len <= k::CHAIN_MAX; ++len) need = std::max(need, batch_of(tensor_bytes(i, len)) * tensor_bytes(i, len));
        ChainTimer tm(need + 256);
        for (int i = 0; i < n && tm.ok; ++i) {
            for (int len = 1; len <= n - i && len <= k::CHAIN_MAX; ++len) {
                if (!candidate(i, len)) break;
                const size_t B = batch_of(tensor_bytes(i, len));
                if (B < 256) continue;
                std::unique_ptr<FusedImpl> owned(len == 1 ? nullptr : fused_chain_create(groups + i, len)); // (freed on every path)
                FusedImpl *f = len == 1 ? groups[i] : owned.get();
                if (!f) continue; // (no plan: longer candidates from i may still exist -- a later pair can be smaller)
                const double t = tm.us([&] { fused_run(f, (const int8_t *)tm.a.p, B, (int8_t *)tm.b.p, tm.st); });
                if (t > 0) measured[(size_t)i][(size_t)len] = t / (double)B;
                if (len == 1 && tune_g && t > 0) {
                    // the single pair's images per step and double buffering, measured: every multiple of the column grids' images up to
                    // 4x / down to 1/4 of the planner's choice, with and without the second input buffer.  The winner's plan replaces
                    // the group's in place.
                    const int G0 = groups[i]->chain.args.G, cg = std::max(1, groups[i]->chain.args.max_cg), db0 = groups[i]->chain.args.dbuf;
                    double best_t = t;
                    std::unique_ptr<FusedImpl> best_f;
                    const int cands[8] = {G0 / 4, G0 / 2, 3 * G0 / 4, G0, 3 * G0 / 2, 2 * G0, 3 * G0, 4 * G0};
                    for (int ci = 0; ci < 8; ++ci) {
                        const int G = cands[ci];
                        if (G < cg || G > 128 || G % cg != 0 || (ci > 0 && G == cands[ci - 1])) continue;
                        for (int db = 0; db < 2; ++db) {
                            if (G == G0 && db == db0) continue;
                            std::unique_ptr<FusedImpl> cand = chain_create(&member(i), 1, G, db);
                            if (!cand || cand->chain.args.dbuf != db) continue;
                            const double tc = tm.us([&] { fused_run(cand.get(), (const int8_t *)tm.a.p, B, (int8_t *)tm.b.p, tm.st); });
                            if (verbose_t) fprintf(stderr, "[microflow_amd] chain autotune: pair %d G %d dbuf %d: %.4f us/image (planner's G %d dbuf %d: %.4f)\n", i, G, db, tc / (double)B, G0, db0, t / (double)B);
                            if (tc > 0 && tc < (best_f ? best_t : t * 0.96)) best_t = tc, best_f = std::move(cand); // (a clear win over the planner's: 4 %)
                        }
                    }
                    if (best_f) {
                        std::swap(*groups[i], *best_f);
                        measured[(size_t)i][1] = best_t / (double)B;
                    }
                }
                if (len == 1) {
                    OpImpl *dw = member(i).first, *pw = member(i).second;
                    const double u = tm.us([&] {
                        op_run(dw, (const int8_t *)tm.a.p, B, (int8_t *)tm.c.p, tm.st);
                        op_run(pw, (const int8_t *)tm.c.p, B, (int8_t *)tm.b.p, tm.st);
                    });
                    if (u > 0) measured_unf[(size_t)i] = u / (double)B;
                }
                if (verbose_t)
                    fprintf(stderr, "[microflow_amd] chain autotune: pairs %d..%d batch %zu: %.4f us/image%s\n", i, i + len - 1, B, measured[(size_t)i][(size_t)len],
                            len == 1 ? (" (unfused " + std::to_string(measured_unf[(size_t)i]) + ")").c_str() : "");
            }
        }
        if (tm.st) (void)hipStreamSynchronize(tm.st);
        (void)hipGetLastError();
        // The measurements are used only as a whole: every pair must have its own time (measured us/image of the chip and estimated
        // us/image per CU are different units and must never meet in one sum); a launch that threw, a pair too large for the scratch
        // or a failed timer send the whole run back to the estimates.
        bool complete = tm.ok && !tm.failed;
        for (int i = 0; i < n && complete; ++i) complete = measured[(size_t)i][1] > 0;
        if (!complete) {
            if (verbose_t || switches().verbose) fprintf(stderr, "[microflow_amd] chain autotune incomplete: planning %d pairs from the cost model\n", n);
            autotune = false;
        }
    }
    for (int i = n - 1; i >= 0; --i) {
        for (int len = 1; len <= n - i && len <= k::CHAIN_MAX; ++len) {
            if (autotune) { // measured costs (a candidate that was not measured does not exist)
                double c = measured[(size_t)i][(size_t)len];
                if (c <= 0) continue;
                if (len > 1) c *= 1.05; // (a chain has to win clearly: isolated timings of this size repeat to 2 - 3 %)
                char unf = 0;
                if (len == 1 && !force_fuse && measured_unf[(size_t)i] > 0 && measured_unf[(size_t)i] < c) c = measured_unf[(size_t)i], unf = 1;
                if (c + best[(size_t)i + len] < best[(size_t)i]) best[(size_t)i] = c + best[(size_t)i + len], choice[(size_t)i] = len, choice_unf[(size_t)i] = unf;
                continue;
            }
            k::ChainArgs a{};
            if (!candidate(i, len) || !k::chain_plan(geo.data() + i, len, tab.data(), a, 150 * 1024)) {
                if (len == 1) { // (cannot happen for a group that exists; keep the programme total)
                    if (best[(size_t)i + 1] < best[(size_t)i]) best[(size_t)i] = best[(size_t)i + 1], choice[(size_t)i] = 1, choice_unf[(size_t)i] = 1;
                }
                continue;
            }
            double c = a.est_us_per_image;
            char unf = 0;
            if (len == 1 && !force_fuse) {
                const double u = k::chain_unfused_us_per_image(geo.data() + i, 1);
                if (u < c) c = u, unf = 1;
            }
            if (c + best[(size_t)i + len] < best[(size_t)i]) best[(size_t)i] = c + best[(size_t)i + len], choice[(size_t)i] = len, choice_unf[(size_t)i] = unf;
        }
    }
    for (int i = 0; i < n; ++i) seg_len[i] = 0, unfused[i] = false;
    for (int i = 0; i < n; i += choice[(size_t)i]) seg_len[i] = choice[(size_t)i], unfused[i] = choice_unf[(size_t)i] != 0;
    // the images per step of the chosen multi-pair chains, measured like the single pairs' (1/2 ... 2x the planner's)
    if (seg_G) {
        for (int i = 0; i < n; ++i) seg_G[i] = 0;
        if (autotune && tune_g) {
            std::unique_ptr<ChainTimer> tm;
            for (int i = 0; i < n; ++i) {
                const int len = seg_len[i];
                if (len < 2) continue;
                if (!tm) {
                    size_t need2 = 0;
                    for (int i2 = 0; i2 < n; ++i2)
                        if (seg_len[i2] >= 2) need2 = std::max(need2, batch_of(tensor_bytes(i2, seg_len[i2])) * tensor_bytes(i2, seg_len[i2]));
                    tm.reset(new ChainTimer(need2 + 256));
                }
                if (!tm->ok || tm->failed) break;
                const size_t B = batch_of(tensor_bytes(i, len));
                std::unique_ptr<FusedImpl> base(fused_chain_create(groups + i, len, 0));
                if (!base || B < 256) continue;
                const double t0 = tm->us([&] { fused_run(base.get(), (const int8_t *)tm->a.p, B, (int8_t *)tm->b.p, tm->st); });
                const int G0 = base->chain.args.G, cg = std::max(1, base->chain.args.max_cg);
                double best_t = t0;
                const int cands[4] = {G0 / 2, 3 * G0 / 4, 3 * G0 / 2, 2 * G0};
                for (int ci = 0; ci < 4 && t0 > 0; ++ci) {
                    const int G = cands[ci];
                    if (G < cg || G > 128 || G % cg != 0 || G == G0) continue;
                    std::unique_ptr<FusedImpl> cand(fused_chain_create(groups + i, len, G));
                    if (!cand) continue;
                    const double tc = tm->us([&] { fused_run(cand.get(), (const int8_t *)tm->a.p, B, (int8_t *)tm->b.p, tm->st); });
                    if (verbose_t) fprintf(stderr, "[microflow_amd] chain autotune: chain %d..%d G %d: %.4f us/image (planner's G %d: %.4f)\n", i, i + len - 1, G, tc / (double)B, G0, t0 / (double)B);
                    if (tc > 0 && tc < (seg_G[i] ? best_t : t0 * 0.96)) best_t = tc, seg_G[i] = G;
                }
            }
            if (tm && tm->st) (void)hipStreamSynchronize(tm->st);
            (void)hipGetLastError();
        }
    }
    const bool verbose = switches().chain_verbose || switches().verbose; // the plan, so that a run can be reproduced
    if (verbose) {
        fprintf(stderr, "[microflow_amd] chain partition of %d pairs:", n);
        for (int i = 0; i < n; ++i)
            if (seg_len[i]) fprintf(stderr, " [%d..%d%s]", i, i + seg_len[i] - 1, unfused[i] ? " unfused" : "");
        fprintf(stderr, " %s %.4f us/image%s\n", autotune ? "measured" : "est", best[0], autotune ? "" : "/CU");
    }
}

} // namespace mf
