// k_pair_band_body.inc -- the statements of a band-by-band pair kernel, included between the braces of pair_band_rt<KSC, MG, XR4>
// (k_pair_band.hip) and pair_band_deep_rt<MG, XR4> (k_pair_band_deep.hip, which sets KSC = 8): one text, so that each kernel is compiled
// exactly as if it were written out in its own file.  Expects in, out, p (PairBandArgs), batch and the constants KSC, MG, XR4 in scope.
    constexpr int NTHR = 512, NWAVE = 8;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, g = lane >> 4;
    typedef __attribute__((address_space(1))) const v4i g_v4i;
    auto ld16 = [](const void *base, uint32_t off) { return *(g_v4i *)((uintptr_t)base + off); };
    auto ldf4 = [&](const void *base, uint32_t off) {
        const v4i v = ld16(base, off);
        return make_float4(__int_as_float(v[0]), __int_as_float(v[1]), __int_as_float(v[2]), __int_as_float(v[3]));
    };
    auto ldi4 = [&](const void *base, uint32_t off) {
        const v4i v = ld16(base, off);
        return magic4<MG>(make_int4(v[0], v[1], v[2], v[3]));
    };
    const int H = p.H, C = p.C, S = p.S, OH = p.OH, OW = p.OW, N = p.N, NQ = p.NQ;
    const int RB = p.RB, NB = p.NB, TR = p.TR, ROW = p.ROW, PLANE = p.PLANE, NCH = p.NCH;
    const int sh = p.swz_sh, mask = p.swz_mask;
    const uint4 z4 = make_uint4(p.izp4, p.izp4, p.izp4, p.izp4);

    DynSteps dq;
    dq.init(lds + p.q_off, p.queue, tid, p.qcfg);
    // once per launch: every tile byte holds the depthwise input zero point (what stays of it are the halo columns)
    {
        uint4 *dst = (uint4 *)(lds + p.tile_off);
        const int n16 = ((p.dbuf ? 2 : 1) * p.TILE) >> 4;
        for (int i = tid; i < n16; i += NTHR) dst[i] = z4;
    }

    // ---- staging of one step's tile: rows inside the image by LDS-DMA, rows outside rewritten with the zero point ----
    auto stage = [&](int st, int buf) {
        const int img = st / NB, band = st - img * NB;
        const int ROWB = p.W * C, ROWCH = ROWB >> 4, lgNQ = p.lgNQ, nqm = NQ - 1;
        const int iy0 = S * band * RB - 1; // input row of tile row 0 (the reference's SAME shift is (K - 1) / 2 for both strides)
        const int8_t *src0 = in + (long)img * ((long)H * ROWB);
        uint8_t *t0 = lds + p.tile_off + buf * p.TILE;
        for (int r = wave; r < TR; r += NWAVE) {
            const int iy = iy0 + r;
            uint8_t *row = t0 + r * ROW;
            if (iy >= 0 && iy < H) {
                const int8_t *src = src0 + (long)iy * ROWB;
                uint8_t *dst = row + C;
                for (int o = 0; o < ROWCH; o += 64) {
                    const int i = o + lane; // 16-byte group i of the row lands at LDS group i; it must hold source group (x, c ^ swz(x))
                    int sidx = i;
                    if (mask != 0) {
                        const int x = i >> lgNQ, c = i & nqm;
                        sidx = (x << lgNQ) + (c ^ (((x + 1) >> sh) & mask));
                    }
                    if (i < ROWCH) dma16(src + sidx * 16, dst + o * 16);
                }
            } else {
                uint4 *d = (uint4 *)row;
                for (int i = lane; i < (ROW >> 4); i += 64) d[i] = z4;
            }
        }
    };

    auto load_dw = [&](int q) {
        BDwW w;
#pragma unroll
        for (int ty = 0; ty < 3; ++ty) w.A[ty] = ld16(p.dw_wmm, (uint32_t)(((q * 3 + ty) * 64 + lane) * 16));
        const uint32_t co = (uint32_t)((4 * q + g) * 16);
        w.a = ldf4(p.dwA, co), w.s = ldf4(p.dwS, co), w.k = ldi4(p.dwK, co);
        return w;
    };
    auto load_pw = [&](int blk) {
        BPwW<KSC> w;
        const int TB = p.TB, KS = p.KS;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int ks = 0; ks < KSC; ++ks) {
                w.A[t][ks] = v4i{0, 0, 0, 0};
                if (t < TB && ks < KS) w.A[t][ks] = ld16(p.pw_w, (uint32_t)((((blk * TB + t) * KS + ks) * 64 + lane) * 16));
            }
            const uint32_t co = (uint32_t)((blk * 16 * TB + g * 4 * TB + 4 * t) * 4);
            if (t < TB) w.a[t] = ldf4(p.pwA, co), w.s[t] = ldf4(p.pwS, co), w.k[t] = ldi4(p.pwK, co);
            else w.a[t] = w.s[t] = make_float4(0.f, 0.f, 0.f, 0.f), w.k[t] = make_int4(0, 0, 0, 0);
        }
        return w;
    };

    // ---- this wave's contiguous range of the depthwise unit list (channel group, then column, then row: the row varies fastest) ----
    const int UX = p.UX, UY = p.UY, U = NQ * UX * UY;
    const int u0 = (wave * U) >> 3, ucnt = (((wave + 1) * U) >> 3) - u0;
    const int us_q = u0 / (UX * UY), us_r = u0 - us_q * (UX * UY), us_x = us_r / UY, us_y = us_r - us_x * UY;
    // The depthwise operands of the wave's first channel group stay in registers for the whole launch -- except with two k steps, where
    // the pointwise phase (two tiles x two k steps of operand A, their constants, B, accumulators) leaves no room for them inside the
    // 128 registers of two workgroups per CU: there they are fetched again at the top of every step, in front of the wait for the tile.
    // Eight k steps (64 registers of operand A, 32 of B) do the same inside their 256.
    constexpr bool DWRES = KSC != 2 && KSC != 8;
    BDwW wd;
    int qcur = -1;
    if (DWRES && ucnt > 0) wd = load_dw(us_q), qcur = us_q;

    // ---- depthwise phase: tile -> MID ----
    auto dw_phase = [&](int tile_base) {
        const int lgCX = p.lgCX, lgCY = p.lgCY, CXv = 1 << lgCX;
        const int gg = g < 2 ? g : 2; // tap column of this lane group (g == 3 meets zero weights: any readable bytes will do)
        const int cx = col & (CXv - 1), cy = col >> lgCX;
        const int xin0 = cx * S + gg;
        const int tb0 = tile_base + cy * S * ROW + xin0 * C;
        const int mb0 = p.mid_off + ((cy * OW + cx) << 4) + 4 * g;
        const int T_UX = CXv * S * C, XSTEP = CXv * S, M_UX = CXv * 16;
        const int TSTEP = (S * ROW) << lgCY, MSTEP = (OW * 16) << lgCY;
        const float lo = p.dw_lo, hi = p.dw_hi;
        int q = us_q, ux = us_x, uy = us_y, n = ucnt;
        while (n > 0) {
            const int seg = min(n, UY - uy);
            if (q != qcur) wd = load_dw(q), qcur = q; // (a wave's range crosses into the next channel group)
            const int xin = xin0 + ux * XSTEP;
            int a = tb0 + ux * T_UX + ((q ^ ((xin >> sh) & mask)) << 4) + uy * TSTEP;
            int m = mb0 + q * PLANE + ux * M_UX + uy * MSTEP;
            v4i t0 = *(const v4i *)(lds + a), t1 = *(const v4i *)(lds + a + ROW), t2 = *(const v4i *)(lds + a + 2 * ROW);
            for (int k = 0; k < seg; ++k) {
                v4i acc = {wd.k.x, wd.k.y, wd.k.z, wd.k.w};
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(wd.A[0], t0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(wd.A[1], t1, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(wd.A[2], t2, acc, 0, 0, 0);
                a += k + 1 < seg ? TSTEP : 0; // the next unit's taps (the last unit of a segment prefetches itself: no branch)
                t0 = *(const v4i *)(lds + a), t1 = *(const v4i *)(lds + a + ROW), t2 = *(const v4i *)(lds + a + 2 * ROW);
                *(uint32_t *)(lds + m) = requant_pack4<MG, XR4>(acc[0], acc[1], acc[2], acc[3], wd.a, wd.s, lo, hi);
                m += MSTEP;
            }
            n -= seg, uy = 0;
            if (++ux == UX) ux = 0, ++q;
        }
    };

    // ---- pointwise phase: MID -> HBM ----
    const int SLOTS = p.SLOTS, NWB = p.NWB, NBLK = p.NBLK;
    const int blk0 = wave / SLOTS, slot = wave - blk0 * SLOTS;
    const bool persist = NBLK <= NWB; // one pass: a wave's block never changes, its operands are fetched once per launch
    BPwW<KSC> wp;
    if (persist && blk0 < NBLK) wp = load_pw(blk0);
    auto pw_items = [&](int step, auto tbc) {
        constexpr int TB = decltype(tbc)::value;
        const int img = step / NB, band = step - img * NB, o0 = band * RB;
        const int pvalid = min(RB, OH - o0) * OW; // rows past OH of the last band are computed and never stored
        int8_t *obase = out + ((size_t)img * OH + (size_t)o0) * OW * N;
        const float lo = p.pw_lo, hi = p.pw_hi;
        int poff[KSC];
#pragma unroll
        for (int ks = 0; ks < KSC; ++ks) {
            const int pl = 4 * ks + g; // plane = 16-channel group; a k step hanging over K meets zero weights
            poff[ks] = p.mid_off + (pl < NQ ? pl : NQ - 1) * PLANE + col * 16;
        }
        for (int b = blk0; b < NBLK; b += NWB) {
            if (!persist) wp = load_pw(b);
            const int ch0 = b * 16 * TB + g * 4 * TB;
            v4i B[KSC], Bn[KSC];
            auto fetch = [&](int c, v4i(&d)[KSC]) {
#pragma unroll
                for (int ks = 0; ks < KSC; ++ks) d[ks] = *(const v4i *)(lds + poff[ks] + c * 256);
            };
            constexpr bool PF = KSC == 1; // operand prefetch of the next chunk while the registers allow it (128 for two workgroups per CU)
            if constexpr (PF) fetch(slot < NCH ? slot : NCH - 1, B);
            for (int c = slot; c < NCH; c += SLOTS) {
                const int pix = 16 * c + col;
                if constexpr (PF) fetch(c + SLOTS < NCH ? c + SLOTS : c, Bn); // the next chunk's operand (the last chunk re-reads itself)
                else fetch(c, B);
                v4i acc[TB];
#pragma unroll
                for (int t = 0; t < TB; ++t) acc[t] = v4i{wp.k[t].x, wp.k[t].y, wp.k[t].z, wp.k[t].w};
#pragma unroll
                for (int ks = 0; ks < KSC; ++ks)
#pragma unroll
                    for (int t = 0; t < TB; ++t) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wp.A[t][ks], B[ks], acc[t], 0, 0, 0);
                uint32_t packed[TB];
#pragma unroll
                for (int t = 0; t < TB; ++t) packed[t] = requant_pack4<MG, XR4>(acc[t][0], acc[t][1], acc[t][2], acc[t][3], wp.a[t], wp.s[t], lo, hi);
                if (pix < pvalid) { // (the ragged last chunk's columns past the band hold whatever MID's pad held)
                    int8_t *o = obase + pix * N + ch0;
                    if constexpr (TB == 2) st_out(o, make_uint2(packed[0], packed[1]));
                    else st_out(o, packed[0]);
                }
                if constexpr (PF) {
#pragma unroll
                    for (int ks = 0; ks < KSC; ++ks) B[ks] = Bn[ks];
                }
            }
        }
    };

    wg_sync(); // the fill is complete before any DMA lands
    const int nsteps = batch * NB;
    if (dq.step < nsteps) stage(dq.step, 0);
    const bool dbuf = p.dbuf != 0;
    int cur = 0;
    for (; dq.step < nsteps; dq.advance(tid)) {
        const int step = dq.step;
        if constexpr (!DWRES) {
            int q0 = us_q < NQ ? us_q : NQ - 1; // (a wave without units fetches the last group's: unconditional, so nothing of the step before stays live)
            asm volatile("" : "+s"(q0)); // (an address the compiler cannot prove loop-invariant: the loads stay here)
            wd = load_dw(q0), qcur = q0;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        wg_sync(); // this step's tile is in LDS; every wave has left the previous step's pointwise phase (MID is free)
        dq.top(tid);
        if (dbuf && dq.nxt < nsteps) stage(dq.nxt, cur ^ 1); // the other region was last read in the previous step's depthwise phase
        dw_phase(p.tile_off + cur * p.TILE);
        wg_sync(); // MID complete; the tile has been read
        if (!dbuf && dq.nxt < nsteps) stage(dq.nxt, 0); // the tile region is free: the next step's rows fly under the pointwise phase
        if (p.TB == 2) pw_items(step, std::integral_constant<int, 2>{});
        else pw_items(step, std::integral_constant<int, 1>{});
        if (dbuf) cur ^= 1;
    }
    dq.finish(tid);
