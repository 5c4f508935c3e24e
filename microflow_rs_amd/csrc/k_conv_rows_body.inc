// k_conv_rows_body.inc -- the statements of conv_rows_lds<WZ, MG, XR4>, conv_rows_lds_f32<WZ, MG, XR4> and conv_rows_bytes<WZ, MG, XR4>
// (k_rt.hip), included between their braces.  Expects in, out, p (ConvRowsArgs), batch, eg (F32Edge) and the constants WZ, MG, XR4,
// F32IN, BYTES in scope.  BYTES: rows that are not whole dwords -- the staging map is conv_rows_bytes_map.hpp's, one packed register
// per element (el[]), and an element is fetched as the two aligned dwords that hold its bytes (v[], vhi[]): both stay in registers
// across the compute loop and meet (v_alignbyte, then the input zero point over the bytes past the row) at the tile write, so that
// the wait for the loads stays where conv_rows_lds has it.  Everything from the second barrier on is the same text for all three.
    constexpr int NTHR = 512, MAXE = 16;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x;
    const int KG = p.KG, KH = p.KH, TWP = p.TWP, TILE = p.TILE, G = p.G, NP = p.NP, NG8 = NP >> 3, N = p.N;
    const int W_OFF = G * TILE;                          // [KH][KG][NP] weight dwords
    const int M_OFF = W_OFF + KH * KG * NP * 4;          // [KG] byte masks of the real taps (WZ)
    const int C_OFF = M_OFF + ((KG * 4 + 15) & ~15);     // A, S, Kc, fzp: [NP] each
    for (int i = tid; i < G * TILE / 4; i += NTHR) ((uint32_t *)lds)[i] = p.izp4;
    for (int i = tid; i < KH * KG * NP; i += NTHR) ((uint32_t *)(lds + W_OFF))[i] = p.wpack[i];
    for (int i = tid; i < KG; i += NTHR) ((uint32_t *)(lds + M_OFF))[i] = p.mask[i];
    for (int i = tid; i < NP; i += NTHR) {
        const bool live = i < N;
        ((float *)(lds + C_OFF))[i] = live ? p.A[i] : 0.0f;
        ((float *)(lds + C_OFF + NP * 4))[i] = live ? p.S[i] : 0.0f;
        ((int *)(lds + C_OFF + NP * 8))[i] = (live ? p.Kc[i] : 0) + (MG != 0 ? MF_MAGIC_I : 0);
        ((int *)(lds + C_OFF + NP * 12))[i] = (WZ && live) ? p.wzp[i] : 0;
    }
    // staging map (the same for every step): dword e of this thread is image g, row y, dword x of the step
    const int ROWD = p.ROWB >> 2, IMGD = p.H * ROWD, STEPD = G * IMGD;
    int gofs[MAXE], lofs[MAXE];
    uint32_t el[BYTES ? MAXE : 1], vhi[BYTES ? MAXE : 1];
    const int IMGB = p.H * p.ROWB;                       // (BYTES) bytes of an image
    if constexpr (BYTES) {
#pragma unroll
        for (int e = 0; e < MAXE; ++e) el[e] = rows_bytes_elem(p, tid + NTHR * e);
    } else {
#pragma unroll
    for (int e = 0; e < MAXE; ++e) {
        const int idx = tid + NTHR * e;
        const int g = idx / IMGD, r = idx - g * IMGD, y = r / ROWD, x = r - y * ROWD;
        gofs[e] = idx < STEPD ? idx : -1;
        lofs[e] = g * TILE + (y + p.shy) * TWP + p.XO + 4 * x;
    }
    }
    const int nsteps = (batch + G - 1) / G;
    uint32_t v[MAXE];
    auto fetch = [&](int st) {
        if constexpr (BYTES) {
            const size_t sb = (size_t)st * G * IMGB;     // the step's first byte: src is the aligned dword that holds it
            const uint32_t *src = (const uint32_t *)in + (sb >> 2);
            const uint32_t low2 = (uint32_t)sb & 3u;
            const int lim = min(G, batch - st * G) * IMGB; // bytes of the step that exist (a ragged last step)
#pragma unroll
            for (int e = 0; e < MAXE; ++e) {
                // (indices selected, not addresses, as below; src[0] holds the step's first byte, so it is never wholly outside the
                // batch.  The loaded dwords are not touched here -- which of them count is decided again at the tile write: a select on
                // them in this place was a wait for the loads ahead of the compute loop)
                const RowsBytesSrc m = rows_bytes_src(el[e], low2, p.ROWB);
                const bool ok = el[e] != ROWS_BYTES_NONE && rows_bytes_first(el[e]) < lim;
                v[e] = src[ok ? m.d0 : 0];
            }
#pragma unroll
            for (int e = 0; e < MAXE; ++e) {       // (the second dwords behind all the first ones: sixteen loads in a row, twice)
                const RowsBytesSrc m = rows_bytes_src(el[e], low2, p.ROWB);
                const bool ok = el[e] != ROWS_BYTES_NONE && rows_bytes_first(el[e]) < lim;
                vhi[e] = src[ok && m.two ? m.d0 + 1 : 0];
                if (el[e] != ROWS_BYTES_NONE) el[e] = rows_bytes_keep(el[e], m.shift);
            }
            return;
        }
        const uint32_t *src = (const uint32_t *)in + (size_t)st * STEPD;
        const long lim = ((long)batch - (long)st * G) * IMGD; // dwords of the step that exist (a ragged last step)
#pragma unroll
        for (int e = 0; e < MAXE; ++e) {
            // (select the VALUE, not the address: `cond ? src[i] : p.izp4` made the compiler choose between a global and a
            // kernel-argument address, i.e. a flat load that also counts on lgkmcnt)
            const bool ok = gofs[e] >= 0 && gofs[e] < lim;
            const uint32_t got = src[ok ? gofs[e] : 0];
            v[e] = ok ? got : p.izp4;
        }
    };
    const float inv_ow = 1.0f / (float)p.OW, inv_opix = 1.0f / (float)(p.OH * p.OW);
    const int OPIX = p.OH * p.OW;
    int step = blockIdx.x;
    if constexpr (!F32IN)
        if (step < nsteps) fetch(step);
    for (; step < nsteps; step += gridDim.x) {
        wg_sync();                                 // the previous step's compute is done with the tiles
        if constexpr (F32IN) {
            // this step's float4s, eight in flight per thread, become its tile dwords (a ragged last step: izp4, as the int8 form --
            // kept for steps of several images, which the host declines today: with G = 1 every dword of a step exists)
            const float4 *src = (const float4 *)in + (size_t)step * STEPD;
            const long lim = ((long)batch - (long)step * G) * IMGD;
#pragma unroll
            for (int h = 0; h < MAXE; h += 8) {
                float4 f[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) f[e] = src[(gofs[h + e] >= 0 && gofs[h + e] < lim) ? gofs[h + e] : 0];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const uint32_t q = pack4(edge_quant(f[e].x, eg), edge_quant(f[e].y, eg), edge_quant(f[e].z, eg), edge_quant(f[e].w, eg)) ^ eg.in_xr4;
                    if (gofs[h + e] >= 0) *(uint32_t *)(lds + lofs[h + e]) = gofs[h + e] < lim ? q : p.izp4;
                }
            }
        } else if constexpr (BYTES) {
            const int lim = min(G, batch - step * G) * IMGB;
#pragma unroll
            for (int e = 0; e < MAXE; ++e) {
                // (vhi[e] may be a dword that was not wanted: its bytes then land past the real ones and rows_bytes_merge drops them)
                const uint32_t got = rows_bytes_merge(__builtin_amdgcn_alignbyte(vhi[e], v[e], rows_bytes_kept(el[e])), rows_bytes_real(el[e], p.ROWB), p.izp4);
                if (el[e] != ROWS_BYTES_NONE) *(uint32_t *)(lds + rows_bytes_tile(el[e])) = rows_bytes_first(el[e]) < lim ? got : p.izp4;
            }
        } else {
#pragma unroll
            for (int e = 0; e < MAXE; ++e)
                if (gofs[e] >= 0) *(uint32_t *)(lds + lofs[e]) = v[e];
        }
        wg_sync();
        if constexpr (!F32IN)
            if (step + gridDim.x < nsteps) fetch(step + gridDim.x); // in flight during the compute below
        const int gvalid = min(G, batch - step * G);
        for (int po = tid; po < G * OPIX; po += NTHR) {
            // pixel item -> (image, row, column); exact float divisions (indices < 2^22)
            const int g = (int)(((float)po + 0.5f) * inv_opix);
            const int o = po - g * OPIX;
            const int oy = (int)(((float)o + 0.5f) * inv_ow), ox = o - oy * p.OW;
            if (g >= gvalid) continue;
            for (int cgp = 0; cgp < NG8; ++cgp) {        // 8 output channels at a time
            int acc[8], wsum = 0;
            const int4 k0 = *(const int4 *)(lds + C_OFF + NP * 8 + cgp * 32), k1 = *(const int4 *)(lds + C_OFF + NP * 8 + cgp * 32 + 16);
            acc[0] = k0.x, acc[1] = k0.y, acc[2] = k0.z, acc[3] = k0.w, acc[4] = k1.x, acc[5] = k1.y, acc[6] = k1.z, acc[7] = k1.w;
            const int base0 = g * TILE + (oy * p.sh) * TWP + ox * p.sw * p.C + p.X0;
            for (int ky = 0; ky < KH; ++ky) {
                const int base = base0 + ky * TWP;
                const uint32_t *row = (const uint32_t *)(lds + (base & ~3));
                const uint32_t sh = (uint32_t)(base & 3);
                uint32_t lo = row[0];
                for (int kg = 0; kg < KG; ++kg) {
                    const uint32_t hi = row[kg + 1];
                    const uint32_t val = __builtin_amdgcn_alignbyte(hi, lo, sh); // window bytes 4 kg .. 4 kg + 3 of this row
                    lo = hi;
                    const uint4 w0 = *(const uint4 *)(lds + W_OFF + ((ky * KG + kg) * NP + cgp * 8) * 4);
                    const uint4 w1 = *(const uint4 *)(lds + W_OFF + ((ky * KG + kg) * NP + cgp * 8) * 4 + 16);
                    acc[0] = sdot4(val, w0.x, acc[0]), acc[1] = sdot4(val, w0.y, acc[1]);
                    acc[2] = sdot4(val, w0.z, acc[2]), acc[3] = sdot4(val, w0.w, acc[3]);
                    acc[4] = sdot4(val, w1.x, acc[4]), acc[5] = sdot4(val, w1.y, acc[5]);
                    acc[6] = sdot4(val, w1.z, acc[6]), acc[7] = sdot4(val, w1.w, acc[7]);
                    if constexpr (WZ) wsum = sdot4(val, ((const uint32_t *)(lds + M_OFF))[kg], wsum);
                }
            }
            if constexpr (WZ) {
                const int4 z0 = *(const int4 *)(lds + C_OFF + NP * 12 + cgp * 32), z1 = *(const int4 *)(lds + C_OFF + NP * 12 + cgp * 32 + 16);
                acc[0] -= z0.x * wsum, acc[1] -= z0.y * wsum, acc[2] -= z0.z * wsum, acc[3] -= z0.w * wsum;
                acc[4] -= z1.x * wsum, acc[5] -= z1.y * wsum, acc[6] -= z1.z * wsum, acc[7] -= z1.w * wsum;
            }
            const float4 a0 = *(const float4 *)(lds + C_OFF + cgp * 32), a1 = *(const float4 *)(lds + C_OFF + cgp * 32 + 16);
            const float4 s0 = *(const float4 *)(lds + C_OFF + NP * 4 + cgp * 32), s1 = *(const float4 *)(lds + C_OFF + NP * 4 + cgp * 32 + 16);
            const uint32_t d0 = requant_pack4<MG, XR4>(acc[0], acc[1], acc[2], acc[3], a0, s0, p.lo_f, p.hi_f);
            const uint32_t d1 = requant_pack4<MG, XR4>(acc[4], acc[5], acc[6], acc[7], a1, s1, p.lo_f, p.hi_f);
            int8_t *dst = out + ((size_t)(step * G + g) * OPIX + o) * N + cgp * 8;
            if ((N & 7) == 0) {
                st_out_t<false>(dst, make_uint2(d0, d1));
            } else {                                     // N not a multiple of 8: byte stores of the channels that exist
                const int nleft = N - cgp * 8;
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (c < nleft) dst[c] = (int8_t)(((c < 4 ? d0 : d1) >> (8 * (c & 3))) & 0xffu);
            }
            }
        }
    }
