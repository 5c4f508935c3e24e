// k_conv_pool_body.inc -- the text of conv_pool_rt (k_conv_pool.hip: Conv2D + AveragePool2D) and of conv_maxpool_rt (k_conv_maxpool.hip:
// Conv2D + MaxPool2D), and of their launchers.  The including file defines
//   MF_CONV_POOL_KERNEL    the kernel's name
//   MF_CONV_POOL_MAX       0: phase B sums the in-range dwords of Y and runs avgpool_generic's arithmetic; 1: it takes their per-byte
//                          max and runs maxpool_generic's (k_common.hpp maxpool_requant)
//   MF_CONV_POOL_LAUNCH, MF_CONV_POOL_LAUNCH_T, MF_CONV_POOL_LAUNCH_W   the launcher's name and its two helpers'
// Steps, phases, plan, bands, barriers and LDS layout are the same for both: the comment at the top of k_conv_pool.hip.
template <int AL, bool WZ, int MG, uint32_t XR4>
__global__ __launch_bounds__(256) void MF_CONV_POOL_KERNEL(const int8_t *__restrict__ in, int8_t *__restrict__ out, ConvPoolArgs p, int batch) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = p.C, N = p.N, KS = p.KS, TB = p.TB, ROW = p.ROW, TILE = p.TILE, G = p.G, RB = p.RB, NT = p.NT;
    const int H = p.H, OH = p.OH, OW = p.OW, ROWB = p.W * C, NB = p.NB, NP = p.NP, YIMG = p.YIMG;
    const int POH = p.POH, POW = p.POW, NQ = (N + 3) >> 2;
    const int nblk = (NT + TB - 1) / TB;
    uint8_t *T = lds + p.xoff;
    const uint32_t izp4 = p.izp4;
    const PoolArgs &pl = p.pool;

    // resident weights: the whole image (1 KiB pieces)
    for (int b = wave * 64; b < NT * KS * 64; b += 256) dma16((const int8_t *)p.wimg + (size_t)(b + lane) * 16, lds + b * 16);
    for (int i = tid; i < (G * TILE + 256) / 16; i += 256) ((uint4 *)T)[i] = make_uint4(izp4, izp4, izp4, izp4);
    for (int i = tid; i < KS * 4; i += 256) ((int *)(lds + p.toff))[i] = p.tap[i];
    if constexpr (WZ)
        for (int i = tid; i < KS * 16; i += 256) ((uint32_t *)(lds + p.moff))[i] = p.kmask[i];
    // the convolution's per-channel constants [Kc | A | S | wzp][NT 16]: a chunk reads them at LDS latency, not through the L2
    for (int i = tid; i < NT * 16; i += 256) {
        int *c = (int *)(lds + p.coff);
        c[i] = p.Kc[i], c[NT * 16 + i] = __float_as_int(p.A[i]), c[NT * 32 + i] = __float_as_int(p.S[i]), c[NT * 48 + i] = p.wzp[i];
    }
    const int *tab = (const int *)(lds + p.toff);
    const uint8_t *cKc = lds + p.coff, *cA = cKc + NT * 64, *cS = cKc + NT * 128, *cZ = cKc + NT * 192;
    const int col = lane & 15, g = lane >> 4;
    const int nsteps = ((batch + G - 1) / G) * NB;
    const v4i ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    const bool dword_out = (N & 3) == 0 && ((uintptr_t)out & 3) == 0;
    wg_sync();
    for (int step = blockIdx.x; step < nsteps; step += gridDim.x) {
        const int band = step % NB, ist = step / NB;
        int py0, py1, c0, c1;
        conv_pool_band(OH, POH, p.PB, p.psh, p.pshy, p.PFH, band, py0, py1, c0, c1);
        const int yfirst = c0 * p.sh - p.padt;          // input row held by tile row 0
        wg_sync();                                       // the previous step's reads of the tile and of Y are done
        const int gvalid = min(G, batch - ist * G);
        const int rlo = yfirst < 0 ? -yfirst : 0, rhi = min(RB, H - yfirst); // the tile rows [rlo, rhi) lie inside the image
        if ((ROWB & 15) == 0) {
            for (int gi = 0; gi < gvalid; ++gi)
                for (int r = rlo + wave; r < rhi; r += 4) {
                    const int8_t *src = in + (((long)ist * G + gi) * H + yfirst + r) * (long)ROWB;
                    uint8_t *dst = T + gi * TILE + r * ROW + p.LP;
                    for (int o = 0; o < ROWB; o += 1024)
                        if (o + lane * 16 < ROWB) dma16(src + o + lane * 16, dst + o);
                }
        } else {
            // dword loads: the step's rows as one index space, four loads in flight per lane before the first store (a row of a small
            // image is a few dwords: a wave per row would wait out one memory latency per row)
            const int RW = ROWB >> 2, nr = rhi - rlo, per = nr * RW, total = gvalid * per;
            for (int base = tid; base < total; base += 1024) {
                uint32_t v[4];
                int at[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int idx = base + u * 256;
                    if (idx < total) {
                        const int gi = idx / per, w = idx - gi * per, r = w / RW, c = w - r * RW;
                        v[u] = *(const uint32_t *)(in + (((long)ist * G + gi) * H + yfirst + rlo + r) * (long)ROWB + c * 4);
                        at[u] = gi * TILE + (rlo + r) * ROW + p.LP + c * 4;
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (base + u * 256 < total) *(uint32_t *)(T + at[u]) = v[u];
            }
        }
        if (NB > 1)                                      // a band's rows outside the image: the input zero point again
            for (int gi = 0; gi < gvalid; ++gi)
                for (int r = wave; r < RB; r += 4)
                    if (r < rlo || r >= rhi)
                        for (int o = lane * 4; o < ROWB; o += 256) *(uint32_t *)(T + gi * TILE + r * ROW + p.LP + o) = izp4;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's DMAs (the first time: and the weights') have landed ...
        wg_sync();                                       // ... and every other wave's
        // ---- phase A: the band's convolution rows c0 .. c1 - 1 of every image of the step into Y ----
        const int bp = (c1 - c0) * OW, npix = gvalid * bp;
        for (int chunk = wave; chunk * 16 < npix; chunk += 4) {
            const int pp = chunk * 16 + col;
            const int pc = pp < npix ? pp : npix - 1;
            const int gi = pc / bp, rr = pc - gi * bp;
            const int oyl = rr / OW, ox = rr - oyl * OW;
            const bool live = pp < npix;
            const int wbase = p.xoff + gi * TILE + (oyl * p.sh) * ROW + p.LP + (ox * p.sw - p.padl) * C; // the window's LDS byte
            // operand B of k step ks: the 16 bytes at (window) + (table offset), from aligned reads
            auto operand = [&](int ks) -> v4i {
                const int off = wbase + tab[ks * 4 + g];
                if constexpr (AL == 16) {
                    return *(const v4i *)(lds + off);
                } else if constexpr (AL == 4) {
                    const uint32_t *q = (const uint32_t *)(lds + off);
                    return v4i{(int)q[0], (int)q[1], (int)q[2], (int)q[3]};
                } else {
                    const uint32_t *q = (const uint32_t *)(lds + (off & ~3));
                    const uint32_t sh = off & 3, d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], d4 = q[4];
                    return v4i{(int)__builtin_amdgcn_alignbyte(d1, d0, sh), (int)__builtin_amdgcn_alignbyte(d2, d1, sh),
                               (int)__builtin_amdgcn_alignbyte(d3, d2, sh), (int)__builtin_amdgcn_alignbyte(d4, d3, sh)};
                }
            };
            int rowsum = 0;
            if constexpr (WZ) {
                v4i acc = {0, 0, 0, 0};
                for (int ks = 0; ks < KS; ++ks) {
                    const v4i m = *(const v4i *)(lds + p.moff + (ks * 4 + g) * 16);
                    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, operand(ks) & m, acc, 0, 0, 0);
                }
                rowsum = acc[0];
            }
            uint8_t *ypix = lds + p.yoff + gi * YIMG + rr * NP;
            for (int blk = 0; blk < nblk; ++blk) {
                const int lt0 = blk * TB, tb = min(TB, NT - lt0);
                v4i acc[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i < tb) {
                        const int4 kc = magic4<MG>(*(const int4 *)(cKc + ((lt0 + i) * 16 + g * 4) * 4));
                        acc[i] = v4i{kc.x, kc.y, kc.z, kc.w};
                    }
                }
                for (int ks = 0; ks < KS; ++ks) {
                    const v4i b = operand(ks);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (i < tb) acc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(*(const v4i *)(lds + (((lt0 + i) * KS + ks) * 64 + lane) * 16), b, acc[i], 0, 0, 0);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int ch = (lt0 + i) * 16 + g * 4; // the lane's 4 output channels
                    if (i < tb && ch < N) {
                        v4i a = acc[i];
                        if constexpr (WZ) {
                            const int4 wz = *(const int4 *)(cZ + ch * 4);
                            a[0] -= wz.x * rowsum, a[1] -= wz.y * rowsum, a[2] -= wz.z * rowsum, a[3] -= wz.w * rowsum;
                        }
                        const uint32_t d = requant_pack4<MG, XR4>(a[0], a[1], a[2], a[3], *(const float4 *)(cA + ch * 4), *(const float4 *)(cS + ch * 4),
                                                                  p.lo_f, p.hi_f);
                        if (live) *(uint32_t *)(ypix + ch) = d; // (the quad's bytes past N, if any, are read by no one)
                    }
                }
            }
        }
        wg_sync();                                       // Y is complete
        // ---- phase B: the band's pooled rows py0 .. py1 - 1 from Y ----
        const int nprow = py1 - py0, items = gvalid * nprow * POW * NQ;
        for (int it = tid; it < items; it += 256) {
            const int q = it % NQ;
            int t = it / NQ;
            const int px = t % POW;
            t /= POW;
            const int pr = t % nprow, gi = t / nprow;
            const int py = py0 + pr;
            const uint8_t *yb = lds + p.yoff + gi * YIMG + q * 4;
#if MF_CONV_POOL_MAX
            // the max of the in-range dwords of Y, per byte: maxpool_c4's two packed 16-bit maxima per tap, maxpool_generic's arithmetic
            mf_short2 odd = {(short)-32768, (short)-32768}, even = odd;
            for (int ky = 0; ky < p.PFH; ++ky) {
                const int iy = py * p.psh + ky - p.pshy;
                if (iy < 0 || iy >= OH) continue;
                for (int kx = 0; kx < p.PFW; ++kx) {
                    const int ix = px * p.psw + kx - p.pshx;
                    if (ix >= 0 && ix < OW) {
                        const uint32_t v = *(const uint32_t *)(yb + ((iy - c0) * OW + ix) * NP);
                        odd = __builtin_elementwise_max(odd, __builtin_bit_cast(mf_short2, v));
                        even = __builtin_elementwise_max(even, __builtin_bit_cast(mf_short2, v << 8));
                    }
                }
            }
            const int r4[4] = {maxpool_requant((int)even.x >> 8, pl), maxpool_requant((int)odd.x >> 8, pl), maxpool_requant((int)even.y >> 8, pl),
                               maxpool_requant((int)odd.y >> 8, pl)};
#else
            int s0 = 0, s1 = 0, s2 = 0, s3 = 0, len = 0;
            for (int ky = 0; ky < p.PFH; ++ky) {
                const int iy = py * p.psh + ky - p.pshy;
                if (iy < 0 || iy >= OH) continue;
                for (int kx = 0; kx < p.PFW; ++kx) {
                    const int ix = px * p.psw + kx - p.pshx;
                    if (ix >= 0 && ix < OW) {
                        const uint32_t v = *(const uint32_t *)(yb + ((iy - c0) * OW + ix) * NP);
                        s0 = sdot4(v, 0x00000001u, s0), s1 = sdot4(v, 0x00000100u, s1);
                        s2 = sdot4(v, 0x00010000u, s2), s3 = sdot4(v, 0x01000000u, s3);
                        ++len;
                    }
                }
            }
            const float inv = __fdiv_rn(1.0f, (float)len);
            const int sums[4] = {s0, s1, s2, s3};
            int r4[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float x = __fmul_rn(inv, (float)(sums[k] + pl.bias * len));
                const float y = __fadd_rn(__fmul_rn(pl.c0, x), pl.c1);
                const float r = __fadd_rn(y, __builtin_copysignf(0x1.fffffep-2f, y));
                int v = (r != r) ? 0 : (int)__builtin_amdgcn_fmed3f(r, pl.sat_lo, pl.sat_hi); // NaN (len == 0) -> 0
                v = max(v, pl.lo);
                r4[k] = min(v, pl.hi);
            }
#endif
            const uint32_t d = pack4(r4[0], r4[1], r4[2], r4[3]) ^ (0x01010101u * (uint32_t)pl.xr);
            int8_t *dst = out + ((((size_t)ist * G + gi) * POH + py) * POW + px) * (size_t)N + q * 4;
            if (dword_out) {
                *(uint32_t *)dst = d;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (q * 4 + j < N) dst[j] = (int8_t)(d >> (8 * j));
            }
        }
    }
}

template <int AL, bool WZ, int MG, uint32_t XR4>
static void MF_CONV_POOL_LAUNCH_T(const int8_t *in, int8_t *out, const ConvPoolArgs &a, int batch, hipStream_t s) {
    int per_cu = 1;
    { // occupancy per (device, LDS bytes), asked once; the attribute is the whole budget, so no shape lowers it for another
        static std::mutex mu;
        static std::map<std::pair<int, int>, int> cache;
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> lock(mu);
        auto it = cache.find({dev, a.lds});
        if (it == cache.end()) {
            (void)hipFuncSetAttribute((const void *)MF_CONV_POOL_KERNEL<AL, WZ, MG, XR4>, hipFuncAttributeMaxDynamicSharedMemorySize, CONV_GEMM_LDS_MAX);
            int n = 1;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, MF_CONV_POOL_KERNEL<AL, WZ, MG, XR4>, 256, (size_t)a.lds) != hipSuccess || n < 1) {
                (void)hipGetLastError();
                n = 1;
            }
            it = cache.emplace(std::make_pair(dev, a.lds), n).first;
        }
        per_cu = it->second;
    }
    const long long nsteps = (long long)((batch + a.G - 1) / a.G) * a.NB;
    const long long walkers = std::min(std::max(1LL, 256LL * per_cu), nsteps); // persistent: the weights are staged once per workgroup
    MF_LAUNCH((MF_CONV_POOL_KERNEL<AL, WZ, MG, XR4>), dim3((unsigned)walkers), dim3(256), a.lds, s, in, out, a, batch);
}
template <int AL, int MG, uint32_t XR4>
static void MF_CONV_POOL_LAUNCH_W(const int8_t *in, int8_t *out, const ConvPoolArgs &a, bool wz, int batch, hipStream_t s) {
    if (wz) MF_CONV_POOL_LAUNCH_T<AL, true, MG, XR4>(in, out, a, batch, s);
    else MF_CONV_POOL_LAUNCH_T<AL, false, MG, XR4>(in, out, a, batch, s);
}
void MF_CONV_POOL_LAUNCH(const int8_t *in, int8_t *out, const ConvPoolArgs &a, bool wz, int batch, hipStream_t s) {
    if (batch <= 0) return;
    if (a.C % 16 == 0) MF_DISPATCH4(a.magic, a.xr, MF_CONV_POOL_LAUNCH_W, (in, out, a, wz, batch, s), 16)
    else if (a.C % 4 == 0) MF_DISPATCH4(a.magic, a.xr, MF_CONV_POOL_LAUNCH_W, (in, out, a, wz, batch, s), 4)
    else MF_DISPATCH4(a.magic, a.xr, MF_CONV_POOL_LAUNCH_W, (in, out, a, wz, batch, s), 1)
}

