// k_resize_bilinear.hip -- RESIZE_BILINEAR (TFLite builtin 23; Keras' UpSampling2D(interpolation="bilinear")) of a rank-4 tensor by
// integer factors (sy, sx), align_corners = false, half_pixel_centers = true.  The reference has no such operator; the contract is
// include/microflow_amd.h's (mf_resize_bilinear_create).  Per axis at factor s, output index o = s q + p:
//     n = 2 p + 1 - s;   n >= 0: taps (q, q + 1), f = n;   n < 0: taps (q - 1, q), f = 2 s + n;   weights (2 s - f, f), taps clamped.
// acc = sum over the four taps of wy wx v, exact in integers; DD = 4 sy sx = the sum of the weights; ONE rounding, half away from zero on
// the value as T: i8 rounds sgn(acc) floor((|acc| + DD / 2) / DD), u8 rounds floor((acc + DD / 2) / DD).
//
// Both kernels work on the UNSIGNED byte u = v + 128 (the internal byte ^ 0x80, for either T): accu = sum w u = acc + 128 DD >= 0, and
//     u8:  out_u = floor((accu + DD / 2) / DD)
//     i8:  out + 128 = floor((accu + DD / 2 - [accu < 128 DD]) / DD)     (half up, and a tie below zero goes down: away from zero)
// and the stored byte is out_u ^ 0x80 either way.
//
// resize_bl_c4<V, SY, SX, U8>:
//   steps   : G whole images, or one band of BH source rows of one image (resize_bl_plan, under an LDS budget); workgroups walk the steps
//             persistently; a band's SY BH output rows are written by that workgroup alone.
//   tile    : source rows q0 - 1 .. q1 + 1 clamped to the image, each with pixel 0 repeated in front and pixel W - 1 behind, bytes already
//             flipped to unsigned: no tap of any output is tested or clamped afterwards.  Global loads of V (16 bytes, or a dword), a wave
//             per tile row.  (LDS-DMA cannot flip the bytes or repeat the edge pixels, so the loads go through registers.)
//   cell    : a thread owns one source word (row q, pixel x, channel word cw): it reads the 3 x 3 neighbourhood words once and produces the
//             SY SX output words of the cell.  Per dword the four channels are split into even and odd bytes, two 16-bit lanes per
//             register (accu + DD / 2 <= 255 * 64 + 32 < 2^16), and everything up to the division is packed 16-bit multiply-adds with
//             the weights as instruction constants: the horizontal sums of the three rows per x phase first (<= 255 * 2 SX, exact), then per
//             (py, px) the vertical sum with the rounding constant in the first multiply-add.
//   divide  : DD is a power of two (a packed shift) unless a factor is 3: DD in {12, 24, 36, 48} divides by a 32-bit multiply-shift per
//             lane, proved exact over the reachable range below (bl_div_exact, a static_assert).
//   stores  : whole words of V; the words of one output pixel are contiguous across neighbouring threads.
#include "k_common.hpp"

#include <algorithm>
#include <map>
#include <mutex>

namespace mf {
namespace k {

namespace {

typedef unsigned short pk16 __attribute__((ext_vector_type(2))); // two 16-bit lanes of one register

// phase p of factor S: the first tap's place in the (q - 1, q, q + 1) neighbourhood and the second tap's weight f (the first's: 2 S - f)
template <int S> struct BlPhase {
    static constexpr int n(int p) { return 2 * p + 1 - S; }
    static constexpr int first(int p) { return n(p) >= 0 ? 1 : 0; }
    static constexpr int f(int p) { return n(p) >= 0 ? n(p) : 2 * S + n(p); }
};

// x / DD for DD no power of two as (x * M) >> 20 with M = floor(2^20 / DD) + 1.  Let e = M DD - 2^20, 0 < e <= DD.  Then
// x M / 2^20 = x / DD + x e / (DD 2^20), and the floor is floor(x / DD) as long as x e < 2^20.  The dividend is accu + DD / 2 <=
// 255 DD + DD / 2 <= 12264 (DD = 48) and e <= 48: x e < 2^20.  The product x M < 256 DD (2^20 / DD + 1) < 2^29: no overflow.
// bl_div_exact checks every reachable dividend at compile time as well.
constexpr uint32_t bl_div_mul(int DD) { return (1u << 20) / (uint32_t)DD + 1; }
constexpr bool bl_div_exact(int DD) {
    for (uint32_t x = 0; x <= 255u * DD + DD / 2; ++x)
        if (((x * bl_div_mul(DD)) >> 20) != x / DD) return false;
    return true;
}
static_assert(bl_div_exact(12) && bl_div_exact(24) && bl_div_exact(36) && bl_div_exact(48), "the factor-3 multiply-shift is not exact");

constexpr int bl_log2(int v) { return v <= 1 ? 0 : 1 + bl_log2(v / 2); }

// both lanes of t divided by DD; the results (<= 255) in bits 0..7 and 16..23
template <int DD> __device__ __forceinline__ uint32_t bl_div(pk16 t) {
    if constexpr ((DD & (DD - 1)) == 0) {
        return __builtin_bit_cast(uint32_t, (pk16)(t >> (unsigned short)bl_log2(DD)));
    } else {
        const uint32_t u = __builtin_bit_cast(uint32_t, t);
        return (((u & 0xffffu) * bl_div_mul(DD)) >> 20) | ((((u >> 16) * bl_div_mul(DD)) >> 20) << 16);
    }
}

// One dword (four channels) of a cell: t[dy][dx] the 3 x 3 neighbourhood dwords (unsigned bytes), o[py][px] the SY SX output dwords
// (internal bytes).
template <int SY, int SX, bool U8> __device__ __forceinline__ void bl_dword(const uint32_t (&t)[3][3], uint32_t (&o)[SY][SX]) {
    constexpr int DD = 4 * SY * SX;
    constexpr unsigned short RC = U8 ? DD / 2 : DD / 2 - 1;       // the rounding constant; i8 adds [accu >= 128 DD] below
    // bit 15 of (accu + 32768 - 128 DD) is [accu >= 128 DD]: accu + 32768 - 128 DD <= 32768 + 127 DD <= 40896 < 2^16.  The sum at hand
    // is accu + RC, so the constant added to it is 32768 - 128 DD - RC
    constexpr unsigned short KZ = 32768 - 128 * DD - (DD / 2 - 1);
    typedef BlPhase<SY> PY;
    typedef BlPhase<SX> PX;
    uint32_t eo[2][SY][SX];
#pragma unroll
    for (int half = 0; half < 2; ++half) { // even bytes (channels 0, 2), odd bytes (channels 1, 3)
        pk16 h[3][SX];                      // the horizontal sums of the three rows, per x phase: <= 255 * 2 SX
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            pk16 a[3];
#pragma unroll
            for (int x = 0; x < 3; ++x) a[x] = __builtin_bit_cast(pk16, (half ? t[r][x] >> 8 : t[r][x]) & 0x00ff00ffu);
#pragma unroll
            for (int px = 0; px < SX; ++px) {
                h[r][px] = a[PX::first(px)] * (unsigned short)(2 * SX - PX::f(px));
                if (PX::f(px)) h[r][px] = a[PX::first(px) + 1] * (unsigned short)PX::f(px) + h[r][px];
            }
        }
#pragma unroll
        for (int py = 0; py < SY; ++py)
#pragma unroll
            for (int px = 0; px < SX; ++px) {
                pk16 acc = h[PY::first(py)][px] * (unsigned short)(2 * SY - PY::f(py)) + RC;
                if (PY::f(py)) acc = h[PY::first(py) + 1][px] * (unsigned short)PY::f(py) + acc;
                if (!U8) acc = acc + ((acc + KZ) >> (unsigned short)15);
                eo[half][py][px] = bl_div<DD>(acc);
            }
    }
#pragma unroll
    for (int py = 0; py < SY; ++py)
#pragma unroll
        for (int px = 0; px < SX; ++px) o[py][px] = (eo[0][py][px] | (eo[1][py][px] << 8)) ^ 0x80808080u;
}

template <typename V> union BlWord {
    V v;
    uint32_t d[sizeof(V) / 4];
};

// i / d for i, d < 2^16 with m = ceil(2^32 / d): e = m d - 2^32 < d, i m / 2^32 = i / d + i e / (d 2^32) and i e < 2^32
__device__ __forceinline__ int bl_idiv(int i, uint32_t m, int d) { return d == 1 ? i : (int)__umulhi((uint32_t)i, m); }

} // namespace

template <typename V, int SY, int SX, bool U8>
__global__ __launch_bounds__(256) void resize_bl_c4(const int8_t *__restrict__ in, int8_t *__restrict__ out, ResizeBlArgs p, size_t batch) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    constexpr int NW = sizeof(V) / 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = p.H, C = p.C, G = p.G, BH = p.BH, NBANDS = p.NBANDS, ROWP = p.ROWP, TILE = p.TILE;
    const int wpp = p.wpp, wpr = p.wpr, twr = wpr + 2 * wpp; // words per pixel, per source row, per tile row
    const size_t owpr = (size_t)wpr * SX;                    // words per output row
    const size_t nsteps = (batch + G - 1) / G * NBANDS;
    for (size_t step = blockIdx.x; step < nsteps; step += gridDim.x) {
        const int band = (int)(step % NBANDS);
        const size_t img0 = step / NBANDS * G;
        const int gvalid = (int)min((size_t)G, batch - img0);
        const int q0 = band * BH, rows = min(BH, H - q0), trows = rows + 2;
        wg_sync(); // the previous step's reads of the tile are done
        // stage: tile row tr of image g holds source row clamp(q0 - 1 + tr); tile word w holds source word w - wpp, the first and the last
        // pixel once more in front and behind
        for (int item = wave; item < gvalid * trows; item += 4) {
            const int g = item / trows, tr = item - g * trows;
            const int y = min(max(q0 - 1 + tr, 0), H - 1);
            const V *src = (const V *)(in + ((img0 + g) * H + y) * (size_t)p.ROWB);
            V *dst = (V *)(lds + g * TILE + tr * ROWP);
            for (int w = lane; w < twr; w += 64) {
                const int sw = w < wpp ? w : (w >= wpr + wpp ? w - 2 * wpp : w - wpp);
                BlWord<V> v;
                v.v = src[sw];
#pragma unroll
                for (int j = 0; j < NW; ++j) v.d[j] ^= 0x80808080u;
                dst[w] = v.v;
            }
        }
        wg_sync();
        const int ncells = gvalid * rows * wpr; // (below 2^16: a tile is at most 32 KiB)
        for (int i = tid; i < ncells; i += 256) {
            const int rr = bl_idiv(i, p.m_wpr, wpr), w = i - rr * wpr;
            const int g = G == 1 ? 0 : bl_idiv(rr, p.m_bh, BH), r = rr - g * BH; // (G > 1: whole images, rows == BH)
            const int x = bl_idiv(w, p.m_wpp, wpp), cw = w - x * wpp;
            const uint8_t *cell = lds + g * TILE + (r + 1) * ROWP + (w + wpp) * (int)sizeof(V);
            BlWord<V> nb[3][3], o[SY][SX];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) nb[dy][dx].v = *(const V *)(cell + (dy - 1) * ROWP + (dx - 1) * C);
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                uint32_t t[3][3], od[SY][SX];
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) t[dy][dx] = nb[dy][dx].d[j];
                bl_dword<SY, SX, U8>(t, od);
#pragma unroll
                for (int py = 0; py < SY; ++py)
#pragma unroll
                    for (int px = 0; px < SX; ++px) o[py][px].d[j] = od[py][px];
            }
            // output rows SY R .. SY R + SY - 1 of source row R (counted over the batch); pixel SX x + px, the same channel word
            V *dst = (V *)out + ((img0 + g) * H + q0 + r) * SY * owpr + (size_t)(w - cw) * SX + cw;
#pragma unroll
            for (int py = 0; py < SY; ++py)
#pragma unroll
                for (int px = 0; px < SX; ++px) dst[(size_t)py * owpr + (size_t)px * wpp] = o[py][px].v;
        }
    }
}

// The contract in plain C++: one output byte per thread and step; any shape, factors and pointers.
__global__ __launch_bounds__(256) void resize_bl_generic(const int8_t *__restrict__ in, int8_t *__restrict__ out, ResizeArgs p, int u8, size_t total) {
    const size_t C = (size_t)p.C, OW = (size_t)p.W * p.sx, OH = (size_t)p.H * p.sy;
    const long long DD = 4LL * p.sy * p.sx;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t c = i % C, px = i / C;
        const size_t ox = px % OW, row = px / OW;
        const size_t oy = row % OH, img = row / OH;
        int tap[2][2], wgt[2][2]; // [axis][tap]
        for (int ax = 0; ax < 2; ++ax) {
            const int s = ax ? p.sx : p.sy, lim = (ax ? p.W : p.H) - 1, o = (int)(ax ? ox : oy);
            const int q = o / s, n = 2 * (o - q * s) + 1 - s;
            const int i0 = n >= 0 ? q : q - 1, f = n >= 0 ? n : 2 * s + n;
            tap[ax][0] = min(max(i0, 0), lim), tap[ax][1] = min(max(i0 + 1, 0), lim);
            wgt[ax][0] = 2 * s - f, wgt[ax][1] = f;
        }
        const int8_t *ip = in + img * (size_t)p.H * p.W * C + c;
        long long acc = 0;
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) {
                const int8_t v = ip[((size_t)tap[0][a] * p.W + tap[1][b]) * C];
                acc += (long long)wgt[0][a] * wgt[1][b] * (u8 ? (int)(uint8_t)(v ^ 0x80) : (int)v);
            }
        const long long r = acc >= 0 ? (acc + DD / 2) / DD : -((-acc + DD / 2) / DD);
        out[i] = u8 ? (int8_t)((uint8_t)r ^ 0x80) : (int8_t)r;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
// 32 KiB of tile per workgroup: four workgroups per CU stage and compute side by side, which is what hides a step's load latency (the
// kernel has no second buffer).  G whole images (at most 16), else bands of equal height.
bool resize_bl_plan(ResizeBlArgs &a, int H, int W, int C, int sy, int sx, bool u8) {
    if (H < 1 || W < 1 || C < 4 || C % 4 != 0 || sy < 1 || sx < 1 || sy > 4 || sx > 4 || (sy == 1 && sx == 1)) return false;
    const long long cap = 32 * 1024, rowp = (((long long)W + 2) * C + 15) & ~15ll;
    if (3 * rowp > cap) return false;
    a = ResizeBlArgs{};
    a.H = H, a.W = W, a.C = C, a.sy = sy, a.sx = sx, a.u8 = u8;
    a.unit = C % 16 == 0 ? 16 : 4;
    a.wpp = C / a.unit, a.wpr = W * a.wpp;
    a.ROWB = W * C, a.ROWP = (int)rowp;
    if (((long long)H + 2) * rowp <= cap) {
        a.NBANDS = 1, a.BH = H;
        a.G = (int)std::min(16ll, cap / (((long long)H + 2) * rowp));
    } else {
        const int fit = (int)(cap / rowp) - 2, nb = (H + fit - 1) / fit;
        a.BH = (H + nb - 1) / nb, a.NBANDS = (H + a.BH - 1) / a.BH, a.G = 1;
    }
    a.RB = a.BH + 2, a.TILE = a.RB * a.ROWP, a.lds = a.G * a.TILE;
    auto magic = [](int d) { return (uint32_t)(((1ull << 32) + (uint64_t)d - 1) / (uint64_t)d); }; // (d == 1: not used, bl_idiv)
    a.m_wpr = magic(a.wpr), a.m_bh = magic(a.BH), a.m_wpp = magic(a.wpp);
    return true;
}

template <typename V, int SY, int SX, bool U8> static void launch_bl_t(const int8_t *in, int8_t *out, const ResizeBlArgs &a, size_t batch, hipStream_t s) {
    int per_cu = 1;
    { // occupancy per (device, LDS bytes), asked once
        static std::mutex mu;
        static std::map<std::pair<int, int>, int> cache;
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> lock(mu);
        auto it = cache.find({dev, a.lds});
        if (it == cache.end()) {
            int n = 1;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, resize_bl_c4<V, SY, SX, U8>, 256, (size_t)a.lds) != hipSuccess || n < 1) {
                (void)hipGetLastError();
                n = 1;
            }
            it = cache.emplace(std::make_pair(dev, a.lds), n).first;
        }
        per_cu = it->second;
    }
    // persistent.  The plan's G is the most images a step's tiles hold; where the batch leaves the grid fewer than two steps per resident
    // workgroup, fewer images per step (the same tiles, fewer used) make more, shorter steps
    ResizeBlArgs b = a;
    const unsigned long long resident = 256ull * (unsigned long long)per_cu;
    while (b.G > 1 && (batch + b.G - 1) / b.G * (size_t)b.NBANDS < 2 * resident) b.G = (b.G + 1) / 2;
    const unsigned long long nsteps = (unsigned long long)((batch + b.G - 1) / b.G) * b.NBANDS;
    MF_LAUNCH((resize_bl_c4<V, SY, SX, U8>), dim3((unsigned)std::min(resident, nsteps)), dim3(256), (size_t)b.lds, s, in, out, b, batch);
}

template <typename V, bool U8> static void launch_bl_factors(const int8_t *in, int8_t *out, const ResizeBlArgs &a, size_t batch, hipStream_t s) {
#define MF_BL(SY, SX) \
    case SY * 8 + SX: launch_bl_t<V, SY, SX, U8>(in, out, a, batch, s); break;
    switch (a.sy * 8 + a.sx) {
        MF_BL(1, 2) MF_BL(1, 3) MF_BL(1, 4)
        MF_BL(2, 1) MF_BL(2, 2) MF_BL(2, 3) MF_BL(2, 4)
        MF_BL(3, 1) MF_BL(3, 2) MF_BL(3, 3) MF_BL(3, 4)
        MF_BL(4, 1) MF_BL(4, 2) MF_BL(4, 3) MF_BL(4, 4)
    default: fprintf(stderr, "resize_bl_c4: no instance for factors (%d, %d)\n", a.sy, a.sx), abort(); // (resize_bl_plan admits none)
    }
#undef MF_BL
}

void launch_resize_bl(const int8_t *in, int8_t *out, const ResizeBlArgs &a, size_t batch, hipStream_t s) {
    if (!batch) return;
    if (a.unit == 16) a.u8 ? launch_bl_factors<u32x4, true>(in, out, a, batch, s) : launch_bl_factors<u32x4, false>(in, out, a, batch, s);
    else a.u8 ? launch_bl_factors<uint32_t, true>(in, out, a, batch, s) : launch_bl_factors<uint32_t, false>(in, out, a, batch, s);
}

void launch_resize_bl_generic(const int8_t *in, int8_t *out, const ResizeArgs &a, bool u8, size_t batch, hipStream_t s) {
    const size_t total = batch * (size_t)a.H * a.sy * (size_t)a.W * a.sx * (size_t)a.C;
    MF_LAUNCH(resize_bl_generic, dim3(grid_for(total)), dim3(256), 0, s, in, out, a, (int)u8, total);
}

} // namespace k
} // namespace mf
