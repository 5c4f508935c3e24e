// k_windows.hip -- sliding windows of a larger source gathered into the dense batch the model launches read (gfx950).
//
//   window_gather          bytes -> bytes (i8, or u8 with ^ 0x80 on the way: the internal domain of a u8 model)
//   window_gather_quantize f32   -> bytes, q = sat(roundf(x / scale + zp)) per element (quant_byte, k_common.hpp: the arithmetic
//                          of the separate quantise pass, with the 3-instruction division where the host verified it)
//
// One thread owns one 16-byte-aligned chunk of the DESTINATION and stores it with one dwordx4; only the first and the last chunk
// of a launch can be partial (a destination that does not start or end on a 16-byte boundary) and take dword / byte stores.  A
// chunk is cut into runs, each inside one window row: with 40-byte rows a chunk holds parts of two rows, with 1-element rows
// sixteen, and where the window size is no multiple of 16 a chunk continues into the next window.  The walk from run to run is
// incremental (row, then window column, window row, source); the divisions that find a chunk's first run are done once per chunk,
// in 32 bits when the launch is small enough (WinArgs::narrow).
//
// The source may sit at any byte address and every run may start at any byte.  A run is read as the ALIGNED dwords that hold
// its bytes -- the first four of them as one global_load_dwordx4, which needs dword alignment only, when every one of the four
// holds bytes of the run -- and byte-aligned in registers with v_alignbit_b32.  No load is misaligned.  An aligned dword that
// holds one byte of the source lies in that byte's page, so the (at most 3 + 3) bytes read beside a run never fault and are
// never stored: they are masked off before the run is merged into the chunk.  The f32 source is read element by element, all
// sixteen loads of a chunk in flight at once (four float4 where the run is sixteen elements of whole 16-byte lines).
//
// Consecutive chunks belong to consecutive threads and workgroups: windows that overlap are read by workgroups that run close
// together, and the overlap comes from L2 / the Infinity Cache.  All source offsets are size_t (a source may exceed 4 GiB).
#include "k_common.hpp"

namespace mf {
namespace k {

namespace {

// where a chunk's next element comes from
struct WinWalk {
    size_t s, iy, ix;  // the window: source, window row, window column
    size_t base;       // source element of the window's (0, 0)
    uint32_t r, e;     // row inside the window, element inside the row

    __device__ __forceinline__ void set_base(const WinArgs &a) { base = s * a.src_stride + iy * a.hop_row_stride + ix * a.hop_elems; }
    // g: byte of the launch's dense output
    __device__ __forceinline__ void seek(const WinArgs &a, size_t g) {
        uint32_t o;
        if (a.narrow) {
            const uint32_t g32 = (uint32_t)g, q = g32 / a.E;
            o = g32 - q * a.E;
            const uint32_t w32 = (uint32_t)a.first + q, nx32 = (uint32_t)a.nx, ny32 = (uint32_t)a.ny, t = w32 / nx32;
            ix = w32 - t * nx32;
            const uint32_t s32 = t / ny32;
            iy = t - s32 * ny32, s = s32;
        } else {
            const size_t q = g / a.E;
            o = (uint32_t)(g - q * a.E);
            const size_t w = a.first + q, t = w / a.nx;
            ix = w - t * a.nx;
            s = t / a.ny;
            iy = t - s * a.ny;
        }
        r = o / a.WE;
        e = o - r * a.WE;
        set_base(a);
    }
    __device__ __forceinline__ size_t at(const WinArgs &a) const { return base + (size_t)r * a.src_pitch + e; }
    __device__ __forceinline__ void next_row(const WinArgs &a) {
        e = 0;
        if (++r < a.WR) return;
        r = 0;
        if (++ix == a.nx) {
            ix = 0;
            if (++iy == a.ny) iy = 0, ++s;
        }
        set_base(a);
    }
};

// bytes [p, p + L) (1 <= L <= 16) as the low bytes of four dwords; what lies above them is masked off
__device__ __forceinline__ u32x4 load_run(const uint8_t *p, uint32_t L) {
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3), nd = (mis + L + 3) >> 2; // 1 .. 5 aligned dwords hold the run
    const uint32_t *q = (const uint32_t *)(p - mis); // (pointer arithmetic, not an integer round trip: the loads stay global loads)
    uint32_t d0, d1 = 0, d2 = 0, d3 = 0, d4 = 0;
    if (nd >= 4) { // four dwords that all hold bytes of the run: one dwordx4, which asks for dword alignment only
        typedef u32x4 u32x4_dword_aligned __attribute__((aligned(4)));
        const u32x4 v = *(const u32x4_dword_aligned *)q;
        d0 = v[0], d1 = v[1], d2 = v[2], d3 = v[3];
        if (nd > 4) d4 = q[4];
    } else {
        d0 = q[0];
        if (nd > 1) d1 = q[1];
        if (nd > 2) d2 = q[2];
    }
    const uint32_t sh = mis * 8;
    u32x4 v;
    v[0] = __builtin_amdgcn_alignbit(d1, d0, sh), v[1] = __builtin_amdgcn_alignbit(d2, d1, sh);
    v[2] = __builtin_amdgcn_alignbit(d3, d2, sh), v[3] = __builtin_amdgcn_alignbit(d4, d3, sh);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int keep = (int)L - 4 * i; // bytes of dword i inside the run
        v[i] &= keep >= 4 ? 0xffffffffu : keep <= 0 ? 0u : (1u << (8 * keep)) - 1u;
    }
    return v;
}
// acc |= v << (8 pos bytes); v holds no byte that would leave the chunk (pos + L <= 16)
__device__ __forceinline__ void merge_run(u32x4 &acc, const u32x4 &v, uint32_t pos) {
    const uint32_t ws = pos >> 2, bs = (pos & 3) * 8;
    uint32_t y0 = v[0], y1 = v[1], y2 = v[2], y3 = v[3];
    if (bs) {
        y3 = __builtin_amdgcn_alignbit(v[3], v[2], 32 - bs), y2 = __builtin_amdgcn_alignbit(v[2], v[1], 32 - bs);
        y1 = __builtin_amdgcn_alignbit(v[1], v[0], 32 - bs), y0 = v[0] << bs;
    }
    acc[0] |= ws == 0 ? y0 : 0u;
    acc[1] |= ws == 0 ? y1 : ws == 1 ? y0 : 0u;
    acc[2] |= ws == 0 ? y2 : ws == 1 ? y1 : ws == 2 ? y0 : 0u;
    acc[3] |= ws == 0 ? y3 : ws == 1 ? y2 : ws == 2 ? y1 : y0;
}
// bytes [pos, pos + n) of `acc` to the 16-byte line `line`: the whole line, or -- first / last chunk of a launch -- its dwords and bytes
__device__ __forceinline__ void store_chunk(int8_t *line, const u32x4 &acc, uint32_t pos, uint32_t n) {
    if (n == 16) {
        *(u32x4 *)line = acc;
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t lo = 4 * i, d = acc[i];
        if (pos <= lo && lo + 4 <= pos + n) {
            ((uint32_t *)line)[i] = d;
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (lo + b >= pos && lo + b < pos + n) line[lo + b] = (int8_t)(d >> (8 * b));
        }
    }
}
// chunk c of the destination: its line, the position of its first byte of this launch inside the line, the dense output byte that
// goes there, and how many follow
__device__ __forceinline__ uint32_t chunk_range(const WinArgs &a, uint32_t head, size_t c, uint32_t &pos, size_t &g) {
    const size_t d0 = c * 16, end = (size_t)head + a.total;
    const size_t lo = d0 < head ? (size_t)head : d0, hi = d0 + 16 < end ? d0 + 16 : end;
    pos = (uint32_t)(lo - d0);
    g = lo - head;
    return (uint32_t)(hi - lo);
}

} // namespace

// line0: dst rounded down to 16 bytes; head = dst - line0; nchunks = ceil((head + total) / 16)
__global__ __launch_bounds__(256) void window_gather(const uint8_t *__restrict__ src, int8_t *__restrict__ line0, uint32_t head, size_t nchunks,
                                                     WinArgs a) {
    for (size_t c = (size_t)blockIdx.x * 256 + threadIdx.x; c < nchunks; c += (size_t)gridDim.x * 256) {
        uint32_t pos;
        size_t g;
        const uint32_t n = chunk_range(a, head, c, pos, g);
        WinWalk w;
        w.seek(a, g);
        u32x4 acc = {0u, 0u, 0u, 0u};
        for (uint32_t p = pos, rem = n; rem;) {
            const uint32_t left = a.WE - w.e, L = left < rem ? left : rem;
            merge_run(acc, load_run(src + w.at(a), L), p);
            p += L, rem -= L;
            if (L == left) w.next_row(a);
            else w.e += L;
        }
        acc ^= a.xr4;
        store_chunk(line0 + c * 16, acc, pos, n);
    }
}

__global__ __launch_bounds__(256) void window_gather_quantize(const float *__restrict__ src, int8_t *__restrict__ line0, uint32_t head,
                                                              size_t nchunks, WinArgs a) {
    for (size_t c = (size_t)blockIdx.x * 256 + threadIdx.x; c < nchunks; c += (size_t)gridDim.x * 256) {
        uint32_t pos;
        size_t g;
        const uint32_t n = chunk_range(a, head, c, pos, g);
        WinWalk w;
        w.seek(a, g);
        // all sixteen loads are issued before the first value is used: the walk from element to element is address arithmetic only
        float x[16];
        const float *p = src + w.at(a);
        if (n == 16 && a.WE - w.e >= 16 && ((uintptr_t)p & 15) == 0) { // one run of whole 16-byte lines
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float4 f = ((const float4 *)p)[v];
                x[4 * v] = f.x, x[4 * v + 1] = f.y, x[4 * v + 2] = f.z, x[4 * v + 3] = f.w;
            }
        } else {
            size_t at[16];
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                at[b] = w.at(a);
                if ((uint32_t)b >= pos && (uint32_t)b < pos + n && ++w.e == a.WE) w.next_row(a);
            }
#pragma unroll
            for (int b = 0; b < 16; ++b) x[b] = ((uint32_t)b >= pos && (uint32_t)b < pos + n) ? src[at[b]] : 0.0f;
        }
        u32x4 acc = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const int q = quant_byte(x[b], a.scale, a.rcp, a.fast != 0, a.zp_f, a.sat_lo, a.sat_hi);
            acc[b >> 2] |= (uint32_t)(q & 0xff) << (8 * (b & 3));
        }
        acc ^= a.xr4;
        store_chunk(line0 + c * 16, acc, pos, n);
    }
}

template <typename Kern, typename Src> static void launch_windows(Kern kern, const Src *src, int8_t *dst, const WinArgs &a, hipStream_t s) {
    if (!a.total) return;
    const uint32_t head = (uint32_t)((uintptr_t)dst & 15);
    const size_t nchunks = ((size_t)head + a.total + 15) / 16;
    MF_LAUNCH(kern, dim3(grid_for(nchunks, 256, 1 << 20)), dim3(256), 0, s, src, dst - head, head, nchunks, a);
}
void launch_window_gather(const void *src, int8_t *dst, const WinArgs &a, hipStream_t s) {
    launch_windows(window_gather, (const uint8_t *)src, dst, a, s);
}
void launch_window_gather_quantize(const float *src, int8_t *dst, const WinArgs &a, hipStream_t s) {
    launch_windows(window_gather_quantize, src, dst, a, s);
}

} // namespace k
} // namespace mf
