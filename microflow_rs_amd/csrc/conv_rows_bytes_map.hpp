// conv_rows_bytes_map.hpp -- the staging map of conv_rows_bytes (k_rt.hip): where a dword of the LDS tile comes from when image rows
// are NOT whole dwords (ConvRowsArgs::BYTES()).  Host and device run this text: the kernel between its barriers, and
// tests/cpp/conv_rows_bytes_plan.cpp on the CPU, which stages whole batches through it and compares the tile byte for byte.
//
// A step's G images are ONE contiguous byte range of the batch that starts at byte step * G * H * ROWB of `in` (`in` itself is 16-byte
// aligned: mf_op_run's contract for every fast kernel).  A row of the tile is ceil(ROWB / 4) dwords that start at image column 0; tile
// dword x of row y of image g holds the bytes
//     r .. r + nbytes - 1   of the step,   r = (g * H + y) * ROWB + 4 x,   nbytes = min(4, ROWB - 4 x)
// and the input zero point in its other bytes (they are the right halo: without that a row's tail would hold the head of the next
// row).  Neither the step's first byte nor an image's nor a row's is dword aligned in general, so the bytes are taken from the two
// ALIGNED dwords that hold them, (4 d0 .. 4 d0 + 7) of the step's first aligned dword, shifted by the low two bits of the absolute
// byte address (v_alignbyte) -- a shift that differs per element and, where G * H * ROWB is odd, per step.
//   rows_bytes_elem : the part that is the same in every step, packed into ONE register per element (the kernel holds sixteen
//                     elements and both source dwords of each across the compute loop: 48 registers, what conv_rows_lds holds)
//   rows_bytes_src  : the part that depends on the step's first byte
//   rows_bytes_keep : the shift goes into the element's two free bits when its dwords are fetched and is read there at the tile write,
//                     a step later (which also keeps the register loop-carried: unpacked into its fields ahead of the step loop,
//                     the elements were 26 registers more than the launch bound leaves)
// The second dword is wanted only where the element's bytes do not end in the first (shift + nbytes > 4); the byte that makes it
// wanted lies in it, so a dword wholly outside the batch is never indexed.  The first dword holds byte r: an element of an image
// that exists never indexes a dword wholly outside the batch either.
#pragma once
#include <cstdint>

#include "kernels.hpp"

#if defined(__HIPCC__)
#define MF_ROWS_HD __host__ __device__ inline
#else
#define MF_ROWS_HD inline
#endif

namespace mf {
namespace k {

constexpr uint32_t ROWS_BYTES_NONE = 0xffffffffu;       // a staging slot past the step's last element

// slot idx (0 ..) of a step -> bit 31: the last dword of its row (nbytes = ROWB & 3; 4 elsewhere); bits 30..16: r, the element's first
// byte in the step; bits 15..2: its tile byte offset / 4 (the tiles of a step are G * TILE <= 64 KiB and a step is at most 8192
// dwords of rows: both fit); bits 1..0: the shift of the fetch in flight (rows_bytes_keep)
MF_ROWS_HD uint32_t rows_bytes_elem(const ConvRowsArgs &p, int idx) {
    const int ROWD = (p.ROWB + 3) >> 2, IMGD = p.H * ROWD;
    if (idx >= p.G * IMGD) return ROWS_BYTES_NONE;
    const int g = idx / IMGD, q = idx - g * IMGD, y = q / ROWD, x = q - y * ROWD;
    const int r = (g * p.H + y) * p.ROWB + 4 * x;
    const int lofs = g * p.TILE + (y + p.shy) * p.TWP + p.XO + 4 * x;
    return (x == ROWD - 1 ? 0x80000000u : 0u) | ((uint32_t)r << 16) | (uint32_t)lofs;
}
MF_ROWS_HD int rows_bytes_first(uint32_t elem) { return (int)((elem >> 16) & 0x7fffu); } // r
MF_ROWS_HD int rows_bytes_tile(uint32_t elem) { return (int)(elem & 0xfffcu); }    // tile byte offset

struct RowsBytesSrc {
    int d0;          // first source dword, counted from the step's first aligned dword ((step byte) >> 2 of `in`)
    bool two;        // dword d0 + 1 holds bytes of the element too
    uint32_t shift;  // byte of dword d0 that is byte 0 of the tile dword
    int nbytes;      // real bytes of the tile dword (1 .. 4); the rest is the input zero point
};
MF_ROWS_HD int rows_bytes_real(uint32_t elem, int ROWB) { return (elem >> 31) ? (ROWB & 3) : 4; }
// low2 = (the step's first byte) & 3
MF_ROWS_HD RowsBytesSrc rows_bytes_src(uint32_t elem, uint32_t low2, int ROWB) {
    const uint32_t b = (uint32_t)rows_bytes_first(elem) + low2;
    RowsBytesSrc s;
    s.d0 = (int)(b >> 2), s.shift = b & 3u, s.nbytes = rows_bytes_real(elem, ROWB);
    s.two = s.shift + (uint32_t)s.nbytes > 4u;
    return s;
}
MF_ROWS_HD uint32_t rows_bytes_keep(uint32_t elem, uint32_t shift) { return (elem & ~3u) | shift; }
MF_ROWS_HD uint32_t rows_bytes_kept(uint32_t elem) { return elem & 3u; }
// the tile dword from its two source dwords (hi is ignored where !two: its bytes land at or past nbytes)
MF_ROWS_HD uint32_t rows_bytes_merge(uint32_t aligned, int nbytes, uint32_t izp4) {
    const uint32_t m = 0xffffffffu >> (8 * (4 - nbytes));
    return (aligned & m) | (izp4 & ~m);
}

} // namespace k
} // namespace mf
