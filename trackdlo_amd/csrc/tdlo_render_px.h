// tdlo_render_px.h -- what the two result-image kernels (k_render, tdlo_render.hip; k_render_batch, tdlo_render_batch.hip) share, so that they cannot drift
// apart: the blend of four bytes and "this primitive covers this pixel".  Compiles for the host as well (tdlo_render_search.h's host form,
// tests/cpp/render_batch_host_test.cpp).
#pragma once
#include "tdlo_thick_line.h"

#if defined(__HIPCC__)
#define TDLO_PX __host__ __device__ __forceinline__
#else
#include <algorithm>
#define TDLO_PX inline
#endif

namespace tdlo {

#if !defined(__HIPCC__)
using std::max;
using std::min;
#endif

// 0.5 a + 0.5 b on four bytes at once, b = a & m, rounded half to even: s = a + b, out = (s >> 1) + ((s & 1) & ((s >> 1) & 1)).
// h = floor(s / 2) = (a & b) + ((a ^ b) >> 1) per byte; s & 1 = (a ^ b) & 1; an odd s is at most 509, so h + 1 <= 255: no carry leaves a byte.
TDLO_PX unsigned blend4(unsigned a, unsigned m) {
    const unsigned b = a & m, x = a ^ b;
    const unsigned h = (a & b) + ((x >> 1) & 0x7f7f7f7fu);
    return h + (x & h & 0x01010101u);
}

// one primitive against one pixel (bounding box first: the exact line test is 64-bit)
TDLO_PX bool covers(int kind, int c0, int r0, int c1, int r1, int size, int pc, int pr) {
    if (kind) { const int dx = pc - c0, dy = pr - r0; return dx * dx + dy * dy <= size * size; }
    const int hw = (size + 1) >> 1;
    if (pc < min(c0, c1) - hw || pc > max(c0, c1) + hw || pr < min(r0, r1) - hw || pr > max(r0, r1) + hw) return false;
    return within_half_width(Px{pc, pr}, Px{c0, r0}, Px{c1, r1}, size);
}

}  // namespace tdlo
