// tdlo_render_search.h -- what one lane of k_render_batch (tdlo_render_batch.hip) does for its four consecutive pixels p0 .. p0 + 3 of one image: the loads,
// the two-level search for the LAST primitive that covers each pixel, the blend and the stores.  A header of its own, like tdlo_view_lane.h, so that
// the very code the GPU runs can be compiled for the host and run one "lane" at a time under a sanitizer on images and tables allocated at exactly
// their sizes (tests/cpp/render_batch_host_test.cpp).
//
// The picture (include/trackdlo_hip.h, tdlo_render_result_batch): blend once, then the image's ropes in list order, each as k_render draws its one rope.
// Painting order is turned round as in k_render: a pixel takes the colour of the last primitive of the last rope that covers it, so the search runs
// from the end and stops at the first hit -- no pixel is written twice, no list, no capacity.
//   rope level       from the image's last rope to its first, in rounds of 64: lane l tests the head box of rope (base - l) against the wave's row / column
//                    span; the ballot is walked from the rope drawn last.
//   primitive level  inside a surviving rope, from its last primitive to its first, in rounds of 64, exactly as k_render searches its table; the records
//                    are read through wave-uniform addresses (scalar loads).
//   the wave stops as soon as every pixel of it has its colour.
// On the host a vote is a loop over the 64 candidates (their tests depend on the wave's span alone, not on the lane), "wave-uniform" is the value itself
// and "every pixel of the wave" is the lane's own four: the same colours, since a lane that has its four is not changed by what the wave does next.
// Nothing outside [colour, colour + 3 P), [occluder, occluder + P), [out, out + 3 P) is touched: full lanes move dwords (the pointers are 4-byte aligned,
// p0 is a multiple of 4), the image's last 1 .. 3 pixels go byte by byte.
#pragma once
#include <stddef.h>
#include "tdlo_render_px.h"

namespace tdlo {

struct RenderSpan { int r_lo, r_hi, c_lo, c_hi; };             // rows of a wave's 256 flat pixels; within one row, its columns
struct alignas(16) RenderI4 { int x, y, z, w; };              // one aligned 16-byte access
struct alignas(8) RenderI2 { int x, y; };

TDLO_PX RenderSpan render_span(int wave_first, int P, int cols) {
    const int wave_last = min(wave_first + 4 * 64 - 1, P - 1);
    const int r_lo = wave_first / cols, r_hi = wave_last / cols;
    return RenderSpan{r_lo, r_hi, r_lo == r_hi ? wave_first - r_lo * cols : 0, r_lo == r_hi ? wave_last - r_hi * cols : cols - 1};
}

template <class F> TDLO_PX unsigned long long render_vote(int lane, F f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ballot(f(lane));
#else
    (void)lane;
    unsigned long long m = 0ull;
    for (int l = 0; l < 64; ++l) if (f(l)) m |= 1ull << l;
    return m;
#endif
}

TDLO_PX int render_uniform(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane(v);
#else
    return v;
#endif
}

TDLO_PX bool render_all_done(unsigned done) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ballot(done != 0xfu) == 0ull;
#else
    return done == 0xfu;
#endif
}

// the lane's colour words (12 bytes) and occluder bytes (0xff each without an occluder); n = min(4, P - p0), <= 0: a lane behind the image loads nothing
TDLO_PX void render_load4(const unsigned char *colour, const unsigned char *occluder, int p0, int n, unsigned &c0, unsigned &c1, unsigned &c2, unsigned &o4) {
    c0 = 0u; c1 = 0u; c2 = 0u; o4 = 0xffffffffu;
    if (n == 4) {
        const unsigned *cp = (const unsigned *)(colour + 3 * (size_t)p0);
        c0 = cp[0]; c1 = cp[1]; c2 = cp[2];
        if (occluder) o4 = *(const unsigned *)(occluder + p0);
    } else if (n > 0) {
        unsigned w[3] = {0u, 0u, 0u};
        for (int i = 0; i < 3 * n; ++i) w[i >> 2] |= (unsigned)colour[3 * (size_t)p0 + i] << (8 * (i & 3));
        c0 = w[0]; c1 = w[1]; c2 = w[2];
        if (occluder) { o4 = 0u; for (int k = 0; k < n; ++k) o4 |= (unsigned)occluder[p0 + k] << (8 * k); }
    }
}

// bit k of the result: pixel p0 + k exists and a primitive of the ropes [rope_lo, rope_hi) covers it; col[k]: the colour word of the one drawn last
TDLO_PX unsigned render_search4(const RenderSpan &sp, const int *heads, int rope_lo, int rope_hi, const int *prims, int p0, int n, int cols, int lane,
                                unsigned col[4]) {
    unsigned done = n >= 4 ? 0u : (n > 0 ? (0xfu << n) & 0xfu : 0xfu);        // bit k: pixel k has its colour (or does not exist)
    col[0] = 0u; col[1] = 0u; col[2] = 0u; col[3] = 0u;
    int pr[4] = {0, 0, 0, 0}, pc[4] = {0, 0, 0, 0};
    bool have_px = false, finished = false;
    for (int rbase = rope_hi - 1; rbase >= rope_lo && !finished; rbase -= 64) {
        unsigned long long ropes = render_vote(lane, [&](int l) {
            const int j = rbase - l;
            if (j < rope_lo) return false;
            const RenderI4 h = *(const RenderI4 *)(heads + 8 * (size_t)j);  // {c_lo, r_lo, c_hi, r_hi}
            return h.w >= sp.r_lo && h.y <= sp.r_hi && h.z >= sp.c_lo && h.x <= sp.c_hi;
        });
        while (ropes && !finished) {                                          // lowest bit = highest position = drawn last
            const int rb = __builtin_ctzll(ropes);
            ropes &= ropes - 1ull;
            const int *head = heads + 8 * (size_t)render_uniform(rbase - rb);
            const int first = head[4], last = first + head[5] - 1;
            for (int base = last; base >= first; base -= 64) {
                unsigned long long live = render_vote(lane, [&](int l) {
                    const int j = base - l;
                    if (j < first) return false;
                    const RenderI4 ra = *(const RenderI4 *)(prims + 8 * (size_t)j);
                    const RenderI2 rc = *(const RenderI2 *)(prims + 8 * (size_t)j + 4);
                    const int ext = ra.x ? rc.y : (rc.y + 1) >> 1;           // disc: its radius; line: half its width, rounded up
                    const int x0 = min(ra.y, ra.w) - ext, x1 = max(ra.y, ra.w) + ext, y0 = min(ra.z, rc.x) - ext, y1 = max(ra.z, rc.x) + ext;
                    return y1 >= sp.r_lo && y0 <= sp.r_hi && x1 >= sp.c_lo && x0 <= sp.c_hi;
                });
                if (live == 0ull) continue;
                if (!have_px) {                                               // row and column of the lane's pixels: one division, only in waves that draw
                    have_px = true;
                    int r = max(p0, 0) / cols, c = max(p0, 0) - r * cols;
#pragma unroll
                    for (int k = 0; k < 4; ++k) { pr[k] = r; pc[k] = c; if (++c == cols) { c = 0; ++r; } }
                }
                while (live) {
                    const int b = __builtin_ctzll(live);
                    live &= live - 1ull;
                    const int *rec = prims + 8 * (size_t)render_uniform(base - b);
                    const int kind = rec[0], a0 = rec[1], b0 = rec[2], a1 = rec[3], b1 = rec[4], size = rec[5];
                    const unsigned cw = (unsigned)rec[6];
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (!((done >> k) & 1u) && covers(kind, a0, b0, a1, b1, size, pc[k], pr[k])) { col[k] = cw; done |= 1u << k; }
                }
                if (render_all_done(done)) { finished = true; break; }
            }
        }
    }
    return n >= 4 ? done : (n > 0 ? done & ~(0xfu << n) : 0u);
}

// blend (every byte), then the colours found; the lane's 12 bytes out
TDLO_PX void render_store4(unsigned char *out, int p0, int n, unsigned c0, unsigned c1, unsigned c2, unsigned o4, unsigned hit, const unsigned col[4]) {
    const unsigned q0 = o4 & 255u, q1 = (o4 >> 8) & 255u, q2 = (o4 >> 16) & 255u, q3 = o4 >> 24;      // the occluder byte of a pixel, on its three colour bytes
    unsigned w0 = blend4(c0, q0 * 0x010101u | (q1 << 24));
    unsigned w1 = blend4(c1, q1 * 0x0101u | (q2 * 0x01010000u));
    unsigned w2 = blend4(c2, q2 | (q3 * 0x01010100u));
    if (hit & 1u) w0 = (w0 & 0xff000000u) | col[0];
    if (hit & 2u) { w0 = (w0 & 0x00ffffffu) | (col[1] << 24); w1 = (w1 & 0xffff0000u) | (col[1] >> 8); }
    if (hit & 4u) { w1 = (w1 & 0x0000ffffu) | (col[2] << 16); w2 = (w2 & 0xffffff00u) | (col[2] >> 16); }
    if (hit & 8u) w2 = (w2 & 0x000000ffu) | (col[3] << 8);
    if (n == 4) {
        unsigned *op = (unsigned *)(out + 3 * (size_t)p0);
        op[0] = w0; op[1] = w1; op[2] = w2;
    } else if (n > 0) {
        const unsigned w[3] = {w0, w1, w2};
        for (int i = 0; i < 3 * n; ++i) out[3 * (size_t)p0 + i] = (unsigned char)(w[i >> 2] >> (8 * (i & 3)));
    }
}

}  // namespace tdlo
