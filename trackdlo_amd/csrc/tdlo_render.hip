// tdlo_render.hip -- the tracking-result image the ROS node publishes every frame (trackdlo_node.cpp:377-452) in ONE launch:
//   tracking_img = 0.5 * cur_image_orig + 0.5 * cur_image   (cv::addWeighted on 8-bit images: round half to even; cur_image = orig & occlusion mask)
//   per edge, farthest from the camera first: cv::line of 5 pixels, cv::circle of radius 7 at both end nodes -- a later primitive overwrites an earlier
// The primitives arrive as a table the host formed (tdlo_host.cpp, render_primitives: 3 (M - 1) records of eight ints, in drawing order).  The painter's
// order is turned round here: a pixel takes the colour of the LAST primitive that covers it, so every pixel searches the table from its end and stops
// at the first hit -- no pixel is written twice, no ordering between workgroups.
//
// thread = 4 consecutive pixels of the flat image, as k_colour_mask (12 colour bytes + 4 occluder bytes in, 12 bytes out, as dwords); wave = 256 flat
// pixels, i.e. a span of rows [r_lo, r_hi] (and of columns when it lies within one row).  Culling is per WAVE: in rounds of 64 primitives, from the end
// of the table, lane l tests the bounding box of primitive (base - l) against the wave's span; the ballot of the survivors stays in an SGPR pair and is
// walked bit by bit, the record read through a wave-uniform address (scalar loads).  Rounds of 64 until the table is exhausted or every pixel of the
// wave has its colour: no list, hence no capacity.  A wave that meets no primitive (nearly all of them) only blends.
// "Under a line" is within_half_width (tdlo_thick_line.h), the one statement the host's self-occlusion test uses as well; "under a disc" is
// dx^2 + dy^2 <= radius^2.  PARITY UNPINNED against OpenCV's rasterisers (not part of the build image); tests/render_ref.py is the numpy statement.
// The occlusion corners (:198-208: first and last pixel in row-major order whose occluder byte is 0) ride along: one atomicMin and one atomicMax per
// wave that saw such a byte.
#include "tdlo_internal.h"
#include "tdlo_render_px.h"

namespace tdlo {
namespace {

constexpr int kRB = 256;                 // threads per workgroup: 4 waves, 1024 pixels

// (blend4 and covers: tdlo_render_px.h, shared with k_render_batch)

__global__ __launch_bounds__(kRB) void k_render(const unsigned char *__restrict__ colour, const unsigned char *__restrict__ occluder,
                                                unsigned char *__restrict__ out, const int *__restrict__ prims, int n_prims, int P, int cols,
                                                unsigned *__restrict__ corner) {
    const int lane = threadIdx.x & 63;
    const int wave_first = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * kRB + (threadIdx.x & ~63u)) * 4u));
    if (wave_first >= P) return;                                              // (the whole wave)
    const int p0 = wave_first + 4 * lane;
    const int n = min(4, P - p0);                                             // pixels of this lane; <= 0: a lane behind the image (it still votes)
    unsigned c0 = 0u, c1 = 0u, c2 = 0u, o4 = 0xffffffffu;
    if (n == 4) {
        const unsigned *cp = (const unsigned *)(colour + 3 * (size_t)p0);
        c0 = cp[0]; c1 = cp[1]; c2 = cp[2];
        if (occluder) o4 = *(const unsigned *)(occluder + p0);
    } else if (n > 0) {                                                       // the image's last 1 .. 3 pixels: byte by byte, nothing beyond the image is touched
        unsigned w[3] = {0u, 0u, 0u};
        for (int i = 0; i < 3 * n; ++i) w[i >> 2] |= (unsigned)colour[3 * (size_t)p0 + i] << (8 * (i & 3));
        c0 = w[0]; c1 = w[1]; c2 = w[2];
        if (occluder) { o4 = 0u; for (int k = 0; k < n; ++k) o4 |= (unsigned)occluder[p0 + k] << (8 * k); }
    }

    // ---- which primitives does this wave meet?  Its pixels span rows [r_lo, r_hi]; within one row, columns [c_lo, c_hi]
    const int wave_last = min(wave_first + 4 * 64 - 1, P - 1);
    const int r_lo = wave_first / cols, r_hi = wave_last / cols;
    const int c_lo = r_lo == r_hi ? wave_first - r_lo * cols : 0, c_hi = r_lo == r_hi ? wave_last - r_hi * cols : cols - 1;
    unsigned done = n >= 4 ? 0u : (n > 0 ? (0xfu << n) & 0xfu : 0xfu);        // bit k: pixel k has its colour (or does not exist)
    unsigned col[4] = {0u, 0u, 0u, 0u};
    int pr[4], pc[4];
    bool have_px = false;
    for (int base = n_prims - 1; base >= 0; base -= 64) {
        const int j = base - lane;
        bool meets = false;
        if (j >= 0) {
            const int4 ra = *(const int4 *)(prims + 8 * (size_t)j);
            const int2 rb = *(const int2 *)(prims + 8 * (size_t)j + 4);
            const int ext = ra.x ? rb.y : (rb.y + 1) >> 1;                   // disc: its radius; line: half its width, rounded up
            const int x0 = min(ra.y, ra.w) - ext, x1 = max(ra.y, ra.w) + ext, y0 = min(ra.z, rb.x) - ext, y1 = max(ra.z, rb.x) + ext;
            meets = y1 >= r_lo && y0 <= r_hi && x1 >= c_lo && x0 <= c_hi;
        }
        unsigned long long live = __ballot(meets);
        if (live == 0ull) continue;
        if (!have_px) {                                                       // row and column of the lane's pixels: one division, only in waves that draw
            have_px = true;
            int r = max(p0, 0) / cols, c = max(p0, 0) - r * cols;
#pragma unroll
            for (int k = 0; k < 4; ++k) { pr[k] = r; pc[k] = c; if (++c == cols) { c = 0; ++r; } }
        }
        while (live) {                                                        // lowest bit = highest index = drawn last: the first hit is the pixel's colour
            const int b = __builtin_ctzll(live);
            live &= live - 1ull;
            const int *rec = prims + 8 * (size_t)__builtin_amdgcn_readfirstlane(base - b);      // wave-uniform: scalar loads
            const int kind = rec[0], a0 = rec[1], b0 = rec[2], a1 = rec[3], b1 = rec[4], size = rec[5];
            const unsigned cw = (unsigned)rec[6];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (!((done >> k) & 1u) && covers(kind, a0, b0, a1, b1, size, pc[k], pr[k])) { col[k] = cw; done |= 1u << k; }
        }
        if (__ballot(done != 0xfu) == 0ull) break;                            // every pixel of the wave has its colour
    }

    // ---- blend (every byte), then the colours found
    unsigned w0, w1, w2;
    {
        const unsigned q0 = o4 & 255u, q1 = (o4 >> 8) & 255u, q2 = (o4 >> 16) & 255u, q3 = o4 >> 24;      // the occluder byte of a pixel, on its three colour bytes
        w0 = blend4(c0, q0 * 0x010101u | (q1 << 24));
        w1 = blend4(c1, q1 * 0x0101u | (q2 * 0x01010000u));
        w2 = blend4(c2, q2 | (q3 * 0x01010100u));
    }
    const unsigned hit = n >= 4 ? done : (n > 0 ? done & ~(0xfu << n) : 0u);  // pixels that exist and were covered (col is 0 for the others anyway)
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

    // ---- occlusion corners: pixel indices ascend with the lane, so the wave's first / last zero byte is that of the first / last lane that has one
    if (corner) {                                                             // (given only with an occluder)
        unsigned z = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) if (k < n && ((o4 >> (8 * k)) & 255u) == 0u) z |= 1u << k;
        const unsigned long long any = __ballot(z != 0u);
        if (any) {
            const int first = p0 + (z ? __builtin_ctz(z) : 0), last = p0 + (z ? 31 - __builtin_clz(z) : 0);
            const int lo = __shfl(first, __builtin_ctzll(any)), hi = __shfl(last, 63 - __builtin_clzll(any));
            if (lane == 0) { atomicMin(corner, (unsigned)lo); atomicMax((int *)corner + 1, hi); }
        }
    }
}

}  // namespace

// colour / occluder: readable by the device (device memory or the context's pinned buffers), 4-byte aligned; out likewise, 3 P bytes; prims: device
// memory, n_prims records; corner: two device words the caller has set to {0xffffffff, -1} on the stream (only touched when occluder != nullptr)
hipError_t launch_render(const unsigned char *colour, const unsigned char *occluder, unsigned char *out, const int *prims, int n_prims, int P, int cols,
                         unsigned *corner, hipStream_t s) {
    hipLaunchKernelGGL(k_render, dim3((P + 4 * kRB - 1) / (4 * kRB)), dim3(kRB), 0, s, colour, occluder, out, prims, n_prims, P, cols, corner);
    return hipGetLastError();
}

}  // namespace tdlo
