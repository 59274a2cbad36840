// tdlo_render_batch.hip -- the tracking-result image (trackdlo_node.cpp:377-452) for K images of one size with any number of ropes each, in ONE launch:
//   per image: blend ONCE (0.5 a + 0.5 (a & o), round half to even), then the image's ropes in the caller's list order, each exactly as k_render
//   (tdlo_render.hip) draws its one rope -- edges farthest first: line, disc, disc; a later primitive, and a later rope, overwrites an earlier one.
// A picture of several ropes over one camera image cannot be made from k_render calls: each blends the whole image before it paints.
//
// Grid (tiles of 1024 pixels, images); workgroup and lane layout are k_render's: 256 threads, thread = 4 consecutive flat pixels, wave = 256 pixels.  A wave
// belongs to one image (blockIdx.y): its record of the descriptor table -- colour, occluder and out pointers, its range of rope heads, which pair of corner
// words it owns -- is read through a wave-uniform address.  No workgroup waits for another.  The two-level search (rope heads, then the primitives of a
// surviving rope, both from the end, in rounds of 64, 64-bit ballots walked bit by bit, records through scalar loads), the loads, the blend and the stores
// are tdlo_render_search.h, which also compiles for the host; blend4 and covers are tdlo_render_px.h, shared with k_render.  A wave that meets no rope
// only blends.  The image's last 1 .. 3 pixels go byte by byte; nothing beyond an image is read or written.
// PARITY UNPINNED against OpenCV's rasterisers, exactly as for k_render; tests/render_batch_ref.py is the numpy statement.
// The occlusion corners ride along as in k_render: one atomicMin and one atomicMax per wave that saw a zero occluder byte, on the image's own pair of words.
#include "tdlo_internal.h"
#include "tdlo_render_search.h"

namespace tdlo {
namespace {

constexpr int kRB = 256;                 // threads per workgroup: 4 waves, 1024 pixels

__global__ __launch_bounds__(kRB) void k_render_batch(const RenderBatchImage *__restrict__ images, const int *__restrict__ heads,
                                                      const int *__restrict__ prims, int P, int cols, unsigned *__restrict__ corners) {
    const int lane = threadIdx.x & 63;
    const int wave_first = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * kRB + (threadIdx.x & ~63u)) * 4u));
    if (wave_first >= P) return;                                              // (the whole wave)
    const RenderBatchImage im = images[blockIdx.y];                           // wave-uniform: scalar loads
    const int p0 = wave_first + 4 * lane;
    const int n = min(4, P - p0);                                             // pixels of this lane; <= 0: a lane behind the image (it still votes)
    unsigned c0, c1, c2, o4;
    render_load4(im.colour, im.occluder, p0, n, c0, c1, c2, o4);

    unsigned col[4] = {0u, 0u, 0u, 0u};
    unsigned hit = 0u;
    if (im.rope_hi > im.rope_lo) hit = render_search4(render_span(wave_first, P, cols), heads, im.rope_lo, im.rope_hi, prims, p0, n, cols, lane, col);
    render_store4(im.out, p0, n, c0, c1, c2, o4, hit, col);

    // ---- occlusion corners: pixel indices ascend with the lane, so the wave's first / last zero byte is that of the first / last lane that has one
    if (im.corner >= 0 && im.occluder) {
        unsigned z = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) if (k < n && ((o4 >> (8 * k)) & 255u) == 0u) z |= 1u << k;
        const unsigned long long any = __ballot(z != 0u);
        if (any) {
            const int first = p0 + (z ? __builtin_ctz(z) : 0), last = p0 + (z ? 31 - __builtin_clz(z) : 0);
            const int lo = __shfl(first, __builtin_ctzll(any)), hi = __shfl(last, 63 - __builtin_clzll(any));
            unsigned *corner = corners + 2 * (size_t)im.corner;
            if (lane == 0) { atomicMin(corner, (unsigned)lo); atomicMax((int *)corner + 1, hi); }
        }
    }
}

}  // namespace

// images: K records in device memory (their pointers readable / writable by the device, 4-byte aligned); heads / prims: the table of
// tdlo_render_batch_table in device memory, 16-byte aligned; corners: pairs of device words the caller has set to {0xffffffff, -1} on the stream
hipError_t launch_render_batch(const RenderBatchImage *images, int K, const int *heads, const int *prims, int P, int cols, unsigned *corners, hipStream_t s) {
    hipLaunchKernelGGL(k_render_batch, dim3((P + 4 * kRB - 1) / (4 * kRB), K), dim3(kRB), 0, s, images, heads, prims, P, cols, corners);
    return hipGetLastError();
}

}  // namespace tdlo
