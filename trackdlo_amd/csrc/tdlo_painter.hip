// tdlo_painter.hip -- the self-occlusion test under a rig for whole batches (include/trackdlo_hip.h has the statement; tdlo_painter_lane.h the arithmetic, shared
// with the host).  k_rig_painter_batch: grid (largest K_f, F); a workgroup is ONE (camera, frame) job and takes its frame's record out of a table in device
// memory; a workgroup with blockIdx.x >= K_f leaves at once; no workgroup waits for another (the shape of k_cloud_rig_batch and k_node_min_dist_batch).
//
// A job, M <= 1024 nodes, 256 threads = 4 waves:
//   A  thread = node / edge (striding by 256): camera-frame node, pixel, flags, the key of edge m into LDS; a wave's 64 consecutive nodes give two seen words by
//      one ballot, stored by lane 0
//   B  thread = edge: its rank by counting the painted j with (key_j, j) < (key_i, i) -- every lane reads the same key_j (an LDS broadcast, no bank conflict);
//      its own key_i is one ds_read_b64 per lane at consecutive 8-byte addresses: 32 lanes x 2 dwords cover the 64 banks once.  No sort network, no divergence on ties
//   C  wave = one word of 32 nodes, node after node; the lanes stride over the ranks below `first`, a ballot finishes a node (a node with many edges in front of
//      it does not serialise one lane); lane 0 stores the hidden word
// LDS: keys 8 KB + pixels 8 KB + ranks 4 KB + order 4 KB + flags 1 KB = 25 KB a workgroup: six workgroups fit a CU's 160 KB, and a call has K F <= a few hundred
// workgroups over 256 CUs, so occupancy is not what limits it.
// The words go to pinned host memory with ordinary vector stores; the host forms the union over the cameras, the threshold and the gap fill.
// Built with -ffp-contract=off: the bits of steps 1 - 3 are the host's.
#include <hip/hip_runtime.h>
#include "tdlo_internal.h"
#include "tdlo_painter_lane.h"

namespace tdlo {

constexpr int kPainterBlock = 256;

__global__ __launch_bounds__(kPainterBlock) void k_rig_painter_batch(const PainterFrame *__restrict__ tab, int rows, int cols) {
    const PainterFrame f = tab[blockIdx.y];
    const int k = (int)blockIdx.x, M = f.M;
    if (k >= f.K || M < 1 || M > kPainterMaxNodes) return;
    __shared__ double key[kPainterMaxNodes];
    __shared__ int pc[kPainterMaxNodes], pr[kPainterMaxNodes], rank[kPainterMaxNodes], order[kPainterMaxNodes];
    __shared__ unsigned char flag[kPainterMaxNodes];
    __shared__ int nP_s;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, nE = M - 1, W = (M + 31) / 32;
    const PainterCam cam = f.cams[k];
    unsigned *seen = f.seen + (size_t)k * W, *hidden = f.hidden + (size_t)k * W;
    if (tid == 0) nP_s = 0;
    // A
    for (int m0 = wave * 64; m0 < M; m0 += kPainterBlock) {          // (wave-uniform bound: every lane reaches the ballot)
        const int m = m0 + lane;
        unsigned fl = 0u;
        if (m < M) {
            double ky; bool p; int c, r;
            painter_node_edge(cam, f.Y, M, m, rows, cols, c, r, fl, ky, p);
            pc[m] = c; pr[m] = r; key[m] = ky;
            fl |= p ? kPainterPainted : 0u;
            flag[m] = (unsigned char)fl;
        }
        const unsigned long long s = __ballot((fl & kPainterSeen) != 0u);
        if (lane == 0) {
            const int q = m0 >> 5;
            seen[q] = (unsigned)s;
            if (q + 1 < W) seen[q + 1] = (unsigned)(s >> 32);
        }
    }
    __syncthreads();
    // B
    for (int i0 = wave * 64; i0 < nE; i0 += kPainterBlock) {
        const int i = i0 + lane;
        const bool p = i < nE && (flag[i] & kPainterPainted);
        if (i < nE) {
            const int r = p ? painter_rank(key, flag, nE, i) : -1;
            rank[i] = r;
            if (p) order[r] = i;
        }
        const unsigned long long b = __ballot(p);
        if (lane == 0 && b) atomicAdd(&nP_s, __popcll(b));
    }
    __syncthreads();
    // C
    const int nP = nP_s;
    for (int q = wave; q < W; q += kPainterBlock / 64) {
        unsigned word = 0u;
        for (int b = 0; b < 32 && 32 * q + b < M; ++b) {
            const int m = 32 * q + b;
            if (!(flag[m] & kPainterDrawable)) continue;
            const int first = painter_first(rank, M, m, nP);
            for (int r0 = 0; r0 < first; r0 += 64) {
                const int r = r0 + lane;
                const bool hit = r < first && painter_covers(order, pc, pr, r, m, f.width);
                if (__ballot(hit)) { word |= 1u << b; break; }
            }
        }
        if (lane == 0) hidden[q] = word;
    }
}

hipError_t launch_rig_painter_batch(const PainterFrame *tab_dev, int F, int Kmax, int rows, int cols, hipStream_t s) {
    if (F < 1 || F > 65535 || Kmax < 1 || Kmax > kPainterMaxCams) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rig_painter_batch, dim3(Kmax, F), dim3(kPainterBlock), 0, s, tab_dev, rows, cols);
    return hipGetLastError();
}

}  // namespace tdlo
