// tdlo_cell_painter.hip -- the painter test over a cell of ropes for whole batches of cells (include/trackdlo_hip.h has the statement; tdlo_cell_painter_lane.h
// the arithmetic, shared with the host).  Every node of a cell meets every edge of the cell, per camera: a (camera, cell) job is spread over node tiles, grid
// (node blocks of 256 of the largest cell, largest K, cells), lane = flat node.  A workgroup takes its cell's record out of a table in device memory; one
// beyond its cell's node count or its cell's K leaves at once; no workgroup waits for another.  Two launches:
//   k_cell_project  camera-frame node, pixel, flags and the key of the edge that starts at the node into the (camera, cell) table of 16-byte records in device
//                   memory; a wave's 64 consecutive nodes give two seen words by one ballot, stored by lane 0
//   k_cell_cover    the lane keeps its node's pixel and its threshold pair (key, flat index of its first painted incident edge) in registers and streams the
//                   cell's table through LDS in tiles of 512 edges (513 records, 8 KB: the last edge's far end).  Every lane reads the same record: an LDS
//                   broadcast.  Per edge: painted, before my threshold, the box reject, within_half_width.  A wave whose drawable nodes are all decided
//                   skips the tiles that follow (a ballot); it keeps staging them, and the workgroup leaves the loop when no wave has an undecided node.
//                   A wave's hidden bits are two words from one ballot, stored by lane 0
// The words go to pinned host memory with ordinary vector stores; the host forms the union over the cameras, the thresholds and the ropes' sets.
// Built with -ffp-contract=off: the bits of steps 1 - 2 and of the keys are the host's.
#include <hip/hip_runtime.h>
#include "tdlo_internal.h"
#include "tdlo_cell_painter_lane.h"

namespace tdlo {

static_assert(sizeof(CellRec) == 16, "a record is one 16-byte load");

__global__ __launch_bounds__(kCellBlock) void k_cell_project(const CellJob *__restrict__ tab, int rows, int cols) {
    const CellJob j = tab[blockIdx.z];
    const int k = (int)blockIdx.y, N = j.N, n0 = (int)blockIdx.x * kCellBlock + ((int)threadIdx.x & ~63);
    if (k >= j.K || (int)blockIdx.x * kCellBlock >= N) return;
    if (n0 >= N) return;                                              // (wave-uniform: a whole wave beyond the cell)
    const int lane = (int)threadIdx.x & 63, n = n0 + lane, W = (N + 31) / 32;
    unsigned fl = 0u;
    if (n < N) {
        const PainterCam cam = j.cams[k];
        const CellRec r = cell_project(cam, j.X, j.X + N, j.X + 2 * (size_t)N, n, cell_link(j.link, n), rows, cols);
        j.recs[(size_t)k * N + n] = r;
        fl = r.flag;
    }
    const unsigned long long s = __ballot((fl & kPainterSeen) != 0u);
    if (lane == 0) {
        unsigned *seen = j.seen + (size_t)k * W;
        const int q = n0 >> 5;
        seen[q] = (unsigned)s;
        if (q + 1 < W) seen[q + 1] = (unsigned)(s >> 32);
    }
}

__global__ __launch_bounds__(kCellBlock) void k_cell_cover(const CellJob *__restrict__ tab) {
    const CellJob j = tab[blockIdx.z];
    const int k = (int)blockIdx.y, N = j.N, b0 = (int)blockIdx.x * kCellBlock;
    if (k >= j.K || b0 >= N) return;
    __shared__ CellRec tile[kCellTile + 1];
    const int tid = (int)threadIdx.x, lane = tid & 63, n0 = b0 + (tid & ~63), n = n0 + lane, W = (N + 31) / 32;
    const CellRec *T = j.recs + (size_t)k * N;
    CellFirst first{0.0, 0, 0};
    int pc = 0, pr = 0;
    bool undecided = false, hidden = false;
    if (n < N) {
        const CellRec own = T[n];
        undecided = (own.flag & kPainterDrawable) != 0u;
        first = cell_first(T, n);
        pc = cell_px_c(own.px); pr = cell_px_r(own.px);
    }
    for (int e0 = 0; e0 < N; e0 += kCellTile) {
        const int cnt = N - e0 < kCellTile ? N - e0 : kCellTile, have = cnt + (e0 + cnt < N ? 1 : 0);
        for (int i = tid; i < have; i += kCellBlock) tile[i] = T[e0 + i];
        __syncthreads();
        if (__ballot(undecided) && undecided && cell_tile_hides(tile, e0, cnt, first, pc, pr, j.width)) { hidden = true; undecided = false; }
        if (!__syncthreads_or(undecided ? 1 : 0)) break;             // (also the barrier in front of the next tile's stores)
    }
    if (n0 < N) {                                                     // (wave-uniform)
        const unsigned long long h = __ballot(hidden);
        if (lane == 0) {
            unsigned *out = j.hidden + (size_t)k * W;
            const int q = n0 >> 5;
            out[q] = (unsigned)h;
            if (q + 1 < W) out[q + 1] = (unsigned)(h >> 32);
        }
    }
}

hipError_t launch_cell_painter(const CellJob *tab_dev, int C, int Kmax, int Nmax, int rows, int cols, hipStream_t s) {
    if (C < 1 || C > kCellPainterMaxCells || Kmax < 1 || Kmax > kPainterMaxCams || Nmax < 1 || Nmax > kCellPainterMaxNodes) return hipErrorInvalidValue;
    const dim3 grid((Nmax + kCellBlock - 1) / kCellBlock, Kmax, C);
    hipLaunchKernelGGL(k_cell_project, grid, dim3(kCellBlock), 0, s, tab_dev, rows, cols);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cell_cover, grid, dim3(kCellBlock), 0, s, tab_dev);
    return hipGetLastError();
}

}  // namespace tdlo
