// tdlo_cluster.hip -- one resident cloud clustered into ropes (tdlo_cloud_cluster and the tracker call built on it; include/trackdlo_hip.h has the statement,
// tdlo_cluster_lane.h the lane and why the result does not depend on the schedule).
//
// Workspace: parent [n] | size [n] | rank [n] | kcnt [chunks], chunks = ceil(n / kBlock).  Six short launches in front of k_assign_scatter (tdlo_assign.hip,
// unchanged: the stable scatter, the counts to pinned memory and the word the host waits on):
//   k_cluster_init     parent[i] = i, size[i] = 0
//   k_cluster_link     grid (chunks of 256 points, tiles of kClusterTile points): lane = point i against ONE tile staged in LDS; only the tiles at or below the
//                      workgroup's own do anything (a workgroup's 256 points lie in one tile), so a pair is tested once, by the later point's lane.  A
//                      workgroup per (chunk, tile) and not a loop over the tiles: the last chunk's lanes would walk the whole cloud one after the other
//                      (measured: 2.3 ms at 10 000 points, all of it that walk).  In the tile the lane of tdlo_cluster_lane.h: every point j < i within the
//                      gate is joined to i's tree by a compare-and-swap on parent[larger root].  Nobody waits for anybody: no grid barrier, no spinning on
//                      another workgroup, no residency assumption, any order of the workgroups.  A join that runs out of attempts raises the give-up word in
//                      pinned host memory; the driver then serves the call on the host
//   k_cluster_flatten  parent[i] = find(i); one atomic add on size[root] per finite point
//   k_cluster_count    kcnt[b] = the kept roots (parent[i] == i, size[i] >= min_size) among workgroup b's points
//   k_cluster_rank     rank[r] of a kept root = the kept roots in front of it: every workgroup sums the counts in front of it itself, as k_assign_scatter forms
//                      its offsets, then ballot + popcount; workgroup 0 writes C, the sum of all counts, to pinned host memory
//   k_cluster_owner    owner[i] from root, size and rank, and counts[b F + f] in exactly the layout and geometry (assign_geometry) k_assign_count writes
// Every launch needs ALL of the one before it (the sizes all points, the ranks all counts, the owners all ranks), so none of them can ride in its neighbour.
#include "tdlo_devcommon.h"
#include "tdlo_cluster_lane.h"

namespace tdlo {

static_assert(kClusterTile % kBlock == 0, "a workgroup's points lie in one tile");

__global__ __launch_bounds__(kBlock) void k_cluster_init(int n, int *__restrict__ parent, int *__restrict__ size) {
    const int i = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    if (i < n) { parent[i] = i; size[i] = 0; }
}

__global__ __launch_bounds__(kBlock) void k_cluster_link(const double *__restrict__ X, int n, double tol2, int *parent, unsigned long long *giveup_host) {
    __shared__ double L[3 * kClusterTile];                       // the tile: x | y | z, kClusterTile each
    const int t = threadIdx.x, i0 = (int)blockIdx.x * kBlock, i = i0 + t;
    double x = 0, y = 0, z = 0;
    if (i < n) { x = X[i]; y = X[(size_t)n + i]; z = X[2 * (size_t)n + i]; }
    const bool live = i < n && cluster_finite(x, y, z);
    const int tl = (int)blockIdx.y, own = i0 / kClusterTile, end = i0 + kBlock < n ? i0 + kBlock : n;      // (no lane of this workgroup looks at a point from `end` on)
    if (tl > own) return;                                          // a tile behind the workgroup's own: its pairs belong to the lanes over there
    const int t0 = tl * kClusterTile, cnt = end - t0 < kClusterTile ? end - t0 : kClusterTile;
    for (int k = t; k < cnt; k += kBlock) { L[k] = X[t0 + k]; L[kClusterTile + k] = X[(size_t)n + t0 + k]; L[2 * kClusterTile + k] = X[2 * (size_t)n + t0 + k]; }
    __syncthreads();
    int r = i;
    if (live && !cluster_tile(L, L + kClusterTile, L + 2 * kClusterTile, t0, cnt, i, x, y, z, tol2, parent, r))
        __hip_atomic_store(giveup_host, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(kBlock) void k_cluster_flatten(const double *__restrict__ X, int n, int *parent, int *size) {
    const int i = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    if (i >= n) return;
    if (!cluster_finite(X[i], X[(size_t)n + i], X[2 * (size_t)n + i])) return;      // (its own root, member of nothing)
    const int r = cluster_find(parent, i);
    cluster_lower(parent + i, r);
    (void)__hip_atomic_fetch_add(size + r, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kBlock) void k_cluster_count(int n, const int *__restrict__ parent, const int *__restrict__ size, int min_size, int *__restrict__ kcnt) {
    __shared__ int swc[kBlock / kWave];
    const int t = threadIdx.x, i = (int)blockIdx.x * kBlock + t;
    const bool kept = i < n && parent[i] == i && cluster_kept(size[i], min_size);
    const unsigned long long mk = __ballot(kept);
    if ((t & 63) == 0) swc[t >> 6] = (int)__popcll(mk);
    __syncthreads();
    if (t == 0) kcnt[blockIdx.x] = swc[0] + swc[1] + swc[2] + swc[3];
}

__global__ __launch_bounds__(kBlock) void k_cluster_rank(int n, const int *__restrict__ parent, const int *__restrict__ size, int min_size, const int *__restrict__ kcnt,
                                                        int *__restrict__ rank, unsigned long long *n_clusters_host) {
    __shared__ int sfront, stot, swc[kBlock / kWave];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, b = (int)blockIdx.x, nb = (int)gridDim.x, i = b * kBlock + t;
    if (t == 0) { sfront = 0; stot = 0; }
    __syncthreads();
    int front = 0, tot = 0;
    for (int k = t; k < nb; k += kBlock) { const int v = kcnt[k]; tot += v; if (k < b) front += v; }
    if (tot) atomicAdd(&stot, tot);
    if (front) atomicAdd(&sfront, front);
    const bool kept = i < n && parent[i] == i && cluster_kept(size[i], min_size);
    const unsigned long long mk = __ballot(kept);
    if (lane == 0) swc[w] = (int)__popcll(mk);
    __syncthreads();
    if (kept) {
        int rk = sfront + (int)__popcll(mk & ((1ull << lane) - 1ull));
        for (int v = 0; v < w; ++v) rk += swc[v];
        rank[i] = rk;
    }
    if (b == 0 && t == 0) __hip_atomic_store(n_clusters_host, (unsigned long long)(unsigned)stot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(kBlock) void k_cluster_owner(int n, const int *__restrict__ parent, const int *__restrict__ size, const int *__restrict__ rank, int min_size,
                                                         int F, int cpb, int *__restrict__ owner, int *__restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *scnt = (int *)smem;
    const int t = threadIdx.x, lane = t & 63;
    for (int k = t; k < F; k += kBlock) scnt[k] = 0;
    __syncthreads();
    const int chunks = (n + kBlock - 1) / kBlock, c0 = (int)blockIdx.x * cpb, c1 = c0 + cpb < chunks ? c0 + cpb : chunks;
    for (int ch = c0; ch < c1; ++ch) {
        const int i = ch * kBlock + t;
        int o = -1;
        if (i < n) {
            const int r = parent[i], sz = size[r];
            o = cluster_owner(sz, cluster_kept(sz, min_size) ? rank[r] : 0, min_size, F);
            owner[i] = o;
        }
        unsigned long long rem = __ballot(o >= 0);
        while (rem) {                                              // one ballot per cluster present in the wave, as k_assign_count counts its ropes
            const int src = __ffsll((long long)rem) - 1, fr = __shfl(o, src);
            const unsigned long long mk = __ballot(o == fr);
            if (lane == src) atomicAdd(&scnt[fr], (int)__popcll(mk));
            rem &= ~mk;
        }
    }
    __syncthreads();
    for (int k = t; k < F; k += kBlock) counts[(size_t)blockIdx.x * F + k] = scnt[k];
}

hipError_t launch_cluster(const double *X, int n, double tol2, int min_size, int F, int *parent, int *size, int *rank, int *kcnt, int *owner, int *counts,
                          unsigned long long *giveup_host, unsigned long long *n_clusters_host, hipStream_t s) {
    int nwg, cpb;
    assign_geometry(n, &nwg, &cpb);
    const int chunks = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_cluster_init, dim3(chunks), dim3(kBlock), 0, s, n, parent, size);
    hipLaunchKernelGGL(k_cluster_link, dim3(chunks, (n + kClusterTile - 1) / kClusterTile), dim3(kBlock), 0, s, X, n, tol2, parent, giveup_host);
    hipLaunchKernelGGL(k_cluster_flatten, dim3(chunks), dim3(kBlock), 0, s, X, n, parent, size);
    hipLaunchKernelGGL(k_cluster_count, dim3(chunks), dim3(kBlock), 0, s, n, (const int *)parent, (const int *)size, min_size, kcnt);
    hipLaunchKernelGGL(k_cluster_rank, dim3(chunks), dim3(kBlock), 0, s, n, (const int *)parent, (const int *)size, min_size, (const int *)kcnt, rank, n_clusters_host);
    hipLaunchKernelGGL(k_cluster_owner, dim3(nwg), dim3(kBlock), sizeof(int) * (size_t)((F + 3) & ~3), s, n, (const int *)parent, (const int *)size, (const int *)rank,
                       min_size, F, cpb, owner, counts);
    return hipGetLastError();
}

}  // namespace tdlo
