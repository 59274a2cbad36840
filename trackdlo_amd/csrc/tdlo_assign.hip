// tdlo_assign.hip -- one resident cloud dealt out among F slots (tdlo_cloud_assign and the calls built on it; include/trackdlo_hip.h has the statement).
//
// The point workgroups own SPANS: the cloud is cut into chunks of kBlock points, workgroup b owns the cpb consecutive chunks from b cpb on, at most kAssignMaxWgs
// workgroups in all (assign_geometry) -- so the count table stays short however large the cloud is.  Both kernels use the same geometry.
//   table   [off x (F + 1) | dst x F | Yx | Yy | Yz] in device memory, copied up once per call from the pinned staging block: the flat node list of
//           tdlo_assign_lane.h and the destination clouds
//   k_assign_count    lane = point; the node list staged through LDS in tiles of kAssignTile nodes (one tile: staged once per workgroup), the lane of
//                     tdlo_assign_lane.h per tile, the gate; owner and g per point; counts[b F + f] from one wave ballot per rope present in the wave
//   k_assign_scatter  offsets of workgroup b = the counts of the workgroups before it, n_f = all of them (every workgroup sums the table itself: nobody waits);
//                     rank of a point among its rope's points of the chunk = popcount of the rope's ballot below the lane + the earlier waves' counts (LDS);
//                     x, y, z stored at column stride n_f.  ride: per rope present in a wave that rope's nodes against the wave's points, one atomic minimum
//                     on the ordered bits per (wave, node), as k_node_min_dist_batch does.
//   state   [T minima as ordered bits (armed: +inf) | ticket].  The workgroup that draws the last ticket hands [n_f x F | T minima] to pinned host memory,
//           re-arms minima and ticket and raises the word the host waits on (system-scope release): the hand-over of tdlo_batch.hip.
#include "tdlo_devcommon.h"
#include "tdlo_assign_lane.h"

namespace tdlo {

constexpr int kAssignMaxWgs = 1024;

void assign_geometry(int n, int *nwg, int *cpb) {
    const int chunks = (n + kBlock - 1) / kBlock;
    *cpb = (chunks + kAssignMaxWgs - 1) / kAssignMaxWgs;
    if (*cpb < 1) *cpb = 1;
    *nwg = (chunks + *cpb - 1) / *cpb;
}

__device__ __forceinline__ int assign_pad4(int n) { return (n + 3) & ~3; }

__global__ __launch_bounds__(kBlock) void k_assign_count(const double *__restrict__ X, int n, const int *__restrict__ off, const double *__restrict__ Y, int F, int T,
                                                        double dmax2, int cpb, int *__restrict__ owner, double *__restrict__ gout, int *__restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *L = (double *)smem;                                   // the tile: x | y | z, kAssignTile each
    int *soff = (int *)(L + 3 * kAssignTile), *scnt = soff + assign_pad4(F + 1);
    const int t = threadIdx.x, lane = t & 63;
    for (int i = t; i <= F; i += kBlock) soff[i] = off[i];
    for (int i = t; i < F; i += kBlock) scnt[i] = 0;
    const bool one = T <= kAssignTile;
    if (one) for (int i = t; i < T; i += kBlock) { L[i] = Y[i]; L[kAssignTile + i] = Y[(size_t)T + i]; L[2 * kAssignTile + i] = Y[2 * (size_t)T + i]; }
    __syncthreads();
    const int chunks = (n + kBlock - 1) / kBlock, c0 = (int)blockIdx.x * cpb, c1 = c0 + cpb < chunks ? c0 + cpb : chunks;
    for (int ch = c0; ch < c1; ++ch) {
        const int i = ch * kBlock + t;
        const bool valid = i < n;
        double x = 0, y = 0, z = 0;
        if (valid) { x = X[i]; y = X[(size_t)n + i]; z = X[2 * (size_t)n + i]; }
        double g = __builtin_huge_val();
        int o = -1, f = 0;
        if (one) assign_tile(L, L + kAssignTile, L + 2 * kAssignTile, 0, T, soff, F, f, x, y, z, g, o);
        else for (int t0 = 0; t0 < T; t0 += kAssignTile) {
            const int cnt = T - t0 < kAssignTile ? T - t0 : kAssignTile;
            __syncthreads();                                       // (the previous tile has been read)
            for (int k = t; k < cnt; k += kBlock) { L[k] = Y[t0 + k]; L[kAssignTile + k] = Y[(size_t)T + t0 + k]; L[2 * kAssignTile + k] = Y[2 * (size_t)T + t0 + k]; }
            __syncthreads();
            assign_tile(L, L + kAssignTile, L + 2 * kAssignTile, t0, cnt, soff, F, f, x, y, z, g, o);
        }
        o = valid ? assign_gate(g, o, dmax2) : -1;
        if (valid) { owner[i] = o; if (gout) gout[i] = g; }
        unsigned long long rem = __ballot(o >= 0);
        while (rem) {                                              // one ballot per rope present in the wave
            const int src = __ffsll((long long)rem) - 1, fr = __shfl(o, src);
            const unsigned long long mk = __ballot(o == fr);
            if (lane == src) atomicAdd(&scnt[fr], (int)__popcll(mk));
            rem &= ~mk;
        }
    }
    __syncthreads();
    for (int i = t; i < F; i += kBlock) counts[(size_t)blockIdx.x * F + i] = scnt[i];
}

__global__ __launch_bounds__(kBlock) void k_assign_scatter(const double *__restrict__ X, int n, const int *__restrict__ owner, const int *__restrict__ counts, int cpb,
                                                          const int *__restrict__ off, double *const *__restrict__ dst, const double *__restrict__ Y, int F, int T, int ride,
                                                          unsigned long long *__restrict__ state, unsigned long long *__restrict__ ticket,
                                                          unsigned long long *__restrict__ res_host, unsigned epoch) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Fp = assign_pad4(F);
    int *stot = (int *)smem, *srun = stot + Fp, *swc = srun + Fp, *slast = swc + 4 * Fp;      // n_f | this workgroup's running offsets | the waves' counts of a chunk
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, b = (int)blockIdx.x, nb = (int)gridDim.x;
    for (int i = t; i < F; i += kBlock) { stot[i] = 0; srun[i] = 0; }
    __syncthreads();
    for (int i = t; i < nb * F; i += kBlock) {
        const int v = counts[i];
        if (v) { const int f = i % F; atomicAdd(&stot[f], v); if (i / F < b) atomicAdd(&srun[f], v); }
    }
    const int chunks = (n + kBlock - 1) / kBlock, c0 = b * cpb, c1 = c0 + cpb < chunks ? c0 + cpb : chunks;
    for (int ch = c0; ch < c1; ++ch) {
        const int i = ch * kBlock + t;
        const int o = i < n ? owner[i] : -1;
        double x = 0, y = 0, z = 0;
        if (o >= 0) { x = X[i]; y = X[(size_t)n + i]; z = X[2 * (size_t)n + i]; }
        for (int k = t; k < 4 * Fp; k += kBlock) swc[k] = 0;
        __syncthreads();                                           // (also: stot / srun are complete)
        int rank = 0;
        unsigned long long rem = __ballot(o >= 0);
        while (rem) {
            const int src = __ffsll((long long)rem) - 1, fr = __shfl(o, src);
            const unsigned long long mk = __ballot(o == fr);
            if (o == fr) rank = (int)__popcll(mk & ((1ull << lane) - 1ull));
            if (lane == src) swc[w * Fp + fr] = (int)__popcll(mk);
            if (ride) {
                const int m0 = off[fr], M = off[fr + 1] - m0;
                for (int m = 0; m < M; ++m) {
                    double d2 = o == fr ? node_point_d2(Y[m0 + m], Y[(size_t)T + m0 + m], Y[2 * (size_t)T + m0 + m], x, y, z) : __builtin_huge_val();
#pragma unroll
                    for (int s = 32; s > 0; s >>= 1) d2 = ::fmin(d2, __shfl_xor(d2, s));
                    if (lane == 0) (void)__hip_atomic_fetch_min(state + m0 + m, (unsigned long long)__double_as_longlong(d2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            rem &= ~mk;
        }
        __syncthreads();
        if (o >= 0) {
            int idx = srun[o] + rank;
            for (int v = 0; v < w; ++v) idx += swc[v * Fp + o];
            const size_t nf = (size_t)stot[o];
            double *D = dst[o];
            D[idx] = x; D[nf + idx] = y; D[2 * nf + idx] = z;      // idx < n_f <= n <= the destination's capacity (the host sized it for n)
        }
        __syncthreads();
        for (int f = t; f < F; f += kBlock) srun[f] += swc[f] + swc[Fp + f] + swc[2 * Fp + f] + swc[3 * Fp + f];
        __syncthreads();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) *slast = __hip_atomic_fetch_add(ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned long long)(gridDim.x - 1);
    __syncthreads();
    if (!*slast) return;
    for (int i = t; i < F; i += kBlock) res_host[1 + i] = (unsigned long long)(unsigned)stot[i];
    if (ride)
        for (int i = t; i < T; i += kBlock) {
            res_host[1 + F + i] = __hip_atomic_load(state + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(state + i, 0x7ff0000000000000ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    if (t == 0) __hip_atomic_store(ticket, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) __hip_atomic_store(res_host, (unsigned long long)epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

hipError_t launch_assign(const double *X, int n, const int *off, double *const *dst, const double *Y, int F, int T, double dmax2, int *owner, double *g, int *counts,
                         bool ride, unsigned long long *state, unsigned long long *ticket, unsigned long long *res_host, unsigned epoch, hipStream_t s) {
    int nwg, cpb;
    assign_geometry(n, &nwg, &cpb);
    const size_t lds_count = sizeof(double) * 3 * kAssignTile + sizeof(int) * (size_t)(((F + 1 + 3) & ~3) + ((F + 3) & ~3));
    hipLaunchKernelGGL(k_assign_count, dim3(nwg), dim3(kBlock), lds_count, s, X, n, off, Y, F, T, dmax2, cpb, owner, g, counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_assign_scatter(X, n, owner, counts, off, dst, Y, F, T, ride, state, ticket, res_host, epoch, s);
}

hipError_t launch_assign_scatter(const double *X, int n, const int *owner, const int *counts, const int *off, double *const *dst, const double *Y, int F, int T,
                                 bool ride, unsigned long long *state, unsigned long long *ticket, unsigned long long *res_host, unsigned epoch, hipStream_t s) {
    int nwg, cpb;
    assign_geometry(n, &nwg, &cpb);
    const size_t lds_scatter = sizeof(int) * (size_t)(6 * ((F + 3) & ~3) + 4);
    hipLaunchKernelGGL(k_assign_scatter, dim3(nwg), dim3(kBlock), lds_scatter, s, X, n, owner, counts, cpb, off, dst, Y, F, T, ride ? 1 : 0, state, ticket, res_host, epoch);
    return hipGetLastError();
}

}  // namespace tdlo
