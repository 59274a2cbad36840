// tdlo_batch.hip -- the visibility pre-pass of F slots in ONE launch (tdlo_visibility_prepass_batch).
//
// k_node_min_dist_batch is k_node_min_dist_direct (tdlo_device.hip) over a table of frames: per node the shortest squared distance to the frame's raw
// cloud (trackdlo/src/trackdlo_node.cpp:257-277), fp64, node_point_d2 -- the one statement of the distance that every pre-pass kernel shares, so the
// bits are the single call's.  A minimum does not depend on how the points are dealt out to lanes, waves and workgroups.
//   grid    one flat grid over the frames' point workgroups: frame i owns workgroups [wg0[i], wg0[i + 1]), at most 1024 of them (a larger cloud
//           takes further trips of the grid-stride loop, as in the single call)
//   table   VisBatchFrame[F] and wg0[F + 1] in the pinned staging block, the F node blocks (3 M doubles each, column-major) behind them: every
//           workgroup finds its frame, then stages that frame's nodes into LDS
//   state   [0 .. F M) minima as ordered bits (armed: +inf), one ticket behind them.  The workgroup that draws the last ticket of the LAUNCH hands
//           all F M minima to pinned host memory, re-arms minima and ticket and raises the word the host waits on (system-scope release).
#include "tdlo_devcommon.h"

namespace tdlo {

__global__ __launch_bounds__(kBlock) void k_node_min_dist_batch(const VisBatchFrame *__restrict__ tab, const int *__restrict__ wg0, const double *__restrict__ Yhost,
                                                               int F, int M, unsigned long long *__restrict__ state, unsigned long long *__restrict__ ticket,
                                                               unsigned long long *__restrict__ res_host, unsigned epoch) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *Yl = (double *)smem;
    __shared__ int sframe, slast;
    const int t = threadIdx.x, lane = t & 63, b = (int)blockIdx.x;
    if (t == 0) sframe = 0;
    __syncthreads();
    for (int i = t; i < F; i += kBlock)
        if (wg0[i] <= b && b < wg0[i + 1]) sframe = i;      // (the ranges are disjoint and cover the grid: exactly one thread writes)
    __syncthreads();
    const int fr = sframe;
    const double *X = tab[fr].X;
    const int N = tab[fr].N0, first = wg0[fr], nwg = wg0[fr + 1] - first;
    const double *Yf = Yhost + (size_t)fr * 3 * M;
    for (int i = t; i < 3 * M; i += kBlock) Yl[i] = Yf[i];
    __syncthreads();
    unsigned long long *row = state + (size_t)fr * M;
    for (int base = (b - first) * kBlock; base < N; base += nwg * kBlock) {
        const int n = base + t;
        const bool valid = n < N;
        double x = 0, y = 0, z = 0;
        if (valid) { x = X[n]; y = X[(size_t)N + n]; z = X[2 * (size_t)N + n]; }
        for (int m = 0; m < M; ++m) {
            double d2 = valid ? node_point_d2(Yl[m], Yl[M + m], Yl[2 * M + m], x, y, z) : __builtin_huge_val();
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) d2 = ::fmin(d2, __shfl_xor(d2, o));
            if (lane == 0) (void)__hip_atomic_fetch_min(row + m, (unsigned long long)__double_as_longlong(d2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) slast = __hip_atomic_fetch_add(ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned long long)(gridDim.x - 1);
    __syncthreads();
    if (!slast) return;
    const int FM = F * M;
    for (int i = t; i < FM; i += kBlock) {
        res_host[1 + i] = __hip_atomic_load(state + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(state + i, 0x7ff0000000000000ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (t == 0) __hip_atomic_store(ticket, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) __hip_atomic_store(res_host, (unsigned long long)epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

int node_min_dist_batch_wgs(int N) {
    int blocks = (N + kBlock - 1) / kBlock;
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    return blocks;
}

hipError_t launch_node_min_dist_batch(const VisBatchFrame *tab, const int *wg0, const double *Yhost, int F, int M, int nwg, unsigned long long *state,
                                      unsigned long long *ticket, unsigned long long *res_host, unsigned epoch, hipStream_t s) {
    hipLaunchKernelGGL(k_node_min_dist_batch, dim3(nwg), dim3(kBlock), sizeof(double) * 3 * M, s, tab, wg0, Yhost, F, M, state, ticket, res_host, epoch);
    return hipGetLastError();
}

}  // namespace tdlo
