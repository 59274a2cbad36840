// tdlo_reg_batch.hip -- `reg` (tdlo_reg.hip) for F clouds in the same 2 + 2 max_iter launches: the frames are the grid's second dimension.
//
// One tracker's start is tdlo_reg.hip's loop: an E-step of at most 256 workgroups and a one-workgroup M-step per iteration, the kernel boundary the
// hand-over between them.  A first cloud off the voxel grid fills 2 .. 20 workgroups, so F trackers started one by one are F times those launches on a
// nearly empty GPU.  Here every launch serves all frames:
//   k_reg_estep_batch  grid (max nblk_f, F): workgroup (b, f) is workgroup b of frame f's nblk_f and returns at once where b >= nblk_f
//   k_reg_mstep_batch  grid F: frame f's partials added in block order, its sigma2, c and centroids
// Every frame has its own state block and its own partials (RegBatchFrame; tdlo_reg_plan.h lays them out) and no workgroup waits for another.  The
// two bodies are k_reg_estep's and k_reg_mstep's statement by statement -- keep them in step with tdlo_reg.hip -- with the frame's own N, nblk_f and
// pointers in place of the launch's: the same grid-stride, the same butterfly, the same order of every sum, and this unit is built with tdlo_reg.hip's
// flags, so a frame's sigma2 and centroids are the single call's bit for bit whatever else is in the batch (tests/test_init_batch_gpu.py).
// tdlo_reg.hip itself is left as it is: the single call's code object does not change.
// The loop stays 2 launches per iteration: a batch's loop in one launch was measured four times slower, and folding the M-step into
// the last E-step workgroup to arrive would save one launch gap of an iteration's ~58 us.
#include "tdlo_internal.h"

namespace tdlo {
namespace {

constexpr int kRB = 256;

__device__ __forceinline__ double wsum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// state: [0] sigma2, [1] c, [2] Np (last), then Y (3 M, column-major) at +8
// part: per block 5 M + 1 doubles: P1 (M), PX (3 M), sum P d2 per node (M), [5 M] = sum of d2 (init mode)
__global__ __launch_bounds__(kRB) void k_reg_estep_batch(const RegBatchFrame *__restrict__ tab, int M, int init) {
    extern __shared__ double sm[];              // Y (3 M) | acc (4 waves x (5 M + 1))
    const RegBatchFrame fr = tab[blockIdx.y];
    const int nblk = fr.nblk, N = fr.N;
    if ((int)blockIdx.x >= nblk) return;        // (the whole workgroup: no barrier is left waiting)
    const double *__restrict__ X = fr.X, *__restrict__ state = fr.state;
    double *__restrict__ part = fr.part;
    double *Ys = sm, *acc = sm + 3 * M;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, nacc = 5 * M + 1;
    for (int i = t; i < 3 * M; i += kRB) Ys[i] = state[8 + i];
    for (int i = t; i < 4 * nacc; i += kRB) acc[i] = 0.0;
    __syncthreads();
    const double sigma2 = state[0], c = state[1];
    const double k2 = -0.5 / sigma2;
    double *my = acc + w * nacc;
    for (int base = blockIdx.x * kRB; base < N; base += nblk * kRB) {
        const int n = base + t;
        const bool ok = n < N;
        const double x = ok ? X[n] : 0.0, y = ok ? X[(size_t)N + n] : 0.0, z = ok ? X[2 * (size_t)N + n] : 0.0;
        if (init) {
            double s = 0.0;
            for (int m = 0; m < M; ++m) { const double dx = Ys[m] - x, dy = Ys[M + m] - y, dz = Ys[2 * M + m] - z; s += dx * dx + dy * dy + dz * dz; }
            s = wsum(ok ? s : 0.0);
            if (lane == 0) my[5 * M] += s;
            continue;
        }
        double den = 0.0;
        for (int m = 0; m < M; ++m) {
            const double dx = Ys[m] - x, dy = Ys[M + m] - y, dz = Ys[2 * M + m] - z;
            den += exp(k2 * (dx * dx + dy * dy + dz * dz));                        // :55
        }
        const double rden = ok ? 1.0 / (den + c) : 0.0;                            // :58
        for (int m = 0; m < M; ++m) {
            const double dx = Ys[m] - x, dy = Ys[M + m] - y, dz = Ys[2 * M + m] - z;
            const double d2 = dx * dx + dy * dy + dz * dz;
            const double p = exp(k2 * d2) * rden;
            const double s0 = wsum(p), s1 = wsum(p * x), s2 = wsum(p * y), s3 = wsum(p * z), s4 = wsum(p * d2);
            if (lane == 0) { my[m] += s0; my[M + m] += s1; my[2 * M + m] += s2; my[3 * M + m] += s3; my[4 * M + m] += s4; }
        }
    }
    __syncthreads();
    for (int i = t; i < nacc; i += kRB) part[(size_t)blockIdx.x * nacc + i] = ((acc[i] + acc[nacc + i]) + acc[2 * nacc + i]) + acc[3 * nacc + i];
}

__global__ __launch_bounds__(kRB) void k_reg_mstep_batch(const RegBatchFrame *__restrict__ tab, int M, double mu, int init) {
    extern __shared__ double S[];               // 5 M + 1
    const RegBatchFrame fr = tab[blockIdx.x];
    const int nblk = fr.nblk, N = fr.N;
    const double *__restrict__ part = fr.part;
    double *__restrict__ state = fr.state;
    const int t = threadIdx.x, nacc = 5 * M + 1;
    for (int i = t; i < nacc; i += kRB) { double a = 0.0; for (int b = 0; b < nblk; ++b) a += part[(size_t)b * nacc + i]; S[i] = a; }
    __syncthreads();
    if (t == 0) {
        double sigma2;
        if (init) sigma2 = S[5 * M] / (3.0 * (double)M * (double)N);              // :45
        else {
            double num = 0.0, np = 0.0;
            for (int m = 0; m < M; ++m) { num += S[4 * M + m]; np += S[m]; }      // :70-79
            sigma2 = num / (np * 3.0);
            state[2] = np;
        }
        state[0] = sigma2;
        state[1] = pow(2.0 * M_PI * sigma2, 1.5) * mu / (1.0 - mu) * (double)M / (double)N;   // :57
    }
    if (!init) for (int i = t; i < 3 * M; i += kRB) state[8 + i] = S[M + i] / S[i % M];       // :60-68 (0 / 0 -> NaN like the reference)
}

}  // namespace

hipError_t launch_reg_batch(const RegBatchFrame *tab_dev, int F, int max_nblk, int M, double mu, int max_iter, hipStream_t s) {
    const size_t lds_e = sizeof(double) * (3 * (size_t)M + 4 * (5 * (size_t)M + 1)), lds_m = sizeof(double) * (5 * (size_t)M + 1);
    if (lds_e > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)k_reg_estep_batch, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_e);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_reg_estep_batch, dim3(max_nblk, F), dim3(kRB), lds_e, s, tab_dev, M, 1);
    hipLaunchKernelGGL(k_reg_mstep_batch, dim3(F), dim3(kRB), lds_m, s, tab_dev, M, mu, 1);
    for (int it = 0; it < max_iter; ++it) {
        hipLaunchKernelGGL(k_reg_estep_batch, dim3(max_nblk, F), dim3(kRB), lds_e, s, tab_dev, M, 0);
        hipLaunchKernelGGL(k_reg_mstep_batch, dim3(F), dim3(kRB), lds_m, s, tab_dev, M, mu, 0);
    }
    return hipGetLastError();
}

}  // namespace tdlo
