// tdlo_iter_fused.hip -- one launch per EM iteration of ONE frame: k_iter_fused = M-step (k) ; E-step (k + 1).
//
// The two-launch iteration (k_estep, then k_mstep_chain) is two chains of latency with a kernel boundary behind each: the M-step is one workgroup that waits a
// memory round trip for the sums and one for its records, walks its recursion, and publishes nodes and state to memory so that the next launch's ~200 workgroups
// can read them back -- behind a dependent dispatch.  Here EVERY workgroup of the E-step's grid runs the M-step itself: it is a deterministic function of integer
// sums (64-bit fixed point), so all of them get the same bits, at one workgroup's latency, and then hold the new nodes and the E-step's constants in LDS when
// their E-step part starts.  No workgroup waits for another one: the kernel boundary stays the only synchronisation, there is one per iteration instead of two,
// and the workgroup's points are requested at the top of the kernel and arrive behind the whole M-step.
//
// Nothing a launch reads is written in that launch (its workgroups start at different times):
//   * the iteration number comes with the launch (the host counts), never from the state;
//   * state, Y, Yout and the nodes exist twice (the node block's `alt` copies): launch j reads copy j & 1, its workgroup 0 writes copy (j + 1) & 1;
//   * the accumulators rotate over three buffers: launch j reads j % 3, adds into (j + 1) % 3, its workgroup 0 clears (j + 2) % 3 (the buffer launch j - 1 read);
//   * an E-step half that refuses a contribution reports it in one of two words of `sync` (kFusedErrWord), the next launch reads that one.
// The loop: k_estep (iteration 0, from the set-up's nodes) -> k_iter_fused x (iterations - 1) -> k_mstep_chain<.., CLOSE> (the last M-step; run_frames).
// Both halves are the statements of the two-launch kernels (tdlo_mstep_chain_body.h with FUSE = 1, tdlo_estep_body.inc with FUSED): the same arithmetic in the
// same order, so a registration's Y, sigma2 and iteration count are those of the two-launch loop bit for bit (tests/test_fused_iter_gpu.py).
//
// Two kernels.  k_iter_fused serves every chain of up to 64 nodes.  k_iter_fused_w0 serves the chains whose step slots all fit wave 0 (ChainCarve(M).nSl <= 64: up
// to 61 nodes; launch_iter_fused selects it from the carve, TDLO_FUSED_W0=0 keeps k_iter_fused for every chain -- the comparator).  It is one chain of latencies, so
// what it drops are hand-overs, not work.  The sums travel as in k_iter_fused: all 256 threads request their elements' rows and write S[] in LDS, behind ONE barrier
// -- and the progress counter of the covariance pass is zeroed IN FRONT of that barrier, because it is the last one in front of the recursion: everything behind it
// (records, look-ahead slots, the spike columns' zeros) is wave 0's own, so wave 0 goes from the records into the covariance pass behind a wave-local sync, and the
// means wave and wave 2 read a record only behind the counter.  The slot reads its node's four sums from S[] once, for the record, and keeps them for the tail; lane 0
// forms the new state straight from wave_sum4's rows (no cross-wave sum, no barrier in front of it); waves 1 - 3 zero the E-step's accumulators while they wait at the
// half's closing barrier, and the E-step's own first barrier, with nothing written to LDS since, is left out.  The same statements in the same order: the same bits
// as k_iter_fused and as the two-launch loop (tests/test_fused_w0_gpu.py; the compiled text: tests/test_fused_w0_isa.py).
// (Lane = slot requesting its own sums, with no S[] and the barrier behind the requests only, was built and measured slower: profiles/fused_w0_ab.txt.)
#include "tdlo_mstep_chain_body.h"
#include "tdlo_estep_body.h"
#include <hip/hip_ext.h>
#include <type_traits>

namespace tdlo {

// what changes from launch to launch (the descriptor names the copies the launch READS)
struct FusedLaunch {
    IterState *st_w;            // the copies workgroup 0 writes
    double *Y_w, *Yout_w;
    void *nodes_w;
    long long *acc_clr;         // the accumulator buffer workgroup 0 clears
    int iteration;              // the M-step's iteration (0 = the registration's first)
    int acc_r;                  // the buffer the M-step's sums are in; the E-step half adds into the next one
    int err_r;                  // the error word the M-step half reads; the E-step half writes the other one
};

constexpr size_t kFusedStateBytes = 128;        // the LDS copy of the state between the two halves' regions
static_assert(sizeof(IterState) <= kFusedStateBytes, "IterState outgrew its LDS slot");
static size_t fused_estep_bytes(int M) { return (estep_lds_bytes<float, kCB>(M, true) + 15) & ~(size_t)15; }

// LDS: [ the E-step's carve | state | the M-step's carve ] -- side by side, so that the M-step's tail can put the nodes where the E-step reads them
// (a template on the E-step's precision, instantiated for float alone: the E-step's statements discard their fp64 parts as a template's `if constexpr` does)
template <typename T>
__global__ __launch_bounds__(kCB) void k_iter_fused(const FrameDev f0, const FusedLaunch a, const unsigned estep_bytes) {
    constexpr int NCH = 1, EB = kCB;
    constexpr bool VIS = false, SINGLE = true, FUSED = true;
    const FrameDev &f = f0;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    EstepHand<T> h;
    {
        // Every kernel-argument word that an address of the M-step half's prologue is formed from, asked for HERE, in the kernel's first scalar batch (the
        // descriptor is 0x2d8 bytes of kernel arguments: left to the compiler the words come in six batches, each waited for where it is first used --
        // between the requests for the state, the sums and the slot)
        const void *p0 = f.Xs, *p1 = f.st, *p2 = f.chain, *p3 = f.nodes, *p4 = f.Y, *p5 = f.Y0, *p6 = f.aJ, *p7 = f.aYd, *p8 = f.acc, *p9 = f.sync, *p10 = f.ctr;
        asm volatile("" :: "s"(p0), "s"(p1), "s"(p2), "s"(p3), "s"(p4), "s"(p5), "s"(p6), "s"(p7), "s"(p8), "s"(p9), "s"(p10),
                     "s"(f.N0), "s"(f.M), "s"(f.ldx), "s"(f.has_priors), "s"(f.host_epoch), "s"(f.acc_sh[0]), "s"(f.acc_sh[1]), "s"(f.acc_sh[2]),
                     "s"(a.acc_r), "s"(a.err_r), "s"(estep_bytes));
        // (the one word the E-step half alone needs that the compiler otherwise fetches, waits for and sets aside in the middle of the M-step's requests:
        //  as a value it has to keep)
        h.acc_rows = acc_rows_used(f);
        asm volatile("" : "+s"(h.acc_rows));
        // this lane's first point: on its way while the M-step runs
        h.x = 0; h.y = 0; h.z = 0;
        const auto xs = TDLO_AS_GLOBAL(T, f.Xs);
        const size_t ld = f.ldx;
        const int n = ((int)blockIdx.x * (EB / 64) + (int)(threadIdx.x >> 6)) * 64 + (int)(threadIdx.x & 63);
        if (n < f.N0) { h.x = xs[n]; h.y = xs[ld + n]; h.z = xs[2 * ld + n]; }     // N <= N0: always in bounds
        ChainFused z;
        z.iteration = a.iteration; z.err_r = a.err_r;
        z.st_w = a.st_w; z.Y_w = a.Y_w; z.Yout_w = a.Yout_w; z.nodes_w = a.nodes_w; z.acc_clr = a.acc_clr;
        z.stL = (IterState *)(smem + estep_bytes);
        z.nodesL = smem;                        // (the head of the E-step's carve: nodesL)
        z.go = false;
        mstep_chain_run<T, true, false, false, kAccRows, true, 1>(f, 0, smem + estep_bytes + kFusedStateBytes, a.acc_r, &z);
        if (!z.go) return;                      // (the registration is over: workgroup 0 has said so where it has to be said)
        asm volatile("" :: "s"(__builtin_amdgcn_kernarg_segment_ptr()));
        h.st = z.stL;
        h.acc_buf = a.acc_r == 2 ? 0 : a.acc_r + 1;
        h.err_w = a.err_r ^ 1;
    }
    const EstepHand<T> *const hand = &h;
#include "tdlo_estep_body.inc"
}

// The same launch for chains whose step slots all fit wave 0 (ChainCarve(M).nSl <= 64: up to 61 nodes).  The M-step half is policy FUSE = 3 of
// tdlo_mstep_chain_body.h: no barrier between the records and the covariance pass, none in front of the new state, and the kernel closes the M-step half itself
// (mstep_chain_w0_close) behind the part of the E-step's front that does not depend on the new state.
template <typename T>
__global__ __launch_bounds__(kCB) void k_iter_fused_w0(const FrameDev f0, const FusedLaunch a, const unsigned estep_bytes) {
    constexpr int NCH = 1, EB = kCB;
    constexpr bool VIS = false, SINGLE = true, FUSED = true;
    const FrameDev &f = f0;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    EstepHand<T, true> h;
    {
        // Every kernel-argument word that an address of the M-step half's prologue is formed from, asked for HERE, in the kernel's first scalar batch (the
        // descriptor is 0x2d8 bytes of kernel arguments: left to the compiler the words come in six batches, each waited for where it is first used --
        // between the requests for the state, the sums and the slot)
        const void *p0 = f.Xs, *p1 = f.st, *p2 = f.chain, *p3 = f.nodes, *p4 = f.Y, *p5 = f.Y0, *p6 = f.aJ, *p7 = f.aYd, *p8 = f.acc, *p9 = f.sync, *p10 = f.ctr;
        asm volatile("" :: "s"(p0), "s"(p1), "s"(p2), "s"(p3), "s"(p4), "s"(p5), "s"(p6), "s"(p7), "s"(p8), "s"(p9), "s"(p10),
                     "s"(f.N0), "s"(f.M), "s"(f.ldx), "s"(f.has_priors), "s"(f.host_epoch), "s"(f.acc_sh[0]), "s"(f.acc_sh[1]), "s"(f.acc_sh[2]),
                     "s"(a.acc_r), "s"(a.err_r), "s"(estep_bytes));
        // (the one word the E-step half alone needs that the compiler otherwise fetches, waits for and sets aside in the middle of the M-step's requests:
        //  as a value it has to keep)
        h.acc_rows = acc_rows_used(f);
        asm volatile("" : "+s"(h.acc_rows));
        // this lane's first point: on its way while the M-step runs
        h.x = 0; h.y = 0; h.z = 0;
        const auto xs = TDLO_AS_GLOBAL(T, f.Xs);
        const size_t ld = f.ldx;
        const int n = ((int)blockIdx.x * (EB / 64) + (int)(threadIdx.x >> 6)) * 64 + (int)(threadIdx.x & 63);
        if (n < f.N0) { h.x = xs[n]; h.y = xs[ld + n]; h.z = xs[2 * ld + n]; }     // N <= N0: always in bounds
        ChainFused z;
        z.iteration = a.iteration; z.err_r = a.err_r;
        z.st_w = a.st_w; z.Y_w = a.Y_w; z.Yout_w = a.Yout_w; z.nodes_w = a.nodes_w; z.acc_clr = a.acc_clr;
        z.stL = (IterState *)(smem + estep_bytes);
        z.nodesL = smem;                        // (the head of the E-step's carve: nodesL)
        z.go = false;
        mstep_chain_run<T, true, false, false, kAccRows, true, 3>(f, 0, smem + estep_bytes + kFusedStateBytes, a.acc_r, &z);
        if (!z.go) return;                      // (the registration is over: workgroup 0 has said so where it has to be said)
        // the E-step's front that does not depend on the new state, ahead of the half's closing barrier: waves 1 - 3 idle there and zero their own accumulators,
        // wave 3 those of wave 0 as well -- the wave the barrier waits for
        {
            const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
            if (wv != 0) {
                long long *const own = estep_single_accL<T, EB>(smem, f.M, wv);
                for (int i = (int)(threadIdx.x & 63); i < f.M * 4; i += 64) own[i] = 0;
            }
            if (wv == 3) {
                long long *const first = estep_single_accL<T, EB>(smem, f.M, 0);
                for (int i = (int)(threadIdx.x & 63); i < f.M * 4; i += 64) first[i] = 0;
            }
        }
        mstep_chain_w0_close(f, &z);
        if (!z.go) return;                      // (... or ends with this M-step)
        asm volatile("" :: "s"(__builtin_amdgcn_kernarg_segment_ptr()));
        h.st = z.stL;
        h.acc_buf = a.acc_r == 2 ? 0 : a.acc_r + 1;
        h.err_w = a.err_r ^ 1;
    }
    const EstepHand<T, true> *const hand = &h;
#include "tdlo_estep_body.inc"
}

size_t iter_fused_lds_bytes(int M) { return fused_estep_bytes(M) + kFusedStateBytes + ChainCarve(M).total * sizeof(double); }

// fr: the descriptor with the copies launch `iteration` reads; fw: the one with the copies it writes
// w0: chains whose step slots all fit wave 0 take k_iter_fused_w0 (false: k_iter_fused for every chain -- the comparator, TDLO_FUSED_W0=0); *ran_w0: whether this launch did
static bool iter_fused_w0_fits(int M) { return ChainCarve(M).nSl <= 64; }

hipError_t launch_iter_fused(const FrameDev &fr, const FrameDev &fw, int iteration, bool w0, hipStream_t s, bool *ran_w0) {
    const int M = fr.M;
    if (M > kChunk || fr.precision != TDLO_PREC_F32 || fr.vis_branch || fr.eb != kCB || !fr.wide_tile || fr.estep2) return hipErrorInvalidValue;
    const size_t lds = iter_fused_lds_bytes(M);
    const bool take_w0 = w0 && iter_fused_w0_fits(M);
    const auto kern = !take_w0 ? k_iter_fused<float> : k_iter_fused_w0<float>;
    if (lds > 64 * 1024) { const hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (e != hipSuccess) return e; }
    FusedLaunch a;
    a.st_w = fw.st; a.Y_w = fw.Y; a.Yout_w = fw.Yout; a.nodes_w = fw.nodes;
    a.acc_clr = fr.acc + (size_t)((iteration + 2) % 3) * kAccRows * acc_stride(M);
    a.iteration = iteration; a.acc_r = iteration % 3; a.err_r = (iteration + 1) & 1;
    hipLaunchKernelGGL(kern, dim3(fr.nblkE), dim3(kCB), lds, s, fr, a, (unsigned)fused_estep_bytes(M));
    if (ran_w0) *ran_w0 = take_w0;       // (the kernel that was launched: tdlo_debug_route_count 24 counts from here)
    return hipGetLastError();
}

}  // namespace tdlo
