// tdlo_align.hip -- depth aligned to the colour camera on the device (tdlo_align_depth; include/trackdlo_hip.h has the statement): two launches, no grid
// barrier, nobody waits for anybody.
//
//   k_align_splat   lane = depth pixel, a wave's lanes consecutive in u (the depth loads coalesce; one element load per lane by format and pitch, so pitched
//                   and bottom-up rows, U16 and F32 are all views).  Both corners in registers (tdlo_align_lane.h: the host statement's text, this unit
//                   built with -ffp-contract=off and no fast-math flag, so its divisions are IEEE divisions), then the footprint loop: one returnless 32-bit
//                   unsigned atomic minimum per offered word of the rows_c x cols_c scratch plane (there is no 16-bit atomic).  A minimum does not depend
//                   on the order of its operands, so the plane has one right bit pattern whatever the schedule.  The atomics are relaxed and of agent
//                   scope -- adders sit on all eight XCDs, whose L2s are not coherent, and nothing in THIS launch reads a word back; the launch boundary
//                   publishes the plane to k_align_pack.  The four counts: one ballot and popcount per wave and count, one atomic add per wave and count.
//   k_align_pack    lane = four output pixels: one 16-byte load of the scratch plane, one 8-byte store of the uint16 plane (all ones -> 0), one 16-byte
//                   store that arms the words again -- the next call of the size needs no fill launch and a stale word can never leak; the plane's last
//                   1 .. 3 words go element by element.  Its first lanes hand the four counts to the caller's words and zero them.
//
// Workgroups of 256 lanes (four wave64, as the other pixel-parallel kernels here): a lane holds two corners in fp64 and no LDS, so occupancy is bounded by
// registers alone and the launch is short; nothing in it depends on the workgroup's size.
#include "tdlo_internal.h"
#include "tdlo_align_lane.h"

namespace tdlo {

namespace {

__global__ __launch_bounds__(kBlock) void k_align_splat(const AlignJob job, unsigned *__restrict__ scratch, unsigned long long *__restrict__ counts) {
    const int verdict = align_splat_lane(job, (int)(blockIdx.x * kBlock + threadIdx.x), [scratch](int i, unsigned k) {
        (void)__hip_atomic_fetch_min(scratch + i, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // result unused: the returnless form
    });
    const unsigned long long any = __ballot(verdict != kAlignZero);
    if (any == 0ull) return;                                                                           // (wave-uniform)
    const unsigned long long used = __ballot(verdict == kAlignUsed), dropped = __ballot(verdict == kAlignDropped), wide = __ballot(verdict == kAlignWide);
    if ((threadIdx.x & 63u) == 0u) {
        (void)__hip_atomic_fetch_add(counts, (unsigned long long)__popcll(any), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (used) (void)__hip_atomic_fetch_add(counts + 1, (unsigned long long)__popcll(used), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (dropped) (void)__hip_atomic_fetch_add(counts + 2, (unsigned long long)__popcll(dropped), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (wide) (void)__hip_atomic_fetch_add(counts + 3, (unsigned long long)__popcll(wide), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kBlock) void k_align_pack(unsigned *__restrict__ scratch, unsigned short *__restrict__ out, int P,
                                                      unsigned long long *__restrict__ counts, unsigned long long *__restrict__ counts_out) {
    const int t = (int)(blockIdx.x * kBlock + threadIdx.x);
    align_pack_lane(scratch, out, P, t);
    if (t < 4) {                                          // the splat's counts (complete: the launch before this one) -> the caller's words; armed again
        const unsigned long long n = __hip_atomic_load(counts + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(counts_out + t, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(counts + t, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

// scratch: rows_c x cols_c armed words (all ones: the first use of an allocation fills it once, k_align_pack keeps it armed), 16-byte aligned; out: the uint16 plane, 8-byte aligned; counts: 4 zeroed device words; counts_out: 4 words the host
// reads after the stream's next wait (pinned host memory)
hipError_t launch_align(const AlignJob &job, unsigned *scratch, unsigned short *out, unsigned long long *counts, unsigned long long *counts_out, hipStream_t s) {
    if (!job.depth || !scratch || !out || !counts || !counts_out || ((uintptr_t)scratch & 15u) || ((uintptr_t)out & 7u)) return hipErrorInvalidValue;
    if (job.rows_d < 1 || job.cols_d < 1 || job.rows_c < 1 || job.cols_c < 1 || (long long)job.rows_d * job.cols_d > (1ll << 26) ||
        (long long)job.rows_c * job.cols_c > (1ll << 26) || job.max_fp < 1 || job.max_fp > kAlignMaxFootprintLimit)
        return hipErrorInvalidValue;
    const int Pd = job.rows_d * job.cols_d, Pc = job.rows_c * job.cols_c, lanes = (Pc + 3) / 4;
    hipLaunchKernelGGL(k_align_splat, dim3((unsigned)((Pd + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, job, scratch, counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_align_pack, dim3((unsigned)((lanes + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, scratch, out, Pc, counts, counts_out);
    return hipGetLastError();
}

}  // namespace tdlo
