// tdlo_align_batch.hip -- depth aligned to the colour camera for J jobs in two launches (tdlo_align_depth_batch and the aligning rig calls;
// include/trackdlo_hip.h has the statement, tdlo_align_batch_plan.h the arena): the single call's kernels (tdlo_align.hip) with the job as the grid's second
// dimension.  No grid barrier, nobody waits for anybody.
//
//   k_align_splat_batch   grid (blocks of 256 lanes of the job with the most depth pixels, J).  Workgroup row j fetches record j of the job table -- wave-uniform,
//                         read-only kernel input: one copy at the top, in front of every store, so the loads are uniform loads and the record lives in scalar
//                         registers -- and a workgroup past its own job's rows_d x cols_d leaves at once.  The lane is align_splat_lane of tdlo_align_lane.h,
//                         the single kernel's text: one element load by format and pitch, both corners in registers, one returnless relaxed agent-scope 32-bit
//                         atomic minimum per offered word of the job's own scratch plane.  The four counts: ballot and popcount, one atomic add per wave and
//                         count into the job's own words.
//   k_align_pack_batch    grid (blocks of the job with the most colour pixels / 4, J).  The lane is align_pack_lane: one 16-byte load, one 8-byte store, the
//                         words armed again.  A job's first four lanes hand its counts to the pinned words counts_out + 4 j and zero them.
// A job's bits are the single call's: the same lane text, this unit built with tdlo_align.hip's flags (-ffp-contract=off, no fast-math flag), a minimum that does
// not depend on the order of its operands, and no word shared between two jobs.
#include "tdlo_internal.h"
#include "tdlo_align_batch_plan.h"

namespace tdlo {

namespace {

__global__ __launch_bounds__(kBlock) void k_align_splat_batch(const AlignBatchRec *__restrict__ table) {
    const AlignBatchRec *__restrict__ rec = table + blockIdx.y;
    const AlignJob job = rec->job;
    unsigned *const scratch = rec->scratch;
    unsigned long long *const counts = rec->counts;
    if ((int)(blockIdx.x * kBlock) >= job.rows_d * job.cols_d) return;                                   // (workgroup-uniform: a shorter job's spare workgroups)
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

__global__ __launch_bounds__(kBlock) void k_align_pack_batch(const AlignBatchRec *__restrict__ table, unsigned long long *__restrict__ counts_out) {
    const AlignBatchRec *__restrict__ rec = table + blockIdx.y;
    const int P = rec->job.rows_c * rec->job.cols_c;
    unsigned *const scratch = rec->scratch;
    unsigned short *const out = rec->plane;
    unsigned long long *const counts = rec->counts;
    if ((int)(blockIdx.x * kBlock) >= (P + 3) / 4) return;                                               // (workgroup-uniform)
    const int t = (int)(blockIdx.x * kBlock + threadIdx.x);
    align_pack_lane(scratch, out, P, t);
    if (t < 4) {                                          // the job's counts (complete: the launch before this one) -> the caller's words; armed again
        const unsigned long long n = __hip_atomic_load(counts + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(counts_out + 4 * blockIdx.y + t, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(counts + t, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

// table: J records in device memory whose blocks follow align_batch_plan (scratch armed, counts zero); most_Pd / most_Pc: the most depth / colour pixels of a
// job (1 .. 2^26); counts_out: 4 J words the host reads after the stream's next wait (pinned host memory)
hipError_t launch_align_batch(const AlignBatchRec *table, int J, int most_Pd, int most_Pc, unsigned long long *counts_out, hipStream_t s) {
    if (!table || !counts_out || J < 1 || J > kAlignBatchMaxJobs || most_Pd < 1 || most_Pc < 1 || most_Pd > (1 << 26) || most_Pc > (1 << 26)) return hipErrorInvalidValue;
    const int lanes = (most_Pc + 3) / 4;
    hipLaunchKernelGGL(k_align_splat_batch, dim3((unsigned)((most_Pd + kBlock - 1) / kBlock), (unsigned)J), dim3(kBlock), 0, s, table);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_align_pack_batch, dim3((unsigned)((lanes + kBlock - 1) / kBlock), (unsigned)J), dim3(kBlock), 0, s, table, counts_out);
    return hipGetLastError();
}

}  // namespace tdlo
