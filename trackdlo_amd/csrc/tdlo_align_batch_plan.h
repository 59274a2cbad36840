// tdlo_align_batch_plan.h -- where the J jobs of a batched align call (k_align_splat_batch / k_align_pack_batch, tdlo_align_batch.hip; tdlo_align_depth_batch
// and the aligning rig calls) keep their blocks in the context's align-batch arena, the record a workgroup row fetches, and the rule that makes two
// (view, params) entries ONE job.  Plain host code: no HIP, no context (tests/cpp/align_batch_host_test.cpp builds it alone; tdlo_debug_align_batch_plan).
//
//   [ scratch region: job 0's plane of 32-bit words | job 1's | ... ][ uint16 planes: job 0's | job 1's | ... ][ count words: 4 per job ][ job table: one record per job ]
//   scratch  rows_c x cols_c words per job, every plane 16-byte aligned (the pack's one 16-byte access per lane); the region ends on 256 bytes
//   planes   rows_c x cols_c uint16 per job, every plane 256-byte aligned: what device_planes hands out, what tdlo_view_batch_images' consumers and the render
//            batch (4-byte aligned device memory read in place) and the rig calls (a device depth plane) read
//   counts   4 x 64-bit words per job, job j's at counts_off[j] = counts_off[0] + 32 j (zero when a call's launches start: they go up with the table)
//   table    one AlignBatchRec of 256 bytes per job, in the order of the call's jobs
// BYTES.  With r16 / r256 = rounded up to 16 / 256 and P_j = rows_c[j] cols_c[j]:
//   scratch_bytes = r256(sum r16(4 P_j)),  total = scratch_bytes + sum r256(2 P_j) + r256(32 J) + 256 J        (64 cameras of 1280 x 720: about 0.35 GiB)
// THE INVARIANT that makes a change of layout safe: EVERY WORD OF THE SCRATCH REGION IS ARMED (all ones) BETWEEN CALLS.  The region is filled once, when the arena
// is allocated or the region grows beyond the bytes filled so far; the splat offers only to words inside the planes of the CURRENT layout (the lane's decision
// drops a footprint that is not wholly inside its own plane); the pack arms again every word of every plane of the current layout -- and the bytes between two
// planes (up to 12 after a plane, up to 255 at the region's end) are never written by anybody.  So a call whose layout differs from the one before -- other
// sizes, another order, another J -- needs no fill launch and can never see a stale word.  A layout whose scratch region is SHORTER than the one before puts
// planes, counts or the table over words that were armed: the library then counts only the new region as filled (and fills the difference when it grows again).
// LIMITS.  J is 1 .. kAlignBatchMaxJobs; a total beyond the budget (kAlignBatchBudget for the library, 1 GiB) has no plan: the call is refused.
#pragma once

#include "tdlo_align_lane.h"

namespace tdlo {

constexpr int kAlignBatchMaxJobs = 1024;
constexpr long long kAlignBatchBudget = 1ll << 30;

// what workgroup row j of the two batch kernels fetches: wave-uniform, read-only kernel input
struct alignas(16) AlignBatchRec {
    AlignJob job;
    unsigned *scratch;               // the job's rows_c x cols_c armed words
    unsigned short *plane;           // the job's uint16 plane
    unsigned long long *counts;      // the job's four count words (zero when the splat starts)
    unsigned long long spare[3];
};
static_assert(sizeof(AlignBatchRec) == 256, "the align batch record is 256 bytes");

inline long long align_plan_r16(long long b) { return (b + 15) & ~15ll; }
inline long long align_plan_r256(long long b) { return (b + 255) & ~255ll; }

// rows_c, cols_c: J entries.  Fills (bytes from the arena's start; any output may be null) scratch_off / plane_off / counts_off (J entries each), *table_off,
// *scratch_bytes and *total.  Returns 0, or -1 for J outside 1 .. 1024, null sizes, a size below 1 or beyond 2^26 pixels, budget < 1, a total beyond the budget.
inline int align_batch_plan(const int *rows_c, const int *cols_c, int J, long long budget, long long *scratch_off, long long *plane_off, long long *counts_off,
                            long long *table_off, long long *scratch_bytes, long long *total) {
    if (!rows_c || !cols_c || J < 1 || J > kAlignBatchMaxJobs || budget < 1) return -1;
    long long at = 0;
    for (int j = 0; j < J; ++j) {
        if (rows_c[j] < 1 || cols_c[j] < 1 || (long long)rows_c[j] * cols_c[j] > (1ll << 26)) return -1;
        at += align_plan_r16(4ll * rows_c[j] * cols_c[j]);
    }
    const long long sb = align_plan_r256(at);
    long long all = sb;
    for (int j = 0; j < J; ++j) all += align_plan_r256(2ll * rows_c[j] * cols_c[j]);
    const long long cnt_at = all;
    all += align_plan_r256(32ll * J);
    const long long tab_at = all;
    all += (long long)sizeof(AlignBatchRec) * J;
    if (all > budget) return -1;
    at = 0;
    long long pl = sb;
    for (int j = 0; j < J; ++j) {
        const long long P = (long long)rows_c[j] * cols_c[j];
        if (scratch_off) scratch_off[j] = at;
        if (plane_off) plane_off[j] = pl;
        if (counts_off) counts_off[j] = cnt_at + 32ll * j;
        at += align_plan_r16(4 * P);
        pl += align_plan_r256(2 * P);
    }
    if (table_off) *table_off = tab_at;
    if (scratch_bytes) *scratch_bytes = sb;
    if (total) *total = all;
    return 0;
}

// THE DISTINCT-JOB RULE of the aligning rig calls: two (camera, frame) entries with equal view fields (data, format, row_stride, location, ready_stream) and
// bytewise-equal params -- the matrix compared by value: both NULL, or twelve doubles with the same bytes -- are ONE job
inline bool align_same_job(const tdlo_image_view &a, const tdlo_align_params &p, const tdlo_image_view &b, const tdlo_align_params &q) {
    if (a.data != b.data || a.format != b.format || a.row_stride != b.row_stride || a.location != b.location || a.ready_stream != b.ready_stream) return false;
    if (p.rows_d != q.rows_d || p.cols_d != q.cols_d || p.rows_c != q.rows_c || p.cols_c != q.cols_c || p.max_footprint != q.max_footprint) return false;
    const double x[8] = {p.fx_d, p.fy_d, p.cx_d, p.cy_d, p.fx_c, p.fy_c, p.cx_c, p.cy_c}, y[8] = {q.fx_d, q.fy_d, q.cx_d, q.cy_d, q.fx_c, q.fy_c, q.cx_c, q.cy_c};
    if (__builtin_memcmp(x, y, sizeof x)) return false;
    if (!p.depth_to_colour || !q.depth_to_colour) return !p.depth_to_colour && !q.depth_to_colour;
    return __builtin_memcmp(p.depth_to_colour, q.depth_to_colour, 12 * sizeof(double)) == 0;
}

// n entries -> job_of[e] (the index of entry e's job among the distinct ones, numbered in order of first appearance); returns the number of distinct jobs
inline int align_distinct_jobs(const tdlo_image_view *views, const tdlo_align_params *params, int n, int *job_of) {
    int distinct = 0;
    for (int e = 0; e < n; ++e) {
        int seen = -1;
        for (int d = 0; d < e && seen < 0; ++d)
            if (align_same_job(views[d], params[d], views[e], params[e])) seen = job_of[d];
        job_of[e] = seen >= 0 ? seen : distinct++;
    }
    return distinct;
}

}  // namespace tdlo
