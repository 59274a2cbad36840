// tdlo_reg_plan.h -- where the F frames of a batched start (tdlo_reg_batch.hip; tdlo_reg_batch, tdlo_tracker_initialize_from_cloud_batch) keep their
// doubles in the `reg` workspace.  Plain host code: no HIP, no context (tests/cpp/reg_plan_host_test.cpp builds it alone; tdlo_debug_reg_batch_plan).
//
//   [ F state blocks | F frames' partials | F output blocks ]
//   state    8 + 3 M doubles as the single call keeps them (sigma2, c, Np, ... | Y column-major), at a stride of 8 + 3 M + (3 M & 1): every block
//            starts on 16 bytes, and the F start states are ONE contiguous upload
//   partials frame f: nblk_f x (5 M + 1) doubles, nblk_f = max(1, min(ceil(N_f / 256), 256)) -- tdlo_reg's rule -- one frame behind the other
//   output   k_sort_pts' block [sigma2 | status | Y sorted (3 M) | coord (M)] and M ints, 2 + 4 M + ceil(M / 2) doubles, at an even stride from an even
//            offset: 16-byte aligned each
//   total    F (8 + 3 M) + sum nblk_f (5 M + 1) + F (2 + 4 M + ceil(M / 2)) + 8 F: the single call's reg_ws_doubles + sort_pts_out_doubles per frame
//            (its 8 spare doubles pay for the three pads), so one frame asks for exactly what the single call asks for, and its state and partials lie
//            where the single call has them
#pragma once

#include <cstddef>

namespace tdlo {

constexpr int kRegBlock = 256;         // k_reg_estep's workgroup
constexpr int kRegMaxBlocks = 256;     // ... and the most workgroups a frame's E-step is spread over

inline int reg_plan_nblk(int N) {
    const int b = N > 0 ? (int)(((long long)N + kRegBlock - 1) / kRegBlock) : 0;
    return b < 1 ? 1 : (b > kRegMaxBlocks ? kRegMaxBlocks : b);
}
inline long long reg_plan_state_stride(int M) { return 8 + 3 * (long long)M + ((3 * (long long)M) & 1); }
inline long long reg_plan_part_doubles(int M, int nblk) { return (long long)nblk * (5 * (long long)M + 1); }
inline long long reg_plan_out_doubles(int M) { return 2 + 4 * (long long)M + ((long long)M + 1) / 2; }
inline long long reg_plan_out_stride(int M) { const long long o = reg_plan_out_doubles(M); return o + (o & 1); }

// Fills nblk / state_off / part_off / out_off (F entries each, in doubles from the workspace's start; any may be null) and *total.
// Returns 0, or -1 for F < 1, M < 1, a null N or an N[f] < 1.
inline int reg_batch_plan(const int *N, int F, int M, int *nblk, long long *state_off, long long *part_off, long long *out_off, long long *total) {
    if (!N || F < 1 || M < 1) return -1;
    for (int f = 0; f < F; ++f) if (N[f] < 1) return -1;
    const long long S = reg_plan_state_stride(M), O = reg_plan_out_stride(M);
    long long at = S * F, sum = 0;
    for (int f = 0; f < F; ++f) {
        const int b = reg_plan_nblk(N[f]);
        if (nblk) nblk[f] = b;
        if (state_off) state_off[f] = S * f;
        if (part_off) part_off[f] = at;
        at += reg_plan_part_doubles(M, b);
        sum += reg_plan_part_doubles(M, b);
    }
    at += at & 1;
    for (int f = 0; f < F; ++f) if (out_off) out_off[f] = at + O * f;
    if (total) *total = (long long)F * (8 + 3 * (long long)M) + sum + (long long)F * reg_plan_out_doubles(M) + 8 * (long long)F;
    return 0;
}

}  // namespace tdlo
