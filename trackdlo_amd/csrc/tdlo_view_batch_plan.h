// tdlo_view_batch_plan.h -- where the F frames of a batched voxel grid on cloud views (k_cloud_view_batch, tdlo_cloud.hip; tdlo_cloud_view_voxel_grid_batch)
// keep their blocks in the context's view-batch arena.  Plain host code: no HIP, no context (tests/cpp/view_batch_plan_host_test.cpp builds it alone;
// tdlo_debug_view_batch_plan).
//
//   [ Fcap state blocks | descriptor table | frame 0: tile regions, compacted points, tile counts | frame 1: ... ]
//   state    256 bytes per frame (the kernel's box, tickets and spare words), frame f's at 256 f: an array whose place depends on nothing but the frame's
//            position in the call -- neither on the N of any frame nor on F (Fcap is the context's slot count, fixed when it is made).  The words the kernel
//            re-arms at the end of a launch are therefore the words the next call's frame f finds, although every other block moves from call to call
//   table    F descriptors of desc_bytes each (the kernel's records; copied up from pinned memory in front of the launch)
//   frame f  tile regions 3 N_f floats (tile b's kept points at [b 4096 ...) of each coordinate), the compacted points 3 x 32 704 floats, one count per tile
//            of 4096 elements -- sized by the frame's OWN N, one frame behind the other
//   Every block starts on 256 bytes.  A frame of more than kViewBatchMaxN elements has no place here: the call hands it to the single call.
#pragma once

#include <cstddef>

namespace tdlo {

constexpr int kViewBatchTile = 4096;           // elements per tile (k_cloud_fused's: 1024 threads x 4)
constexpr int kViewBatchPts = 32704;           // points the in-LDS sort of a frame's finishing workgroup takes
constexpr int kViewBatchMaxN = 1 << 20;        // elements of a frame the batch launch takes: 256 tiles (a 1280 x 720 organized cloud has 921 600), tile regions of 12.6 MB
constexpr long long kViewBatchState = 256;     // bytes of a frame's state block

inline long long view_plan_r256(long long b) { return (b + 255) & ~255ll; }
inline int view_plan_tiles(int N) { return (int)(((long long)N + kViewBatchTile - 1) / kViewBatchTile); }
inline long long view_plan_tiles_bytes(int N) { return view_plan_r256(3ll * N * 4); }
inline long long view_plan_pts_bytes() { return view_plan_r256(3ll * kViewBatchPts * 4); }
inline long long view_plan_cnt_bytes(int N) { return view_plan_r256(4ll * view_plan_tiles(N)); }

// Fills state_off / tiles_off / pts_off / cnt_off (F entries each, in bytes from the arena's start; any may be null), *table_off and *total.
// Returns 0, or -1 for F < 1, F > Fcap, desc_bytes < 1, a null N or an N[f] outside 1 .. kViewBatchMaxN.
inline int view_batch_plan(const int *N, int F, int Fcap, long long desc_bytes, long long *state_off, long long *tiles_off, long long *pts_off, long long *cnt_off,
                           long long *table_off, long long *total) {
    if (!N || F < 1 || F > Fcap || desc_bytes < 1) return -1;
    for (int f = 0; f < F; ++f) if (N[f] < 1 || N[f] > kViewBatchMaxN) return -1;
    long long at = kViewBatchState * Fcap;
    if (table_off) *table_off = at;
    at += view_plan_r256(desc_bytes * F);
    for (int f = 0; f < F; ++f) {
        if (state_off) state_off[f] = kViewBatchState * f;
        if (tiles_off) tiles_off[f] = at;
        at += view_plan_tiles_bytes(N[f]);
        if (pts_off) pts_off[f] = at;
        at += view_plan_pts_bytes();
        if (cnt_off) cnt_off[f] = at;
        at += view_plan_cnt_bytes(N[f]);
    }
    if (total) *total = at;
    return 0;
}

}  // namespace tdlo
