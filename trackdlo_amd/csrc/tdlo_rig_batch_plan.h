// tdlo_rig_batch_plan.h -- where the F frames of a batched rig call (k_cloud_rig_batch, tdlo_cloud.hip; tdlo_rig_to_cloud_batch) keep their blocks in the
// context's rig-batch arena, and which frames share a launch.  Plain host code: no HIP, no context (tests/cpp/rig_batch_plan_host_test.cpp builds it alone;
// tdlo_debug_rig_batch_plan).
//
//   [ Fcap state blocks | frame table | camera table | planes | the frame blocks of ONE launch: frame a: tile regions, compacted points, tile counts | frame b: ... ]
//   state    256 bytes per SLOT of the context (the kernel's box, tickets and spare words), the block of the frame that names slot s at 256 s: its place depends
//            on nothing but the slot -- neither on the other frames, nor on F, K or the image size (Fcap is the context's slot count, fixed when it is made).
//            The words the kernel re-arms at the end of a launch are therefore the words the next call into that slot finds, although every other block moves
//   table    F descriptors of desc_bytes each, in the order of the call's frames (the kernel's records; copied up from pinned memory in front of the launches)
//   cameras  sum K_f records of cam_bytes each, frame after frame: frame f's K_f records start at cams_off[f]
//   planes   every distinct (pointer, kind) of the call once -- kind 0 depth (2 P bytes), 1 mask (P), 2 colour (3 P), 3 occluder (P) --, each padded as the
//            single calls pad their planes (the colour lanes' 12-byte loads end up to 9 bytes beyond an image) and rounded up to 256 bytes: 8-byte aligned
//   frame f  tile regions 3 x K_f x Tc x 4096 floats (Tc = ceil(P / 4096) tiles a camera; tile b's kept points at [b 4096 ...) of each coordinate), the
//            compacted points 3 x 32 704 floats, one count per tile.  Every block starts on 256 bytes.
// BYTES.  With r(b) = b rounded up to 256:
//   fixed    = 256 Fcap + r(desc_bytes F) + r(cam_bytes sum K_f) + sum over distinct planes of { r(2 P), r(P), r(3 P + 16), r(P + 16) }[kind]
//   frame(K) = r(12 K Tc 4096) + r(12 x 32 704) + r(4 K Tc)            -- K times the cloud batch's: about 33 MB for three 1280 x 720 cameras
//   total    = fixed + max over the launches of the sum of frame(K_f) over the launch's frames
// THE BUDGET.  A launch covers only as many frames as keep fixed + its frames' blocks within `budget` bytes (kRigBatchBudget for the library): walking the
// frames in the call's order, a frame that would push the running sum beyond the budget starts the next launch -- a launch has at least one frame, whatever
// its size.  The launches follow one another on one stream, so the frame blocks of launch l + 1 lie where those of launch l lay: only blocks of the SAME launch
// (and the fixed part) are disjoint.  A rig of more than 4095 tiles has no place here: the call hands it to the single call.
#pragma once

#include <cstddef>

namespace tdlo {

constexpr int kRigBatchTile = 4096;            // pixels per tile (k_cloud_fused's: 1024 threads x 4)
constexpr int kRigBatchPts = 32704;            // points the in-LDS sort of a frame's finishing workgroup takes
constexpr int kRigBatchMaxTiles = 4095;        // tiles of a frame (their offsets live in the finishing workgroup's LDS)
constexpr int kRigBatchMaxCams = 64;           // cameras of a rig (tdlo_rig_point.h: kRigMaxCams)
constexpr long long kRigBatchState = 256;      // bytes of a slot's state block
constexpr long long kRigBatchBudget = 1ll << 30;      // bytes of arena one launch may address: 1 GiB

inline long long rig_plan_r256(long long b) { return (b + 255) & ~255ll; }
inline int rig_plan_tiles(int P) { return (int)(((long long)P + kRigBatchTile - 1) / kRigBatchTile); }      // of ONE camera
inline long long rig_plan_plane_bytes(int kind, long long P) {
    return rig_plan_r256(kind == 0 ? 2 * P : kind == 1 ? P : kind == 2 ? 3 * P + 16 : P + 16);
}
inline long long rig_plan_tiles_bytes(int K, int P) { return rig_plan_r256(3ll * K * rig_plan_tiles(P) * kRigBatchTile * 4); }
inline long long rig_plan_pts_bytes() { return rig_plan_r256(3ll * kRigBatchPts * 4); }
inline long long rig_plan_cnt_bytes(int K, int P) { return rig_plan_r256(4ll * K * rig_plan_tiles(P)); }
inline long long rig_plan_frame_bytes(int K, int P) { return rig_plan_tiles_bytes(K, P) + rig_plan_pts_bytes() + rig_plan_cnt_bytes(K, P); }

// slot, K: F entries.  plane: 4 keys per camera (depth, mask, colour, occluder; 0: the camera has none), camera after camera, frame after frame -- 4 sum K_f
// entries; two entries name the same plane when key and kind agree.  Fills (bytes from the arena's start; any output may be null) state_off / cams_off /
// tiles_off / pts_off / cnt_off / launch_of (F entries each), plane_off (4 sum K_f entries; -1 where the key is 0), *table_off, *total, *n_planes (distinct
// planes) and *n_launches.  Returns 0, or -1 for F < 1, F > Fcap, P < 1, desc_bytes / cam_bytes / budget < 1, a null slot / K / plane, a slot outside
// 0 .. Fcap - 1 or named twice, a K[f] outside 1 .. 64 or with more than 4095 tiles.
inline int rig_batch_plan(const int *slot, const int *K, int F, int Fcap, int P, const unsigned long long *plane, long long desc_bytes, long long cam_bytes,
                          long long budget, long long *state_off, long long *cams_off, long long *plane_off, long long *tiles_off, long long *pts_off,
                          long long *cnt_off, int *launch_of, long long *table_off, long long *total, int *n_planes, int *n_launches) {
    if (!slot || !K || !plane || F < 1 || F > Fcap || P < 1 || desc_bytes < 1 || cam_bytes < 1 || budget < 1) return -1;
    const int Tc = rig_plan_tiles(P);
    long long cams = 0;
    for (int f = 0; f < F; ++f) {
        if (slot[f] < 0 || slot[f] >= Fcap) return -1;
        for (int g = 0; g < f; ++g) if (slot[g] == slot[f]) return -1;
        if (K[f] < 1 || K[f] > kRigBatchMaxCams || (long long)K[f] * Tc > kRigBatchMaxTiles) return -1;
        cams += K[f];
    }
    long long at = kRigBatchState * Fcap;
    if (table_off) *table_off = at;
    at += rig_plan_r256(desc_bytes * F);
    {
        long long k0 = 0;
        for (int f = 0; f < F; ++f) {
            if (state_off) state_off[f] = kRigBatchState * slot[f];
            if (cams_off) cams_off[f] = at + cam_bytes * k0;
            k0 += K[f];
        }
    }
    at += rig_plan_r256(cam_bytes * cams);
    // ---- the planes: entry e is new unless an earlier entry has its key and kind (a quadratic walk over 4 sum K_f entries: a few hundred in a work cell)
    int distinct = 0;
    const long long E = 4 * cams;
    for (long long e = 0; e < E; ++e) {
        if (!plane[e]) { if (plane_off) plane_off[e] = -1; continue; }
        long long seen = -1;
        for (long long d = e & 3; d < e; d += 4) if (plane[d] == plane[e]) { seen = d; break; }
        if (seen >= 0) {
            if (plane_off) plane_off[e] = plane_off[seen];
            continue;
        }
        if (plane_off) plane_off[e] = at;
        at += rig_plan_plane_bytes((int)(e & 3), P);
        ++distinct;
    }
    if (n_planes) *n_planes = distinct;
    // ---- the frame blocks, launch by launch
    const long long fixed = at;
    long long cur = 0, most = 0;
    int launch = 0;
    for (int f = 0; f < F; ++f) {
        const long long need = rig_plan_frame_bytes(K[f], P);
        if (cur > 0 && fixed + cur + need > budget) { ++launch; cur = 0; }
        long long b = fixed + cur;
        if (tiles_off) tiles_off[f] = b;
        b += rig_plan_tiles_bytes(K[f], P);
        if (pts_off) pts_off[f] = b;
        b += rig_plan_pts_bytes();
        if (cnt_off) cnt_off[f] = b;
        if (launch_of) launch_of[f] = launch;
        cur += need;
        most = cur > most ? cur : most;
    }
    if (total) *total = fixed + most;
    if (n_launches) *n_launches = launch + 1;
    return 0;
}

}  // namespace tdlo
