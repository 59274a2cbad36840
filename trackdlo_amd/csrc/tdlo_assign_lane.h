// tdlo_assign_lane.h -- one cloud dealt out among F ropes (include/trackdlo_hip.h, "ropes of one colour", has the statement): the owner and the distance g
// of ONE point from a list of nodes, as functions over plain arrays.  No HIP type: the very code a lane of k_assign_count runs per node tile (tdlo_assign.hip)
// compiles for the host (tdlo_assign_host.cpp: tdlo_cloud_assign_host) and runs tile by tile under a sanitizer (tests/cpp/assign_lane_host_test.cpp).
//
// THE ARITHMETIC is node_point_d2's (tdlo_devcommon.h): dx = fl(y - x) per coordinate, then fma(dz, dz, fma(dy, dy, fl(dx dx))) -- the fused operations written
// out, so that no contraction setting changes them (the g++ unit that includes this header is built with -ffp-contract=off all the same).  Minima are fmin: a
// NaN never wins.
// THE NODE LIST is flat: the ropes' nodes one rope behind the other, coordinate by coordinate (Yx, Yy, Yz of off[F] entries each), rope f at [off[f], off[f + 1]).
// A TILE is a window [t0, t0 + cnt) of the flat list; a lane walks the tiles in ascending order with a cursor f (the first rope that is not finished) and folds
// every piece of a rope it meets into (g, owner): ropes ascend and only `<` replaces, so the lowest rope wins a tie wherever a tile border falls.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define TDLO_ASSIGN __host__ __device__ __forceinline__
#else
#define TDLO_ASSIGN inline
#endif

namespace tdlo {

constexpr int kAssignTile = 512;         // nodes of one LDS tile of k_assign_count (3 x 512 doubles = 12 KB)
constexpr int kAssignRideMaxNodes = 1024;   // nodes of a rope up to which its pre-pass may ride in k_assign_scatter (the pre-pass's own one-launch limit)

TDLO_ASSIGN double assign_d2(double yx, double yy, double yz, double x, double y, double z) {
    const double dx = yx - x, dy = yy - y, dz = yz - z;
    return __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
}

// cnt >= 1 consecutive nodes of rope f folded into the point's running (g, owner)
TDLO_ASSIGN void assign_fold(const double *yx, const double *yy, const double *yz, int cnt, int f, double x, double y, double z, double &g, int &owner) {
    double d = __builtin_huge_val();
    for (int m = 0; m < cnt; ++m) d = __builtin_fmin(d, assign_d2(yx[m], yy[m], yz[m], x, y, z));
    if (d < g) { g = d; owner = f; }
}

// the tile [t0, t0 + cnt) of the flat list, its nodes at Lx / Ly / Lz [0, cnt): every rope piece inside it, in ascending rope order.  f: the cursor, 0 before the first tile
TDLO_ASSIGN void assign_tile(const double *Lx, const double *Ly, const double *Lz, int t0, int cnt, const int *off, int F, int &f,
                             double x, double y, double z, double &g, int &owner) {
    const int t1 = t0 + cnt;
    while (f < F) {
        const int a = off[f] > t0 ? off[f] : t0, b = off[f + 1] < t1 ? off[f + 1] : t1;
        if (a >= t1) break;
        if (b > a) assign_fold(Lx + (a - t0), Ly + (a - t0), Lz + (a - t0), b - a, f, x, y, z, g, owner);
        if (off[f + 1] > t1) break;      // the rope goes on in the next tile
        ++f;
    }
}

// the gate: g must be finite and g <= fl(d_max d_max) (dmax2; +inf: no gate)
TDLO_ASSIGN int assign_gate(double g, int owner, double dmax2) { return (owner >= 0 && g < __builtin_huge_val() && g <= dmax2) ? owner : -1; }

}  // namespace tdlo
