// tdlo_cluster_lane.h -- one cloud clustered into ropes (include/trackdlo_hip.h, "starting ropes of one colour", has the statement): the link predicate, find,
// "hook the larger root under the smaller" and "owner from root, size and rank", as functions over plain arrays.  No HIP type: the very code a lane of
// k_cluster_link runs per tile of points (tdlo_cluster.hip) compiles for the host (tdlo_cluster_host.cpp: tdlo_cloud_cluster_host) and runs tile by tile, in
// any visiting order, under a sanitizer (tests/cpp/cluster_lane_host_test.cpp).
//
// THE ARITHMETIC is node_point_d2's (tdlo_devcommon.h): dx = fl(a - b) per coordinate, then fma(dz, dz, fma(dy, dy, fl(dx dx))), the fused operations written
// out.  The differences of (a, b) and (b, a) negate exactly, so the predicate is symmetric and a lane needs the points in front of its own only.
// THE FOREST is one int per point: parent[i] <= i always, parent[i] == i for a root, and a word only ever DECREASES -- a root is hooked under a smaller root by
// a compare-and-swap that succeeds once per node, and find shortens the paths it walks by an atomic minimum.  So a walk descends strictly (it ends after at
// most i steps whatever anybody else does), the root of a tree is its smallest index, and once every linked pair has been joined the root of a component is
// its smallest index whatever the schedule was.  On the device the words are read and written by agent-scope atomics (another CU must see them); on the host
// the same functions are plain loads and stores.
// A failed compare-and-swap means somebody else hooked that very root meanwhile; the join goes on from where it points now, at strictly smaller indices.  The
// loop is bounded all the same (kClusterMaxTries): a lane that runs out says so and the driver serves the call on the host.  No lane waits for another.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define TDLO_CLUSTER __host__ __device__ __forceinline__
#else
#define TDLO_CLUSTER inline
#endif

namespace tdlo {

constexpr int kClusterTile = 512;            // points of one LDS tile of k_cluster_link (3 x 512 doubles = 12 KB); a multiple of the workgroup's 256 lanes
// The device route tests ALL pairs in front of every point (n^2 / 2 distance tests: 3.4e10 at this size, some milliseconds of a whole MI355X); the GPU is shared
// and a call's time must stay bounded, so a larger source is refused.  (At this size the per-workgroup tables also stay within the 1024 workgroups of a span.)
constexpr int kClusterMaxPoints = 262144;
constexpr int kClusterMaxTries = 1024;       // compare-and-swap attempts of one join before the lane gives up (each failure is a hook somebody else made)

TDLO_CLUSTER bool cluster_finite(double x, double y, double z) { return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z); }

TDLO_CLUSTER double cluster_d2(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
}

// link(a, b) for a != b: both finite and node_point_d2(a, b) <= fl(tol tol)
TDLO_CLUSTER bool cluster_link(double ax, double ay, double az, double bx, double by, double bz, double tol2) {
    return cluster_d2(ax, ay, az, bx, by, bz) <= tol2 && cluster_finite(ax, ay, az) && cluster_finite(bx, by, bz);
}

TDLO_CLUSTER int cluster_load(const int *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}

// *p = min(*p, v): a parent only decreases
TDLO_CLUSTER void cluster_lower(int *p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    if (v < *p) *p = v;
#endif
}

// if (*p == expect) *p = v; returns what *p held
TDLO_CLUSTER int cluster_cas(int *p, int expect, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)__hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expect;
#else
    const int old = *p;
    if (old == expect) *p = v;
    return old;
#endif
}

// the root of i's tree; every node on the way is pointed at its grandparent.  parent[k] < k for every node that is not a root: at most i steps
TDLO_CLUSTER int cluster_find(int *parent, int i) {
    int p = cluster_load(parent + i);
    while (p != i) {
        const int g = cluster_load(parent + p);
        if (g != p) cluster_lower(parent + i, g);
        i = p; p = g;
    }
    return i;
}

// The trees of r and j become one: the larger root is hooked under the smaller.  r: any node of the lane's own tree, replaced by the root the join ended on (a
// lane keeps it from pair to pair, so its own walk stays short).  false: kClusterMaxTries compare-and-swaps failed, nothing is promised about the pair
TDLO_CLUSTER bool cluster_join(int *parent, int &r, int j) {
    int a = r, b = j;
    for (int tries = 0; tries < kClusterMaxTries; ++tries) {
        a = cluster_find(parent, a); b = cluster_find(parent, b);
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        if (a == b || cluster_cas(parent + hi, hi, lo) == hi) {
            r = lo;
            cluster_lower(parent + j, lo);      // j hangs directly under the root now: the next lane that meets it need not walk (cluster_tile)
            return true;
        }
        a = hi; b = lo;      // (hi is no root any more: the next find goes on from where it points now)
    }
    return false;
}

// The lane of the FINITE point i = (x, y, z) against the tile [t0, t0 + cnt) of the cloud, its points at Lx / Ly / Lz [0, cnt): every point j < i of the tile
// that links is joined.  The tiles in front of i may come in any order.  false: a join gave up
TDLO_CLUSTER bool cluster_tile(const double *Lx, const double *Ly, const double *Lz, int t0, int cnt, int i, double x, double y, double z, double tol2,
                               int *parent, int &r) {
    const int lim = i - t0 < cnt ? i - t0 : cnt;
    for (int k0 = 0; k0 < lim; k0 += 64) {
        // 64 points at a time.  First the links alone, as a word of bits: arithmetic and the tile, no forest word is touched
        const int kc = lim - k0 < 64 ? lim - k0 : 64;
        unsigned long long m = 0;
        for (int k = 0; k < kc; ++k) {
            const double bx = Lx[k0 + k], by = Ly[k0 + k], bz = Lz[k0 + k];
            m |= (unsigned long long)(cluster_d2(x, y, z, bx, by, bz) <= tol2 && cluster_finite(bx, by, bz)) << k;
        }
        // then the linked points four at a time: their parents are loaded together (one memory round trip for four), and a point that hangs directly under r
        // is in the lane's tree already -- a word read a while ago still names an ancestor, trees never split -- so only the others are joined
        while (m) {
            int j[4] = {0, 0, 0, 0}, p[4] = {0, 0, 0, 0}, c = 0;      // (loops of a fixed four: the arrays stay in registers)
            for (int q = 0; q < 4; ++q)
                if (m) { j[q] = t0 + k0 + __builtin_ctzll(m); m &= m - 1; c = q + 1; }
            for (int q = 0; q < 4; ++q)
                if (q < c) p[q] = cluster_load(parent + j[q]);
            for (int q = 0; q < 4; ++q)
                if (q < c && p[q] != r && !cluster_join(parent, r, j[q])) return false;
        }
    }
    return true;
}

// a root r with size(r) finite members is a cluster that is kept
TDLO_CLUSTER bool cluster_kept(int size_r, int min_size) { return size_r >= min_size; }

// owner(i) from i's root r: size_r = size(r) (0 for a point that is not finite: it is its own root and counts nowhere), rank_r = the number of kept roots
// below r (read only where the root is kept)
TDLO_CLUSTER int cluster_owner(int size_r, int rank_r, int min_size, int F) { return (cluster_kept(size_r, min_size) && rank_r < F) ? rank_r : -1; }

}  // namespace tdlo
