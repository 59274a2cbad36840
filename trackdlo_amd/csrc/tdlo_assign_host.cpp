// tdlo_assign_host.cpp -- one cloud dealt out among F ropes on the host (include/trackdlo_hip.h has the statement): the argument check, the flat node list as
// the kernels' staging block holds it, and the lane of tdlo_assign_lane.h run point by point.  Pure C++: no HIP, no device, so that a stand-alone program can run
// every line under a sanitizer (tests/cpp/assign_lane_host_test.cpp); built with -ffp-contract=off like tdlo_rig_host.cpp.
#include "tdlo_assign_host.h"

#include <cmath>

namespace tdlo {

const char *assign_fault(const tdlo_assign_rope *ropes, int F, double d_max) {
    if (!ropes) return "cloud assign: null ropes";
    if (F < 1) return "cloud assign: F < 1";
    if (!(d_max > 0)) return "cloud assign: d_max must be positive (INFINITY: no gate)";
    long long total = 0;
    for (int f = 0; f < F; ++f) {
        if (!ropes[f].Y || ropes[f].M < 1) return "cloud assign: a rope without nodes";
        total += ropes[f].M;
        if (total > (1ll << 30)) return "cloud assign: too many nodes";
        for (size_t q = 0; q < 3 * (size_t)ropes[f].M; ++q)
            if (!std::isfinite(ropes[f].Y[q])) return "cloud assign: a node that is not finite";
    }
    return nullptr;
}

void assign_flatten(const tdlo_assign_rope *ropes, int F, int *off, double *Yx, double *Yy, double *Yz) {
    int o = 0;
    for (int f = 0; f < F; ++f) {
        const int M = ropes[f].M;
        off[f] = o;
        for (int m = 0; m < M; ++m) { Yx[o + m] = ropes[f].Y[m]; Yy[o + m] = ropes[f].Y[(size_t)M + m]; Yz[o + m] = ropes[f].Y[2 * (size_t)M + m]; }
        o += M;
    }
    off[F] = o;
}

void assign_points_host(const double *X, int n, const int *off, int F, const double *Yx, const double *Yy, const double *Yz, double dmax2, int tile,
                        int *owner, double *owner_d2) {
    const int total = off[F];
    for (int i = 0; i < n; ++i) {
        const double x = X[i], y = X[(size_t)n + i], z = X[2 * (size_t)n + i];
        double g = __builtin_huge_val();
        int o = -1, f = 0;
        for (int t0 = 0; t0 < total; t0 += tile) {
            const int cnt = total - t0 < tile ? total - t0 : tile;
            assign_tile(Yx + t0, Yy + t0, Yz + t0, t0, cnt, off, F, f, x, y, z, g, o);
        }
        if (owner) owner[i] = assign_gate(g, o, dmax2);
        if (owner_d2) owner_d2[i] = g;
    }
}

}  // namespace tdlo

extern "C" {

int tdlo_cloud_assign_host(const double *X, int n, const tdlo_assign_rope *ropes, int F, double d_max, int *owner, double *owner_d2, int *n_each, int *n_unowned) {
    if (n < 0 || (n > 0 && !X) || tdlo::assign_fault(ropes, F, d_max)) return TDLO_E_INVALID;
    std::vector<int> off((size_t)F + 1), own((size_t)n);
    long long total = 0;
    for (int f = 0; f < F; ++f) total += ropes[f].M;
    std::vector<double> Y(3 * (size_t)total);
    tdlo::assign_flatten(ropes, F, off.data(), Y.data(), Y.data() + total, Y.data() + 2 * total);
    tdlo::assign_points_host(X, n, off.data(), F, Y.data(), Y.data() + total, Y.data() + 2 * total, d_max * d_max, tdlo::kAssignTile, own.data(), owner_d2);
    std::vector<int> cnt((size_t)F, 0);
    int un = 0;
    for (int i = 0; i < n; ++i) { if (own[i] >= 0) ++cnt[own[i]]; else ++un; }
    if (owner) for (int i = 0; i < n; ++i) owner[i] = own[i];
    if (n_each) for (int f = 0; f < F; ++f) n_each[f] = cnt[f];
    if (n_unowned) *n_unowned = un;
    return TDLO_OK;
}

}  // extern "C"
