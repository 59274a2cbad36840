// tdlo_cluster_host.cpp -- one cloud clustered into ropes on the host (include/trackdlo_hip.h has the statement): the argument check, the plain all-pairs form
// over the lane of tdlo_cluster_lane.h -- point by point, every point in front of it, the whole cloud as one tile -- and the owners from roots, sizes and ranks.
// It is the statement, not a competitor of the kernels.  Pure C++: no HIP, no device, so that a stand-alone program can run every line under a sanitizer
// (tests/cpp/cluster_lane_host_test.cpp); built with -ffp-contract=off like tdlo_assign_host.cpp.  The driver's declarations are in tdlo_internal.h.
#include <cmath>
#include <vector>

#include "../../include/trackdlo_hip.h"
#include "tdlo_cluster_lane.h"

namespace tdlo {

const char *cluster_fault(int F, double tol, int min_size) {
    if (F < 1) return "cloud cluster: F < 1";
    if (!(tol > 0) || !std::isfinite(tol)) return "cloud cluster: tol must be positive and finite";
    if (min_size < 1) return "cloud cluster: min_size < 1";
    return nullptr;
}

// owner [n] of checked arguments (X: n x 3 column-major); returns C, the number of kept clusters.  false: a join gave up (on the host: never)
bool cluster_owners_host(const double *X, int n, int F, double tol2, int min_size, int *owner, int *n_clusters) {
    std::vector<int> parent((size_t)n), size((size_t)n, 0), rank((size_t)n, 0);
    const double *Xx = X, *Xy = X + (size_t)n, *Xz = X + 2 * (size_t)n;
    for (int i = 0; i < n; ++i) parent[i] = i;
    for (int i = 0; i < n; ++i) {
        if (!cluster_finite(Xx[i], Xy[i], Xz[i])) continue;
        int r = i;
        if (!cluster_tile(Xx, Xy, Xz, 0, n, i, Xx[i], Xy[i], Xz[i], tol2, parent.data(), r)) return false;
    }
    for (int i = 0; i < n; ++i) {
        parent[i] = cluster_find(parent.data(), i);
        if (cluster_finite(Xx[i], Xy[i], Xz[i])) ++size[parent[i]];
    }
    int C = 0;
    for (int i = 0; i < n; ++i)
        if (parent[i] == i && cluster_kept(size[i], min_size)) rank[i] = C++;
    for (int i = 0; i < n; ++i) owner[i] = cluster_owner(size[parent[i]], rank[parent[i]], min_size, F);
    *n_clusters = C;
    return true;
}

// counts [nwg x F] as k_assign_count leaves them: workgroup b owns the cpb chunks of `block` points from chunk b cpb on
void cluster_counts_host(const int *owner, int n, int F, int block, int nwg, int cpb, int *counts) {
    for (size_t k = 0; k < (size_t)nwg * F; ++k) counts[k] = 0;
    for (int i = 0; i < n; ++i)
        if (owner[i] >= 0) ++counts[(size_t)(i / block / cpb) * F + owner[i]];
}

}  // namespace tdlo

extern "C" {

int tdlo_cloud_cluster_host(const double *X, int n, int F, double tol, int min_size, int *owner, int *n_clusters, int *n_each, int *n_unowned) {
    if (n < 0 || n > tdlo::kClusterMaxPoints || (n > 0 && !X) || tdlo::cluster_fault(F, tol, min_size)) return TDLO_E_INVALID;
    std::vector<int> own((size_t)n), cnt((size_t)F, 0);
    int C = 0, un = 0;
    if (!tdlo::cluster_owners_host(X, n, F, tol * tol, min_size, own.data(), &C)) return TDLO_E_NUMERIC;
    for (int i = 0; i < n; ++i) { if (own[i] >= 0) ++cnt[own[i]]; else ++un; }
    if (owner) for (int i = 0; i < n; ++i) owner[i] = own[i];
    if (n_clusters) *n_clusters = C;
    if (n_each) for (int f = 0; f < F; ++f) n_each[f] = cnt[f];
    if (n_unowned) *n_unowned = un;
    return TDLO_OK;
}

}  // extern "C"
