// The drop-in class started from its first cloud, from plain C++ (include/trackdlo_shim.hpp): initialize_from_cloud on a matrix and on a float view
// must leave exactly sort_pts(reg(cloud)) in the tracker -- reg through the C ABI, sort_pts through the shim's free function (the host twin) -- and
// the tracker must then step.  Built and run by tests/test_init_gpu.py; prints OK.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/trackdlo_shim.hpp"

struct MatrixXd {                       // the subset of Eigen::MatrixXd the shim relies on
    int r = 0, c = 0;
    std::vector<double> v;
    MatrixXd() {}
    MatrixXd(int rows, int cols) : r(rows), c(cols), v((size_t)rows * cols, 0.0) {}
    int rows() const { return r; }
    int cols() const { return c; }
    double *data() { return v.data(); }
    const double *data() const { return v.data(); }
    double &operator()(int i, int j) { return v[(size_t)j * r + i]; }
    double operator()(int i, int j) const { return v[(size_t)j * r + i]; }
};
using trackdlo = tdlo::trackdlo_t<MatrixXd>;

static unsigned long long rng_state = 88172645463325252ull;
static double urand() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (rng_state >> 11) * (1.0 / 9007199254740992.0); }

static bool same(const MatrixXd &a, const MatrixXd &b) { return a.r == b.r && a.c == b.c && std::memcmp(a.data(), b.data(), sizeof(double) * a.v.size()) == 0; }

int main() {
    const int M = 12, N = 600;
    MatrixXd X(N, 3);
    std::vector<float> Xf(8 * (size_t)N, -1.0f);                       // the node's cloud: float points at a stride of 8
    for (int n = 0; n < N; ++n) {
        const double s = urand();
        const double p[3] = {0.15 * std::sin(6.283185307179586 * s), 0.7 * (s - 0.5), 0.05 * std::cos(3.141592653589793 * s)};
        for (int d = 0; d < 3; ++d) { Xf[8 * (size_t)n + d] = (float)(p[d] + 0.004 * (urand() - 0.5)); X(n, d) = (double)Xf[8 * (size_t)n + d]; }
    }
    int err = 0;
    tdlo_ctx *ctx = tdlo_create(nullptr, &err);
    if (!ctx) { std::printf("no device (%d)\n", err); return 1; }
    MatrixXd Yr(M, 3);
    double s2r = 0.0;
    if (tdlo_reg(ctx, 0, X.data(), N, Yr.data(), &s2r, M, 0.05, 30) != TDLO_OK) { std::printf("reg: %s\n", tdlo_last_error(ctx)); return 1; }
    const MatrixXd want = tdlo::sort_pts_t<MatrixXd>(Yr);

    trackdlo tracker(M, 0.008, 0.35, 50000.0, 3.0, 50.0, 0.1, 30, 0.0002, 3.0, 1.0, 10.0);
    tracker.set_precision(TDLO_PREC_F64);
    const double s2 = tracker.initialize_from_cloud(X, 0.05, 30);
    if (!same(tracker.get_tracking_result(), want) || std::memcmp(&s2, &s2r, 8) != 0) { std::printf("matrix route differs\n"); return 1; }
    trackdlo other(M);
    const double s2v = other.initialize_from_cloud(tdlo::view_of(Xf.data(), 8), N, 0.05, 30);
    if (!same(other.get_tracking_result(), want) || std::memcmp(&s2v, &s2r, 8) != 0) { std::printf("view route differs\n"); return 1; }
    if (tracker.get_sigma2() != 0.0) { std::printf("the tracker's sigma2 was touched\n"); return 1; }

    std::vector<int> vis(M);
    for (int m = 0; m < M; ++m) vis[m] = m;
    tracker.set_sigma2(s2);
    tracker.tracking_step(X, vis, vis, MatrixXd(3, 4), 720, 1280);
    const MatrixXd Y = tracker.get_tracking_result();
    double worst = 0.0;
    for (size_t i = 0; i < Y.v.size(); ++i) { if (!std::isfinite(Y.v[i])) { std::printf("non-finite node\n"); return 1; } worst = std::fmax(worst, std::fabs(Y.v[i] - want.v[i])); }
    if (!(worst < 0.05)) { std::printf("the step moved a node by %g m\n", worst); return 1; }
    bool threw = false;
    try { MatrixXd bad(3, 3); tdlo::sort_pts_t<MatrixXd>(bad); } catch (const std::runtime_error &) { threw = true; }      // three equal nodes
    if (!threw) { std::printf("sort_pts accepted equal nodes\n"); return 1; }
    tdlo_destroy(ctx);
    std::printf("OK sigma2 %.6e, the step moved the nodes by at most %.2e m\n", s2, worst);
    return 0;
}
