// The view overloads of the drop-in C++ class (include/trackdlo_shim.hpp): a float cloud at a 32-byte point stride -- the layout of the node's
// pcl::PointCloud<pcl::PointXYZRGB> -- handed over where it lies through tdlo::view_of, against the Matrix overloads on the widened, column-major
// copy that trackdlo_node.cpp:242 makes.  float -> double is exact: the results must be the same BITS.
//   view_test --layout   prints sizeof(tdlo_cloud_view) and the offset of every field (no GPU needed; tests/test_cloud_view.py holds the ctypes
//                        structure to it)
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <limits>
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

struct alignas(16) PointXYZRGB { float x, y, z, pad0; float rgb, pad1, pad2, pad3; };      // pcl::PointXYZRGB's 32 bytes
static_assert(sizeof(PointXYZRGB) == 32, "point stride");

static unsigned long long rng_state = 88172645463325252ull;
static double urand() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (rng_state >> 11) * (1.0 / 9007199254740992.0); }
static double nrand() { return std::sqrt(-2 * std::log(urand() + 1e-300)) * std::cos(6.283185307179586 * urand()); }
static bool same_bits(const std::vector<double> &a, const std::vector<double> &b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; }

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--layout") == 0) {
        std::printf("sizeof=%zu data=%zu dtype=%zu location=%zu stride_point=%zu stride_comp=%zu ready_stream=%zu flags=%zu\n", sizeof(tdlo_cloud_view),
                    offsetof(tdlo_cloud_view, data), offsetof(tdlo_cloud_view, dtype), offsetof(tdlo_cloud_view, location), offsetof(tdlo_cloud_view, stride_point),
                    offsetof(tdlo_cloud_view, stride_comp), offsetof(tdlo_cloud_view, ready_stream), offsetof(tdlo_cloud_view, flags));
        return 0;
    }
    const int M = 30, N = 3001;
    MatrixXd Y0(M, 3), X(N, 3);
    std::vector<PointXYZRGB> cloud(N);
    for (int m = 0; m < M; ++m) { const double s = m / (double)(M - 1); Y0(m, 0) = 0.58 * (s - 0.5); Y0(m, 1) = 0.08 * std::sin(6.283185307179586 * s); Y0(m, 2) = 0.6 + 0.03 * std::cos(9.42477796076938 * s); }
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int n = 0; n < N; ++n) {
        const int i = (int)(urand() * (M - 1)); const double t = urand();
        float p[3];
        for (int d = 0; d < 3; ++d) p[d] = (float)((1 - t) * Y0(i, d) + t * Y0(i + 1, d) + 0.002 * nrand() + (d == 1 ? 0.005 : 0.0));
        cloud[n] = PointXYZRGB{p[0], p[1], p[2], nan, nan, nan, nan, nan};      // (a lane read as a coordinate would show)
        for (int d = 0; d < 3; ++d) X(n, d) = (double)p[d];                     // trackdlo_node.cpp:242
    }
    const tdlo_cloud_view view = tdlo::view_of(&cloud[0].x, sizeof(PointXYZRGB) / 4);
    std::vector<double> coord(M, 0.0);
    for (int m = 1; m < M; ++m) { double s = 0; for (int d = 0; d < 3; ++d) s += (Y0(m, d) - Y0(m - 1, d)) * (Y0(m, d) - Y0(m - 1, d)); coord[m] = coord[m - 1] + std::sqrt(s); }
    int fails = 0;

    // ---- cpd_lle: view overload against the Matrix overload
    for (int lle = 0; lle < 2; ++lle) {
        trackdlo a(M), b(M);
        MatrixXd Ya = Y0, Yb = Y0; double sa = 0, sb = 0;
        const bool ca = a.cpd_lle(view, N, Ya, sa, lle ? 3.0 : 0.35, lle ? 1.0 : 50000, 10.0, 0.1, 20, 0.0, lle != 0);
        const bool cb = b.cpd_lle(X, Yb, sb, lle ? 3.0 : 0.35, lle ? 1.0 : 50000, 10.0, 0.1, 20, 0.0, lle != 0);
        const bool same = same_bits(Ya.v, Yb.v) && std::memcmp(&sa, &sb, sizeof sa) == 0 && ca == cb;
        std::printf("cpd_lle (include_lle=%d) from the view: %s (sigma2 %.9e / %.9e)\n", lle, same ? "identical" : "DIFFERS", sa, sb);
        if (!same) ++fails;
    }
    // ---- tracking_step: three frames, every node visible, then one with a stretch hidden
    {
        trackdlo a(M, 0.008, 0.35, 50000, 3.0, 50.0, 0.1, 30, 0.0002, 3.0, 1.0, 10.0), b(M, 0.008, 0.35, 50000, 3.0, 50.0, 0.1, 30, 0.0002, 3.0, 1.0, 10.0);
        a.initialize_nodes(Y0); a.initialize_geodesic_coord(coord);
        b.initialize_nodes(Y0); b.initialize_geodesic_coord(coord);
        std::vector<int> all, part;
        for (int m = 0; m < M; ++m) { all.push_back(m); if (m < 12 || m >= 19) part.push_back(m); }
        MatrixXd proj(3, 4);
        for (int step = 0; step < 4; ++step) {
            const std::vector<int> &vis = step == 3 ? part : all;
            a.tracking_step(view, N, vis, vis);
            b.tracking_step(X, vis, vis, proj, 720, 1280);
            const double s2a = a.get_sigma2(), s2b = b.get_sigma2();
            std::vector<MatrixXd> Pa = a.get_correspondence_pairs(), Pb = b.get_correspondence_pairs();
            bool same = same_bits(a.get_tracking_result().v, b.get_tracking_result().v) && same_bits(a.get_guide_nodes().v, b.get_guide_nodes().v) &&
                        std::memcmp(&s2a, &s2b, sizeof s2a) == 0 && Pa.size() == Pb.size() && !Pa.empty();
            for (size_t i = 0; same && i < Pa.size(); ++i) same = same_bits(Pa[i].v, Pb[i].v);
            std::printf("tracking_step %d from the view (%zu nodes visible): %s\n", step, vis.size(), same ? "identical" : "DIFFERS");
            if (!same) ++fails;
        }
    }
    std::printf(fails ? "FAILED (%d)\n" : "OK\n", fails);
    return fails;
}
