// tdlo_cell_painter_host.cpp -- the painter test over a cell of ropes on the host (include/trackdlo_hip.h has the statement): the argument check, the cell
// flattened as the kernels take it, the lane of tdlo_cell_painter_lane.h run camera by camera, and each rope's verdict from the cameras' words.  Pure C++: no
// HIP, no device, so that a stand-alone program can run every line under a sanitizer (tests/cpp/cell_painter_lane_host_test.cpp); built with
// -ffp-contract=off like tdlo_painter_host.cpp.
#include "tdlo_cell_painter_host.h"

#include <cstring>

namespace tdlo {

const char *cell_painter_fault(const tdlo_cell_rope *ropes, int F, const tdlo_rig_camera *cams, const double *rig_to_cam, int K, int rows, int cols,
                               int dlo_pixel_width, bool need_dist) {
    if (!ropes || F < 1) return "cell occlusion: null ropes or F < 1";
    static const double some_dist = 0.0;
    // (every refusal of the rig test -- the cameras, the width, the image size -- with the first rope; the other ropes bring nodes and distances alone)
    if (const char *why = rig_painter_fault(ropes[0].Y, ropes[0].M, cams, rig_to_cam, K, rows, cols, dlo_pixel_width, need_dist ? ropes[0].node_dist : &some_dist))
        return why;
    long long N = 0;
    for (int f = 0; f < F; ++f) {
        const tdlo_cell_rope &r = ropes[f];
        if (!r.Y || (need_dist && !r.node_dist)) return "cell occlusion: null Y / node_dist";
        if (r.M < 1 || r.M > kPainterMaxNodes) return "cell occlusion: 1 .. 1024 nodes a rope";
        N += r.M;
        if (N > kCellPainterMaxNodes) return "cell occlusion: more than 16 384 nodes in a cell (every node meets every edge: a call's time must stay bounded)";
    }
    return nullptr;
}

int cell_painter_nodes(const tdlo_cell_rope *ropes, int F) {
    int N = 0;
    for (int f = 0; f < F; ++f) N += ropes[f].M;
    return N;
}

void cell_painter_flatten(const tdlo_cell_rope *ropes, int F, double *X, double *Y, double *Z, unsigned *link) {
    std::vector<int> Ms(F);
    int off = 0;
    for (int f = 0; f < F; ++f) {
        const int M = ropes[f].M;
        Ms[f] = M;
        std::memcpy(X + off, ropes[f].Y, sizeof(double) * M);
        std::memcpy(Y + off, ropes[f].Y + M, sizeof(double) * M);
        std::memcpy(Z + off, ropes[f].Y + 2 * (size_t)M, sizeof(double) * M);
        off += M;
    }
    cell_link_words(Ms.data(), F, link);
}

void cell_painter_host(const double *X, const double *Y, const double *Z, const unsigned *link, int N, const PainterCam *cams, int K, int rows, int cols,
                       int dlo_pixel_width, unsigned *seen_words, unsigned *hidden_words) {
    const int W = (N + 31) / 32;
    std::vector<CellRec> tab(N);
    for (int k = 0; k < K; ++k)
        cell_job(cams[k], X, Y, Z, link, N, rows, cols, dlo_pixel_width, tab.data(), seen_words + (size_t)k * W, hidden_words + (size_t)k * W);
}

void cell_painter_verdict(const unsigned *seen_words, const unsigned *hidden_words, int K, int N, int off, int M, const double *node_dist,
                          double visibility_threshold, std::vector<int> &vis) {
    const int W = (N + 31) / 32;
    vis.clear();
    for (int m = 0; m < M; ++m) {
        if (!(node_dist[m] <= visibility_threshold)) continue;      // (a NaN distance fails)
        const int n = off + m;
        unsigned ok = 0u;
        for (int k = 0; k < K; ++k) ok |= seen_words[(size_t)k * W + (n >> 5)] & ~hidden_words[(size_t)k * W + (n >> 5)];
        if (ok & (1u << (n & 31))) vis.push_back(m);
    }
}

}  // namespace tdlo

extern "C" {

int tdlo_cell_occlusion_visible(const tdlo_cell_rope *ropes, int F, const tdlo_rig_camera *cams, const double *rig_to_cam, int K, int rows, int cols,
                                int dlo_pixel_width, int *const *visible_nodes, int *n_vis, unsigned *seen_words, unsigned *hidden_words) {
    using namespace tdlo;
    if (!visible_nodes || !n_vis || cell_painter_fault(ropes, F, cams, rig_to_cam, K, rows, cols, dlo_pixel_width)) return TDLO_E_INVALID;
    for (int f = 0; f < F; ++f) if (!visible_nodes[f]) return TDLO_E_INVALID;
    const int N = cell_painter_nodes(ropes, F), W = (N + 31) / 32;
    std::vector<PainterCam> pc(K);
    for (int k = 0; k < K; ++k) rig_painter_camera(cams[k], rig_to_cam ? rig_to_cam + 12 * (size_t)k : nullptr, pc[k]);
    std::vector<double> xyz(3 * (size_t)N);
    std::vector<unsigned> link(W), seen((size_t)K * W), hidden((size_t)K * W);
    cell_painter_flatten(ropes, F, xyz.data(), xyz.data() + N, xyz.data() + 2 * (size_t)N, link.data());
    cell_painter_host(xyz.data(), xyz.data() + N, xyz.data() + 2 * (size_t)N, link.data(), N, pc.data(), K, rows, cols, dlo_pixel_width, seen.data(), hidden.data());
    std::vector<int> vis;
    int off = 0;
    for (int f = 0; f < F; ++f) {
        cell_painter_verdict(seen.data(), hidden.data(), K, N, off, ropes[f].M, ropes[f].node_dist, ropes[f].visibility_threshold, vis);
        n_vis[f] = (int)vis.size();
        for (size_t i = 0; i < vis.size(); ++i) visible_nodes[f][i] = vis[i];
        off += ropes[f].M;
    }
    if (seen_words) std::memcpy(seen_words, seen.data(), sizeof(unsigned) * seen.size());
    if (hidden_words) std::memcpy(hidden_words, hidden.data(), sizeof(unsigned) * hidden.size());
    return TDLO_OK;
}

}  // extern "C"
