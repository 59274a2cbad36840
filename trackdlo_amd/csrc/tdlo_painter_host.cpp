// tdlo_painter_host.cpp -- the self-occlusion test under a rig on the host (include/trackdlo_hip.h has the statement): the argument check, a camera as the
// kernel's table holds it, the lane of tdlo_painter_lane.h run camera by camera, and the rig's verdict from the cameras' words.  Pure C++: no HIP, no device, so
// that a stand-alone program can run every line under a sanitizer (tests/cpp/rig_painter_test.cpp); built with -ffp-contract=off like tdlo_rig_host.cpp.
#include "tdlo_painter_host.h"

#include <cmath>
#include <cstring>

namespace tdlo {

static bool all_nan12(const double *T) {
    for (int q = 0; q < 12; ++q) if (!std::isnan(T[q])) return false;
    return true;
}

const char *rig_painter_fault(const double *Y, int M, const tdlo_rig_camera *cams, const double *rig_to_cam, int K, int rows, int cols, int dlo_pixel_width,
                              const double *node_dist) {
    if (!Y || !cams || !node_dist) return "rig self-occlusion: null Y / cams / node_dist";
    if (M < 1 || M > kPainterMaxNodes) return "rig self-occlusion: 1 .. 1024 nodes";
    if (K < 1 || K > kPainterMaxCams) return "rig self-occlusion: 1 .. 64 cameras";
    if (dlo_pixel_width < 1 || dlo_pixel_width > 255) return "rig self-occlusion: dlo_pixel_width 1 .. 255";
    if (rows < 1 || rows > 8192 || cols < 1 || cols > 8192) return "rig self-occlusion: rows / cols 1 .. 8192";
    for (int k = 0; k < K; ++k) {
        const tdlo_rig_camera &c = cams[k];
        if (!std::isfinite(c.fx) || !std::isfinite(c.fy) || !std::isfinite(c.cx) || !std::isfinite(c.cy)) return "rig self-occlusion: an intrinsic that is not finite";
        if (c.fx == 0 || c.fy == 0) return "rig self-occlusion: fx or fy is 0";
        if (rig_to_cam && !all_nan12(rig_to_cam + 12 * (size_t)k))
            for (int q = 0; q < 12; ++q)
                if (!std::isfinite(rig_to_cam[12 * (size_t)k + q])) return "rig self-occlusion: rig_to_cam has an entry that is not finite";
    }
    return nullptr;
}

void rig_painter_camera(const tdlo_rig_camera &cam, const double *rig_to_cam_k, PainterCam &pc) {
    pc = PainterCam{};
    pc.fx = cam.fx; pc.fy = cam.fy; pc.cx = cam.cx; pc.cy = cam.cy;
    pc.has_T = (rig_to_cam_k && !all_nan12(rig_to_cam_k)) ? 1 : 0;
    if (pc.has_T) std::memcpy(pc.T, rig_to_cam_k, sizeof pc.T);
}

void rig_painter_host(const double *Y, int M, const PainterCam *cams, int K, int rows, int cols, int dlo_pixel_width, unsigned *seen_words, unsigned *hidden_words) {
    const int W = (M + 31) / 32;
    std::vector<int> pc(M), pr(M), rank(M), order(M);
    std::vector<double> key(M);
    std::vector<unsigned char> flag(M);
    for (int k = 0; k < K; ++k)
        painter_job(cams[k], Y, M, rows, cols, dlo_pixel_width, pc.data(), pr.data(), rank.data(), order.data(), key.data(), flag.data(),
                    seen_words + (size_t)k * W, hidden_words + (size_t)k * W);
}

void rig_painter_verdict(const unsigned *seen_words, const unsigned *hidden_words, int K, int M, const double *node_dist, double visibility_threshold,
                         std::vector<int> &vis) {
    const int W = (M + 31) / 32;
    vis.clear();
    for (int m = 0; m < M; ++m) {
        if (!(node_dist[m] <= visibility_threshold)) continue;      // (a NaN distance fails, as in self_occlusion_visible)
        unsigned ok = 0u;
        for (int k = 0; k < K; ++k) ok |= seen_words[(size_t)k * W + (m >> 5)] & ~hidden_words[(size_t)k * W + (m >> 5)];
        if (ok & (1u << (m & 31))) vis.push_back(m);
    }
}

}  // namespace tdlo

extern "C" {

int tdlo_rig_self_occlusion_visible(const double *Y, int M, const tdlo_rig_camera *cams, const double *rig_to_cam, int K, int rows, int cols, int dlo_pixel_width,
                                    const double *node_dist, double visibility_threshold, int *visible_nodes, int *n_vis, unsigned *seen_words,
                                    unsigned *hidden_words) {
    if (!visible_nodes || !n_vis || tdlo::rig_painter_fault(Y, M, cams, rig_to_cam, K, rows, cols, dlo_pixel_width, node_dist)) return TDLO_E_INVALID;
    const int W = (M + 31) / 32;
    std::vector<tdlo::PainterCam> pc(K);
    for (int k = 0; k < K; ++k) tdlo::rig_painter_camera(cams[k], rig_to_cam ? rig_to_cam + 12 * (size_t)k : nullptr, pc[k]);
    std::vector<unsigned> seen((size_t)K * W), hidden((size_t)K * W);
    tdlo::rig_painter_host(Y, M, pc.data(), K, rows, cols, dlo_pixel_width, seen.data(), hidden.data());
    std::vector<int> vis;
    tdlo::rig_painter_verdict(seen.data(), hidden.data(), K, M, node_dist, visibility_threshold, vis);
    *n_vis = (int)vis.size();
    for (size_t i = 0; i < vis.size(); ++i) visible_nodes[i] = vis[i];
    if (seen_words) std::memcpy(seen_words, seen.data(), sizeof(unsigned) * seen.size());
    if (hidden_words) std::memcpy(hidden_words, hidden.data(), sizeof(unsigned) * hidden.size());
    return TDLO_OK;
}

}  // extern "C"
