// tdlo_rig_host.cpp -- the host half of a rig (tdlo_rig_to_cloud; include/trackdlo_hip.h has the contract): the argument check, a camera as the kernels'
// table holds it, and the rig's point list R formed on the host through tdlo_rig_point.h -- lane by lane over the (camera, tile) grid of the one-launch
// kernel, so that the code the GPU runs is the code that runs here.  Pure C++: no HIP, no device, so that a stand-alone program can exercise every line of
// it under a sanitizer (tests/cpp/rig_host_test.cpp); built with -ffp-contract=off like tdlo_host.cpp: the transform's products and sums are rounded one by one.
//
// THE RULE: nothing outside a plane's rows x cols elements is read (tdlo_rig_point.h's loads; the colour bytes here element by element).
#include "tdlo_rig_host.h"

#include <cmath>
#include <cstring>

namespace tdlo {

// tdlo_colour_params as the kernels take it -- the ONE statement of the rule (tdlo_api.cpp's colour_pack goes through it): bounds clamped to 0 .. 255 and
// packed H | S << 8 | V << 16, upper - lower per channel beside them; a range whose lower bound lies above its upper bound on a channel passes nothing and
// is left out.  false: no params, or not 1 .. 4 ranges
bool colour_ranges_pack(const tdlo_colour_params *p, unsigned lo_out[4], unsigned span_out[4], int *n_out, int *rgb_out) {
    *n_out = 0; *rgb_out = 0;
    for (int k = 0; k < 4; ++k) { lo_out[k] = 0u; span_out[k] = 0u; }
    if (!p || p->n_ranges < 1 || p->n_ranges > 4) return false;
    *rgb_out = p->rgb_order ? 1 : 0;
    for (int k = 0; k < p->n_ranges; ++k) {
        unsigned lo = 0, sp = 0;
        bool empty = false;
        for (int ch = 0; ch < 3; ++ch) {
            const int l = p->lower[k][ch] < 0 ? 0 : (p->lower[k][ch] > 255 ? 255 : p->lower[k][ch]);
            const int u = p->upper[k][ch] < 0 ? 0 : (p->upper[k][ch] > 255 ? 255 : p->upper[k][ch]);
            if (l > u) empty = true;
            lo |= (unsigned)l << (8 * ch); sp |= (unsigned)(u - l) << (8 * ch);
        }
        if (!empty) { lo_out[*n_out] = lo; span_out[*n_out] = sp; ++*n_out; }
    }
    return true;
}
static bool rig_colour_pack(const tdlo_colour_params *p, RigCam &rc) { return colour_ranges_pack(p, rc.lo, rc.span, &rc.n_ranges, &rc.rgb); }

bool rig_camera_colour(const tdlo_rig_camera &cam) { return cam.mask == nullptr && cam.colour != nullptr; }

const char *rig_fault(const tdlo_rig_camera *cams, int K, int rows, int cols, double leaf_size) {
    if (!cams) return "rig: no cameras";
    if (K < 1 || K > kRigMaxCams) return "rig: 1 .. 64 cameras";
    if (rows <= 0 || cols <= 0 || (long long)rows * cols > (1ll << 26)) return "bad image";
    if ((long long)K * rows * cols > (1ll << 26)) return "rig: more than 2^26 pixels over all cameras";
    const float leaf = (float)leaf_size;
    if (!(leaf_size > 0) || !(leaf > 0.0f) || !std::isfinite(leaf)) return "voxel grid: the leaf size is not a positive finite float";
    for (int k = 0; k < K; ++k) {
        const tdlo_rig_camera &cam = cams[k];
        if (!cam.depth) return "rig: a camera without a depth image";
        if (!cam.mask && !cam.colour) return "rig: a camera with neither a mask nor a colour image";
        if (rig_camera_colour(cam) != rig_camera_colour(cams[0])) return "rig: cameras segmented by mask and cameras segmented by colour in one rig";
        if (rig_camera_colour(cam)) {
            RigCam rc{};
            if (!rig_colour_pack(cam.colour_params, rc)) return "tdlo_colour_params: 1 .. 4 ranges";
        }
        if (cam.fx == 0 || cam.fy == 0) return "bad leaf size / intrinsics";
        if (cam.cam_to_rig)
            for (int q = 0; q < 12; ++q)
                if (!std::isfinite(cam.cam_to_rig[q])) return "rig: cam_to_rig has an entry that is not finite";
    }
    return nullptr;
}

void rig_camera_record(const tdlo_rig_camera &cam, RigCam &rc) {
    rc = RigCam{};
    rc.depth = cam.depth; rc.mask = cam.mask; rc.colour = cam.colour; rc.occluder = cam.occluder;
    rc.fx = cam.fx; rc.fy = cam.fy; rc.cx = cam.cx; rc.cy = cam.cy;
    rc.has_T = cam.cam_to_rig ? 1 : 0;
    if (cam.cam_to_rig) std::memcpy(rc.T, cam.cam_to_rig, sizeof rc.T);
    if (rig_camera_colour(cam)) (void)rig_colour_pack(cam.colour_params, rc);
}

// the segmentation of one pixel on the host: 8-bit BGR -> HSV by the integer routine of tdlo_cloud.hip (colour_hsv: two tables of rounded fixed-point
// quotients), the ranges as the kernels test them, the occluder byte.  tab: 512 ints, sdiv then hdiv
static void rig_colour_tables(int *tab) {
    for (int i = 0; i < 512; ++i) {
        const int k = i & 255;
        const double q = i < 256 ? (double)(255 << 12) / (1.0 * (double)k) : (double)(180 << 12) / (6.0 * (double)k);
        tab[i] = k ? (int)std::rint(q) : 0;
    }
}
static bool rig_colour_pixel(const RigCam &rc, int p, const int *tab) {
    const unsigned char *q = rc.colour + 3 * (size_t)p;
    const int b = rc.rgb ? q[2] : q[0], g = q[1], r = rc.rgb ? q[0] : q[2];
    const int v = b > g ? (b > r ? b : r) : (g > r ? g : r), vmin = b < g ? (b < r ? b : r) : (g < r ? g : r), d = v - vmin;
    const int s = (d * tab[v] + 2048) >> 12;
    int h = (v == r) ? g - b : ((v == g) ? b - r + 2 * d : r - g + 4 * d);
    h = (h * tab[256 + d] + 2048) >> 12;                                      // (arithmetic shift)
    h += h < 0 ? 180 : 0;
    bool ok = false;
    for (int k = 0; k < rc.n_ranges; ++k) {
        const unsigned lo = rc.lo[k], sp = rc.span[k];
        ok = ok || (((unsigned)h - (lo & 255u)) <= (sp & 255u) && ((unsigned)s - ((lo >> 8) & 255u)) <= ((sp >> 8) & 255u) && ((unsigned)v - (lo >> 16)) <= (sp >> 16));
    }
    return ok && (!rc.occluder || rc.occluder[p] != 0);
}

int rig_points_host(const tdlo_rig_camera *cams, int K, int rows, int cols, float *R_out, int capacity, int *n_raw_out) {
    const int P = rows * cols, Tc = (P + kRigTile - 1) / kRigTile;
    int tab[512];
    rig_colour_tables(tab);
    long long n = 0;
    for (int k = 0; k < K; ++k) {
        RigCam rc;
        rig_camera_record(cams[k], rc);
        const bool colour = rig_camera_colour(cams[k]);
        for (int bt = 0; bt < Tc; ++bt)
            for (int t = 0; t < kRigTile / 4; ++t) {                          // the lanes of the tile's workgroup
                const int p0 = bt * kRigTile + 4 * t;
                if (p0 >= P) break;
                unsigned m4 = 0u;
                if (colour) { for (int q = 0; q < 4 && p0 + q < P; ++q) if (rig_colour_pixel(rc, p0 + q, tab)) m4 |= 255u << (8 * q); }
                else m4 = rig_mask4(rc.mask, p0, P);
                float x[4], y[4], z[4];
                const unsigned keep = rig_lane4(rc, m4, p0, P, cols, x, y, z);
                for (int q = 0; q < 4; ++q)
                    if (keep & (1u << q)) {
                        if (R_out && n < capacity) { R_out[3 * n] = x[q]; R_out[3 * n + 1] = y[q]; R_out[3 * n + 2] = z[q]; }
                        ++n;
                    }
            }
    }
    if (n_raw_out) *n_raw_out = (int)n;
    return (R_out && n > capacity) ? TDLO_E_INVALID : TDLO_OK;
}

}  // namespace tdlo

extern "C" {

int tdlo_rig_check(const tdlo_rig_camera *cams, int K, int rows, int cols, double leaf_size) {
    return tdlo::rig_fault(cams, K, rows, cols, leaf_size) ? TDLO_E_INVALID : TDLO_OK;
}

int tdlo_rig_points_host(const tdlo_rig_camera *cams, int K, int rows, int cols, float *R_out, int capacity, int *n_raw_out) {
    if (tdlo::rig_fault(cams, K, rows, cols, 1.0) || capacity < 0) return TDLO_E_INVALID;
    return tdlo::rig_points_host(cams, K, rows, cols, R_out, capacity, n_raw_out);
}

}  // extern "C"
