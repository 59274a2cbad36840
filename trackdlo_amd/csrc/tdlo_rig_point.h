// tdlo_rig_point.h -- one camera of a rig, and what one lane of the one-launch kernel's phase A does when the points come from a rig's images
// (k_cloud_team's rig instantiations, tdlo_cloud.hip): its four consecutive pixels p0 .. p0 + 3 of ONE camera (p0 a multiple of 4) -- the mask bytes, the
// depth loads, the back-projection in double, the camera -> rig transform without a fused multiply-add, the rounding to float and the finiteness test.
// A header of its own, like tdlo_view_lane.h, so that the very code the GPU runs can be compiled for the host (tdlo_rig_host.cpp: tdlo_rig_points_host)
// and run lane by lane under a sanitizer on planes allocated at exactly their extents (tests/cpp/rig_host_test.cpp).
//
// THE ARITHMETIC (include/trackdlo_hip.h, the rig contract): pixel (i, j) of a camera, depth d millimetres,
//   zd = d / 1000.0,  xd = ((double)j - cx) * zd / fx,  yd = ((double)i - cy) * zd / fy              (trackdlo_node.cpp:219-224 before the store as float)
//   no transform:  ((float)xd, (float)yd, (float)zd)                                                 -- the single call's bits
//   transform T = [A | b], 3 x 4 row-major:  component r = (float)(((A[r][0] xd + A[r][1] yd) + A[r][2] zd) + b[r]), every product and sum rounded to
//   double on its own, in this order.  tdlo_cloud.hip is built with contraction allowed: the products and sums are plain operators under
//   `#pragma clang fp contract(off)` (host and device passes of clang); the g++ unit that includes this header is built with -ffp-contract=off.
// A point whose three floats are not all finite is dropped.
// THE LOADS touch nothing outside a plane of P pixels: a 4-byte mask word / an 8-byte depth word where the lane's four pixels lie wholly inside the plane
// (the planes are 8-byte aligned: the arena's, or an allocation's), else element by element.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TDLO_RIG __host__ __device__ __forceinline__
#else
#define TDLO_RIG inline
#endif
#if defined(__clang__)
#define TDLO_RIG_UNROLL _Pragma("unroll")
#else
#define TDLO_RIG_UNROLL
#endif

namespace tdlo {

constexpr int kRigMaxCams = 64;          // cameras of a rig
constexpr int kRigTile = 4096;           // pixels of a phase-A tile (tdlo_cloud.hip: kFPix)

// one record of the camera table (device memory; the kernel fetches its tile's record, workgroup-uniform).  mask: the camera's mask plane -- for a colour rig
// the plane k_colour_mask fills when the rig takes the multi-launch form; lo / span / n_ranges / rgb: the camera's colour ranges as CloudColour packs them
struct RigCam {
    const unsigned short *depth; const unsigned char *mask, *colour, *occluder;
    double fx, fy, cx, cy;
    double T[12];
    unsigned lo[4], span[4];
    int n_ranges, rgb, has_T, pad_;
};

TDLO_RIG bool rig_finite(float v) { unsigned u; __builtin_memcpy(&u, &v, 4); return (u & 0x7f800000u) != 0x7f800000u; }

// one product / one sum rounded to double on its own.  Plain operators under the contraction pragma, on the device as on the host (tdlo_lle_dev.h, tdlo_init.hip
// do the same): this toolchain's __dmul_rn / __dadd_rn are plain operators compiled WITHOUT the pragma, which the backend fuses after inlining
TDLO_RIG double rig_mul(double a, double b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return a * b;
}
TDLO_RIG double rig_add(double a, double b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return a + b;
}

// pixel (i, j) with depth d of camera c: its point in the rig's frame; false: not all three floats are finite (the point is dropped)
TDLO_RIG bool rig_point(const RigCam &c, int i, int j, unsigned d, float &x, float &y, float &z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double zd = (double)d / 1000.0;
    const double xd = ((double)j - c.cx) * zd / c.fx;
    const double yd = ((double)i - c.cy) * zd / c.fy;
    if (!c.has_T) { x = (float)xd; y = (float)yd; z = (float)zd; }
    else {
        x = (float)rig_add(rig_add(rig_add(rig_mul(c.T[0], xd), rig_mul(c.T[1], yd)), rig_mul(c.T[2], zd)), c.T[3]);
        y = (float)rig_add(rig_add(rig_add(rig_mul(c.T[4], xd), rig_mul(c.T[5], yd)), rig_mul(c.T[6], zd)), c.T[7]);
        z = (float)rig_add(rig_add(rig_add(rig_mul(c.T[8], xd), rig_mul(c.T[9], yd)), rig_mul(c.T[10], zd)), c.T[11]);
    }
    return rig_finite(x) && rig_finite(y) && rig_finite(z);
}

// the mask bytes of pixels p0 .. p0 + 3, little endian, 0 for a pixel at or beyond P
TDLO_RIG unsigned rig_mask4(const unsigned char *mask, int p0, int P) {
    if (p0 >= P) return 0u;
    const unsigned char *q = mask + p0;
    if (p0 + 4 <= P && ((uintptr_t)q & 3u) == 0u) return *reinterpret_cast<const unsigned *>(q);
    unsigned m = 0u;
TDLO_RIG_UNROLL
    for (int k = 0; k < 4; ++k)
        if (p0 + k < P) m |= (unsigned)q[k] << (8 * k);
    return m;
}

// m4: the mask word of pixels p0 .. p0 + 3 (a byte per pixel; bytes of pixels at or beyond P do not count).  Bit k of the result: pixel p0 + k is kept --
// its byte is set and its point is finite -- and x[k], y[k], z[k] are its floats (what the arrays hold for the other pixels is not to be used)
TDLO_RIG unsigned rig_lane4(const RigCam &c, unsigned m4, int p0, int P, int cols, float x[4], float y[4], float z[4]) {
TDLO_RIG_UNROLL
    for (int k = 0; k < 4; ++k) { x[k] = 0.0f; y[k] = 0.0f; z[k] = 0.0f; }
    if (p0 >= P) return 0u;
    if (p0 + 4 > P) m4 &= 0xffffffffu >> (8 * (4 - (P - p0)));
    if (m4 == 0u) return 0u;
    const unsigned short *dq = c.depth + p0;
    unsigned d[4] = {0u, 0u, 0u, 0u};
    if (p0 + 4 <= P && ((uintptr_t)dq & 7u) == 0u) {
        const unsigned long long w = *reinterpret_cast<const unsigned long long *>(dq);
        d[0] = (unsigned)(w & 0xffffu); d[1] = (unsigned)((w >> 16) & 0xffffu); d[2] = (unsigned)((w >> 32) & 0xffffu); d[3] = (unsigned)(w >> 48);
    } else {
TDLO_RIG_UNROLL
        for (int k = 0; k < 4; ++k)
            if (p0 + k < P && ((m4 >> (8 * k)) & 255u)) d[k] = dq[k];
    }
    int i = p0 / cols, j = p0 - i * cols;
    unsigned keep = 0u;
TDLO_RIG_UNROLL
    for (int k = 0; k < 4; ++k) {
        if (((m4 >> (8 * k)) & 255u) && rig_point(c, i, j, d[k], x[k], y[k], z[k])) keep |= 1u << k;
        if (++j == cols) { j = 0; ++i; }
    }
    return keep;
}

}  // namespace tdlo
