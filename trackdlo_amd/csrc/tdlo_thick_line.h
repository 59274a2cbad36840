// tdlo_thick_line.h -- the library's ONE statement of "this pixel lies under a thick line", for the host (the self-occlusion test, tdlo_host.cpp) and the
// device (the result image, tdlo_render.hip).
#pragma once

#if defined(__HIPCC__)
#define TDLO_HD __host__ __device__
#else
#define TDLO_HD
#endif

namespace tdlo {

struct Px { long long c, r; };

// The geometric content of cv::line with a thickness w: pixel p is covered when it lies within w / 2 of the segment between the end pixels a and b, in
// exact integer arithmetic.  OpenCV's own fixed-point rasteriser is not available to pin the boundary pixels against: PARITY UNPINNED.
// The result image keeps every coordinate in [-8192, 8191] (render_primitives refuses anything else, and images beyond 8192 x 8192) and w <= 255:
// differences < 2^14, len2 and |along| < 2^29, |area| < 2^29, 4 area^2 < 2^60, w^2 len2 < 2^45 -- every product fits int64.
TDLO_HD inline bool within_half_width(const Px &p, const Px &a, const Px &b, long long w) {
    const long long ex = b.c - a.c, ey = b.r - a.r, fx = p.c - a.c, fy = p.r - a.r;
    const long long len2 = ex * ex + ey * ey, along = fx * ex + fy * ey;
    if (along <= 0 || len2 == 0) return 4 * (fx * fx + fy * fy) <= w * w;                 // in front of the first end pixel (or a zero-length edge): its cap
    if (along >= len2) { const long long gx = p.c - b.c, gy = p.r - b.r; return 4 * (gx * gx + gy * gy) <= w * w; }
    const long long area = fx * ey - fy * ex;                                               // twice the triangle's area: distance = |area| / len
    return 4 * area * area <= w * w * len2;
}

}  // namespace tdlo
