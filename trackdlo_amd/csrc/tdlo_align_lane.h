// tdlo_align_lane.h -- depth aligned to the colour camera (tdlo_align_depth; include/trackdlo_hip.h has the statement): the ONE text of the per-pixel
// steps for the host statement (tdlo_align_host.cpp) and for the kernels (tdlo_align.hip) -- the depth load by format and pitch, the two corners, the
// decision, the footprint loop over "offer k to word i", and the pack of the 32-bit scratch plane into the uint16 plane.  Both sides are built with
// -ffp-contract=off and without fast-math flags: every product, quotient and sum below is rounded on its own, the quotients are IEEE divisions, and a
// compiler that fused one multiply-add would move a corner that lies within one rounding of k + 1/2 to the next pixel.
//
// THE RULES: no load touches a byte outside the depth view's extent (element loads only: one uint16 or one float); no word outside the
// rows_c x cols_c scratch plane is offered to (the decision drops a footprint that is not wholly inside before the loop runs); the pack's one 16-byte
// access per lane lies wholly inside the plane, its last 1 .. 3 words go element by element.
#pragma once
#include "tdlo_image.h"

namespace tdlo {

constexpr unsigned kAlignEmpty = 0xffffffffu;        // a scratch word nobody has offered to
constexpr int kAlignMaxFootprintDefault = 16, kAlignMaxFootprintLimit = 64;
enum AlignVerdict { kAlignZero = 0, kAlignUsed = 1, kAlignDropped = 2, kAlignWide = 3 };

// tdlo_align_params and the depth view as a lane takes them (align_job, tdlo_align_host.cpp)
struct AlignJob {
    const unsigned char *depth;      // pixel (0, 0) of the depth view
    long long row_stride;            // bytes, signed
    int format;                      // TDLO_IMG_U16C1 / TDLO_IMG_F32C1
    int rows_d, cols_d, rows_c, cols_c;
    int has_T, max_fp;               // max_fp: 1 .. 64 (0 already replaced by 16)
    double fx_d, fy_d, cx_d, cy_d, fx_c, fy_c, cx_c, cy_c;
    double T[12];
};

struct alignas(16) AlignU4 { unsigned x, y, z, w; };
struct alignas(8) AlignU2 { unsigned x, y; };

// k = D[v, u] in millimetres: one element load at data + v x row_stride + u x element size
TDLO_HD inline unsigned align_load_k(const AlignJob &j, int v, int u) {
    const unsigned char *q = j.depth + (long long)v * j.row_stride + (long long)u * (j.format == TDLO_IMG_F32C1 ? 4 : 2);
    if (j.format == TDLO_IMG_F32C1) { float d; __builtin_memcpy(&d, q, 4); return (unsigned)image_f32_to_mm(d); }
    unsigned short k; __builtin_memcpy(&k, q, 2);
    return k;
}

// One corner (uu, vv) = (u + s, v + s) of a depth pixel at z metres -> the colour pixel (X, Y) it lands on.  false: the corner is bad
TDLO_HD inline bool align_corner(const AlignJob &j, double uu, double vv, double z, int *X, int *Y) {
    const double x = ((uu - j.cx_d) / j.fx_d) * z, y = ((vv - j.cy_d) / j.fy_d) * z;
    double qx = x, qy = y, qz = z;
    if (j.has_T) {
        const double *T = j.T;
        qx = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
        qy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
        qz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
    }
    if (!(qz > 0.0) || !__builtin_isfinite(qx) || !__builtin_isfinite(qy) || !__builtin_isfinite(qz)) return false;
    const double px = (qx / qz) * j.fx_c + j.cx_c, py = (qy / qz) * j.fy_c + j.cy_c;
    const double lim = 1073741824.0;                                      // 2^30: floor(p + 1/2) fits an int (NaN fails the comparison)
    if (!(__builtin_fabs(px) < lim) || !(__builtin_fabs(py) < lim)) return false;
    *X = (int)__builtin_floor(px + 0.5);                                  // floor, not truncation: -1.5 < px < -0.5 lands on -1, outside
    *Y = (int)__builtin_floor(py + 0.5);
    return true;
}

// The decision for depth pixel (u, v) holding k != 0, in the statement's order: dropped, wide, used.  r = {x0, y0, x1, y1} when used
TDLO_HD inline int align_decide(const AlignJob &j, int u, int v, unsigned k, int r[4]) {
    const double z = (double)k / 1000.0;
    int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    const bool ok0 = align_corner(j, (double)u + -0.5, (double)v + -0.5, z, &x0, &y0);
    const bool ok1 = align_corner(j, (double)u + 0.5, (double)v + 0.5, z, &x1, &y1);
    if (!ok0 || !ok1) return kAlignDropped;
    if (x0 < 0 || y0 < 0 || x1 >= j.cols_c || y1 >= j.rows_c || x1 < x0 || y1 < y0) return kAlignDropped;      // never clipped
    if (x1 - x0 + 1 > j.max_fp || y1 - y0 + 1 > j.max_fp) return kAlignWide;
    r[0] = x0; r[1] = y0; r[2] = x1; r[3] = y1;
    return kAlignUsed;
}

// lane g of the splat: depth pixel g = v x cols_d + u (a wave's lanes are consecutive in u).  offer(i, k): "k is offered to word i of the scratch plane"
template <class Offer>
TDLO_HD inline int align_splat_lane(const AlignJob &j, int g, Offer offer) {
    if (g >= j.rows_d * j.cols_d) return kAlignZero;
    const int v = g / j.cols_d, u = g - v * j.cols_d;
    const unsigned k = align_load_k(j, v, u);
    if (k == 0u) return kAlignZero;
    int r[4];
    const int verdict = align_decide(j, u, v, k, r);
    if (verdict == kAlignUsed)
        for (int y = r[1]; y <= r[3]; ++y)
            for (int x = r[0]; x <= r[2]; ++x) offer(y * j.cols_c + x, k);
    return verdict;
}

// lane t of the pack: words 4 t .. 4 t + 3 of the scratch plane (P words, 16-byte aligned) -> uint16 (kAlignEmpty -> 0) at out (8-byte aligned), and the
// words read are armed again for the next call
TDLO_HD inline void align_pack_lane(unsigned *scratch, unsigned short *out, int P, int t) {
    if (t >= (P + 3) / 4) return;                                         // (before 4 t: a spare lane's 4 t could pass 2^31)
    const int p0 = 4 * t;
    if (p0 + 4 <= P) {
        AlignU4 w;                                                        // (memcpy at a stated alignment: one 16-byte access, no aliasing question on the host)
        __builtin_memcpy(&w, __builtin_assume_aligned(scratch + p0, 16), 16);
        const unsigned a = w.x == kAlignEmpty ? 0u : w.x, b = w.y == kAlignEmpty ? 0u : w.y, c = w.z == kAlignEmpty ? 0u : w.z, d = w.w == kAlignEmpty ? 0u : w.w;
        const AlignU2 o{a | (b << 16), c | (d << 16)};
        const AlignU4 e{kAlignEmpty, kAlignEmpty, kAlignEmpty, kAlignEmpty};
        __builtin_memcpy(__builtin_assume_aligned(out + p0, 8), &o, 8);
        __builtin_memcpy(__builtin_assume_aligned(scratch + p0, 16), &e, 16);
        return;
    }
    for (int p = p0; p < P; ++p) {                                        // the plane's last 1 .. 3 words
        const unsigned w = scratch[p];
        out[p] = (unsigned short)(w == kAlignEmpty ? 0u : w);
        scratch[p] = kAlignEmpty;
    }
}

}  // namespace tdlo
