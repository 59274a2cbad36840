// tdlo_view_lane.h -- what one lane of the one-launch kernel's phase A does when the points come from a cloud view (k_cloud_team's view instantiations,
// tdlo_cloud.hip): its four consecutive elements p0 .. p0 + 3 (p0 a multiple of 4) -- the selection test, the loads in the form the host chose, the
// conversion to float and the finiteness test.  A header of its own, like tdlo_image_lane.h, so that the very code the GPU runs can be compiled for the
// host and run lane by lane under a sanitizer on buffers allocated at exactly their extents (tests/cpp/view_lane_host_test.cpp).
//
// THE RULE is tdlo_view_load.h's: no load of any width touches a byte outside the view's extent (tdlo_cloud_view_extent), nor outside [select, select + N).
//   selection   a caller's device pointer has neither alignment nor padding: ONE 4-byte load where the lane's four bytes lie at a 4-aligned address
//               wholly inside [select, select + N), else byte by byte (the last lane of the view; every lane of a pointer that is not 4-aligned).
//   kXyz12 / kGeneric   an element is loaded only where its selection byte is set.
//   kCols2      the lane's elements are the pairs (p0, p0 + 1) and (p0 + 2, p0 + 3), each at an 8-aligned address (data 8-aligned, stride_comp even,
//               p0 a multiple of 4): a pair with a selected element is loaded by one 8-byte load per column when its second element is below N, else
//               its first element alone, element by element.
// An element is KEPT iff it is below N, its selection byte is not 0 (select == nullptr: every element is selected) and its three floats are finite after
// the (float) conversion (a double beyond float range has become +-inf) -- ViewSrc::fetch's rule, rule 2 of include/trackdlo_hip.h.
#pragma once
#include <stdint.h>
#include "tdlo_view_load.h"

#if defined(__HIPCC__)
#define TDLO_LANE __host__ __device__ __forceinline__
#else
#define TDLO_LANE inline
#endif

namespace tdlo {

struct alignas(8) ViewF2 { float x, y; };                    // one aligned 8-byte access

TDLO_LANE bool view_finite(float v) { unsigned u; __builtin_memcpy(&u, &v, 4); return (u & 0x7f800000u) != 0x7f800000u; }

// the selection bytes of elements p0 .. p0 + 3, little endian, 0 for an element at or beyond N
TDLO_LANE unsigned view_select4(const unsigned char *sel, int p0, int N) {
    if (p0 >= N) return 0u;
    const int left = N - p0;
    if (!sel) return left >= 4 ? 0x01010101u : (0x01010101u >> (8 * (4 - left)));
    const unsigned char *q = sel + p0;
    if (left >= 4 && ((uintptr_t)q & 3u) == 0u) return *reinterpret_cast<const unsigned *>(q);
    unsigned m = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < left) m |= (unsigned)q[k] << (8 * k);
    return m;
}

// bit k of the result: element p0 + k is kept, and x[k], y[k], z[k] are its floats (what the arrays hold for the other elements is not to be used)
template <typename T, int FORM>
TDLO_LANE unsigned view_lane4(const T *src, long long sp, long long sc, const unsigned char *sel, int p0, int N, float x[4], float y[4], float z[4]) {
    const unsigned m4 = view_select4(sel, p0, N);
#pragma unroll
    for (int k = 0; k < 4; ++k) { x[k] = 0.0f; y[k] = 0.0f; z[k] = 0.0f; }
    if (m4 == 0u) return 0u;
    if constexpr (FORM == kCols2) {
        const T *p = src + p0;
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if ((m4 >> (16 * h)) & 0xffffu) {                // (a set byte: the pair's first element is below N)
                const T *q = p + 2 * h;
                if (p0 + 2 * h + 1 < N) {
                    const ViewF2 a = *reinterpret_cast<const ViewF2 *>(q), b = *reinterpret_cast<const ViewF2 *>(q + sc), c = *reinterpret_cast<const ViewF2 *>(q + 2 * sc);
                    x[2 * h] = a.x; x[2 * h + 1] = a.y; y[2 * h] = b.x; y[2 * h + 1] = b.y; z[2 * h] = c.x; z[2 * h + 1] = c.y;
                } else { x[2 * h] = q[0]; y[2 * h] = q[sc]; z[2 * h] = q[2 * sc]; }
            }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((m4 >> (8 * k)) & 255u) {
                const T *q = src + (long long)(p0 + k) * sp;
                if constexpr (FORM == kXyz12) { const Xyz12 v = *reinterpret_cast<const Xyz12 *>(q); x[k] = v.x; y[k] = v.y; z[k] = v.z; }
                else { x[k] = (float)q[0]; y[k] = (float)q[sc]; z[k] = (float)q[2 * sc]; }
            }
    }
    unsigned keep = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (((m4 >> (8 * k)) & 255u) && view_finite(x[k]) && view_finite(y[k]) && view_finite(z[k])) keep |= 1u << k;
    return keep;
}

}  // namespace tdlo
