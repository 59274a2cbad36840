// tdlo_view_load.h -- the loads that read a cloud view (tdlo_cloud_view) on the device, shared by k_cloud_import (tdlo_import.hip) and the voxel
// grid's view source (tdlo_cloud.hip).
//
// THE RULE: no load, vector or scalar, touches a byte outside the view's extent (tdlo_cloud_view_extent).  Every loader below loads whole elements
// that the view addresses and nothing else; the forms are chosen on the host (cloud_import_form) from the strides and the alignment of `data` only.
//   kGeneric   any strides, float32 / float64: three scalar loads per point (a float64 scalar is an 8-byte load already).
//   kXyz12     float32, stride_comp == 1, stride_point in {3, 4, 8}: ONE 12-byte load per point (x, y, z are adjacent; 4-byte alignment is all a
//              global 12-byte load needs) -- exactly the point's three elements, so neither heads, tails nor the unused lanes of a padded point
//              (PointXYZ's fourth float, PointXYZRGB's rgb + padding) are ever read.
//   kCols2     float32, stride_point == 1 (column-major), stride_comp even, data 8-byte aligned: two consecutive points (n even, n + 1 < N) by one
//              aligned 8-byte load per column.
// Offsets are 64-bit throughout: n * stride_point may pass 2^31 elements.
// (The forms and the 12-byte point are plain C++, so that tdlo_view_lane.h -- a lane of the one-launch kernel's phase A over a view -- compiles for the host.)
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace tdlo {

enum ImportForm { kGeneric = 0, kXyz12 = 1, kCols2 = 2 };

struct __attribute__((packed, aligned(4))) Xyz12 { float x, y, z; };

#if defined(__HIPCC__)

// point n of the view, element by element or (kXyz12) by its one 12-byte load; kCols2 reads a single point element by element
template <typename T, int FORM>
__device__ __forceinline__ void view_load_point(const T *__restrict__ src, long long sp, long long sc, long long n, T &x, T &y, T &z) {
    const T *p = src + n * sp;
    if constexpr (FORM == kXyz12) {
        const Xyz12 v = *reinterpret_cast<const Xyz12 *>(p); x = v.x; y = v.y; z = v.z;
    } else {
        x = p[0]; y = p[sc]; z = p[2 * sc];
    }
}

// kCols2: points n and n + 1 (n even, n + 1 < N: both are the view's) -- .x of each pair is point n's component, .y point n + 1's
__device__ __forceinline__ void view_load_pair(const float *__restrict__ src, long long sc, long long n, float2 &a, float2 &b, float2 &c) {
    const float *p = src + n;
    a = *reinterpret_cast<const float2 *>(p); b = *reinterpret_cast<const float2 *>(p + sc); c = *reinterpret_cast<const float2 *>(p + 2 * sc);
}
#endif

}  // namespace tdlo
