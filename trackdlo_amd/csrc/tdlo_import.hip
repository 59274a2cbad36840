// tdlo_import.hip -- k_cloud_import: a cloud as its producer holds it (float32 or float64, any strides) -> the slot's resident cloud
// (Slot::Xraw: N x 3 column-major doubles).  Component c of point n is read from src + n * stride_point + c * stride_comp (elements) and written
// to Xraw[c * N + n] = (double)value.  Element-wise and memory-bound: 12 + 24 algorithmic bytes per point for packed float32.
//
// THE RULE OF THIS FILE: no load, vector or scalar, touches a byte outside the view's extent (tdlo_cloud_view_extent).  A device source is the
// caller's allocation and carries no padding of ours -- the licence tdlo_cloud.hip's colour path has on our own padded image buffers (up to 9 bytes
// past the image) does not exist here.  Every form below therefore loads whole elements of the view and nothing else: a lane's vector covers
// elements the view addresses, or the lane loads element by element.
//
// Forms (chosen from the strides and the alignment of `data` only, cloud_import_form):
//   kGeneric   any strides, float32 / float64: three scalar loads per point (a float64 scalar is an 8-byte load already).
//   kXyz12     float32, stride_comp == 1, stride_point in {3, 4, 8}: ONE 12-byte load per point (x, y, z are adjacent; 4-byte alignment is all a
//              global 12-byte load needs) -- exactly the point's three elements, so neither heads, tails nor the unused lanes of a padded point
//              (PointXYZ's fourth float, PointXYZRGB's rgb + padding) are ever read.
//              (A 16-byte load of a whole padded point from 16-byte aligned data was tried as a form of its own: the compiler drops the unused
//              fourth lane and emits the same 12-byte load, so there is one form.)
//   kCols2     float32, stride_point == 1 (column-major), stride_comp even, data 8-byte aligned: a lane takes two consecutive points, one aligned
//              8-byte load per column; an odd last point is loaded element by element.
// Stores: a lane writes its point's three doubles to the three output columns -- consecutive lanes, consecutive addresses (kCols2: pairs).
// Offsets are 64-bit throughout: n * stride_point may pass 2^31 elements, 3 N doubles pass 2^32 bytes at N = 2^28.
#include "tdlo_internal.h"
#include "tdlo_view_load.h"      // the loaders and the forms' definitions: shared with the voxel grid's view source (tdlo_cloud.hip)

namespace tdlo {

namespace {

// what lane i of a frame does: the frame's point i (kCols2: its points 2 i and 2 i + 1); a lane beyond the frame's points does nothing
template <typename T, int FORM>
__device__ __forceinline__ void cloud_import_lane(const T *__restrict__ src, long long sp, long long sc, int N, double *__restrict__ X, long long i) {
    const size_t ld = (size_t)N;
    if constexpr (FORM == kCols2) {
        const long long n = 2 * i;
        if (n >= N) return;
        if (n + 1 < N) {
            float2 a, b, c;
            view_load_pair(src, sc, n, a, b, c);
            X[n] = (double)a.x; X[n + 1] = (double)a.y;
            X[ld + n] = (double)b.x; X[ld + n + 1] = (double)b.y;
            X[2 * ld + n] = (double)c.x; X[2 * ld + n + 1] = (double)c.y;
        } else {
            T x, y, z;
            view_load_point<T, kGeneric>(src, 1, sc, n, x, y, z);
            X[n] = (double)x; X[ld + n] = (double)y; X[2 * ld + n] = (double)z;
        }
    } else {
        if (i >= N) return;
        T x, y, z;
        view_load_point<T, FORM>(src, sp, sc, i, x, y, z);
        X[i] = (double)x; X[ld + i] = (double)y; X[2 * ld + i] = (double)z;
    }
}

template <typename T, int FORM>
__global__ __launch_bounds__(kBlock) void k_cloud_import(const T *__restrict__ src, long long sp, long long sc, int N, double *__restrict__ X) {
    cloud_import_lane<T, FORM>(src, sp, sc, N, X, (long long)blockIdx.x * kBlock + threadIdx.x);
}

// F views in one launch (tdlo_set_cloud_view_batch): grid (blocks of the frame with the most lanes, F), blockIdx.y picks the frame's record out of a table in
// device memory.  The same lane behind a switch on the frame's form (the same for every thread of the block); a block beyond its frame's lanes leaves.
// THE RULE holds unchanged: the loaders are the single kernel's, and a lane loads nothing but elements of its own frame's view.
__global__ __launch_bounds__(kBlock) void k_cloud_import_batch(const ImportBatchFrame *__restrict__ table) {
    const ImportBatchFrame f = table[blockIdx.y];
    const long long lanes = f.form == 2 ? ((long long)f.N + 1) / 2 : (long long)f.N;
    const long long i0 = (long long)blockIdx.x * kBlock;
    if (i0 >= lanes) return;
    const long long i = i0 + threadIdx.x;
    switch (f.form) {
    case 0: cloud_import_lane<double, kGeneric>((const double *)f.src, f.sp, f.sc, f.N, f.X, i); break;
    case 1: cloud_import_lane<float, kXyz12>((const float *)f.src, f.sp, f.sc, f.N, f.X, i); break;
    case 2: cloud_import_lane<float, kCols2>((const float *)f.src, f.sp, f.sc, f.N, f.X, i); break;
    default: cloud_import_lane<float, kGeneric>((const float *)f.src, f.sp, f.sc, f.N, f.X, i); break;
    }
}

}  // namespace

int cloud_import_form(const void *src, bool f64, long long sp, long long sc) {
    if (f64) return kGeneric;
    const uintptr_t a = (uintptr_t)src;
    if (sc == 1 && (sp == 3 || sp == 4 || sp == 8)) return kXyz12;
    if (sp == 1 && sc % 2 == 0 && a % 8 == 0) return kCols2;
    return kGeneric;
}

hipError_t launch_cloud_import(const void *src, bool f64, long long sp, long long sc, int N, double *Xraw, hipStream_t s) {
    if (N <= 0) return hipErrorInvalidValue;
    const int form = cloud_import_form(src, f64, sp, sc);
    const long long lanes = form == kCols2 ? ((long long)N + 1) / 2 : (long long)N;
    const dim3 grid((unsigned)((lanes + kBlock - 1) / kBlock)), block(kBlock);
    const float *f = (const float *)src;
    if (f64) hipLaunchKernelGGL((k_cloud_import<double, kGeneric>), grid, block, 0, s, (const double *)src, sp, sc, N, Xraw);
    else if (form == kXyz12) hipLaunchKernelGGL((k_cloud_import<float, kXyz12>), grid, block, 0, s, f, sp, sc, N, Xraw);
    else if (form == kCols2) hipLaunchKernelGGL((k_cloud_import<float, kCols2>), grid, block, 0, s, f, sp, sc, N, Xraw);
    else hipLaunchKernelGGL((k_cloud_import<float, kGeneric>), grid, block, 0, s, f, sp, sc, N, Xraw);
    return hipGetLastError();
}

hipError_t launch_cloud_import_batch(const ImportBatchFrame *frames, const bool *f64, int F, void *table_pinned, void *table_dev, hipStream_t s) {
    if (F < 1) return hipErrorInvalidValue;
    ImportBatchFrame *tab = (ImportBatchFrame *)table_pinned;
    long long most = 0;
    for (int f = 0; f < F; ++f) {
        if (frames[f].N <= 0) return hipErrorInvalidValue;
        tab[f] = frames[f];
        const int form = cloud_import_form(frames[f].src, f64[f], frames[f].sp, frames[f].sc);
        tab[f].form = f64[f] ? 0 : (form == kXyz12 ? 1 : (form == kCols2 ? 2 : 3));
        const long long lanes = tab[f].form == 2 ? ((long long)frames[f].N + 1) / 2 : (long long)frames[f].N;
        most = lanes > most ? lanes : most;
    }
    if (const hipError_t e = hipMemcpyAsync(table_dev, tab, sizeof(ImportBatchFrame) * (size_t)F, hipMemcpyHostToDevice, s)) return e;
    hipLaunchKernelGGL(k_cloud_import_batch, dim3((unsigned)((most + kBlock - 1) / kBlock), (unsigned)F), dim3(kBlock), 0, s, (const ImportBatchFrame *)table_dev);
    return hipGetLastError();
}

}  // namespace tdlo
