// tdlo_image.hip -- k_image_import: a frame's images as their producer holds them in device memory (pitched or bottom-up rows, RGBA8 / BGRA8 colour,
// 32FC1 depth in metres) -> the packed canonical images the kernels behind it read (uint16 millimetre depth and the mask in cloud_ws, 3 bytes a
// pixel of colour and the occluder in col_dev): ONE launch for all of a frame's images, because every further launch on the context's stream is a
// dependent-dispatch gap of several microseconds.  Memory-bound: per pixel up to 4 + 4 + 1 bytes read, 2 + 3 + 1 written.
//
// THE RULE OF THIS FILE: no load, vector or scalar, touches a byte outside a view's extent (tdlo_image_view_extent: its rows, each from its first
// pixel's first byte to its last pixel's last byte).  A device source is the caller's allocation and carries no padding of ours -- the licence
// tdlo_cloud.hip has on the context's own padded image buffers (a 12-byte load that ends up to 9 bytes past the image) does not exist here.  A vector
// load is therefore issued only at a naturally aligned address that lies wholly inside one row of the view; everything else is loaded element by
// element (one byte, one uint16, one float -- of a 4-channel pixel the three bytes that are used).
//
// A lane takes four consecutive pixels of the canonical image -- the grain the consumers read: one mask / occluder dword, 12 colour bytes, 8 depth
// bytes -- and writes them as 1, 3 and 2 dwords (the canonical buffers are 256-byte aligned).  The lane holding the image's last 1 .. 3 pixels
// (rows x cols no multiple of 4) writes them byte by byte: the padding behind the image keeps what the copy route leaves there, i.e. is not written.
// Forms per image (image_import_form, tdlo_image_host.cpp, from data, row_stride and cols only; uniform over the launch, so a scalar branch):
//   kImgWide    cols % 4 == 0 (a lane's pixels lie in one row), data and pitch multiples of 8 (U16C1) / 16 (U8C4, F32C1): one 8- / 16-byte load
//   kImgDwords  cols % 4 == 0, data and pitch multiples of 4: 1 (U8C1), 2 (U16C1), 3 (U8C3), 4 (U8C4, F32C1) dword loads of the row's own bytes
//   kImgElem    anything else (odd widths: the four pixels may straddle rows, each has its own (row, column); misaligned data or pitch)
// Offsets are 64-bit throughout: row x row_stride passes 2^31 bytes.  The lane's code is tdlo_image_lane.h (compiled for the host as well, by a test).
#include "tdlo_internal.h"
#include "tdlo_image_lane.h"

namespace tdlo {

namespace {

__global__ __launch_bounds__(kBlock) void k_image_import(const ImageJob job) { image_import_lane(job, blockIdx.x * kBlock + threadIdx.x); }

// K images in one launch (tdlo_frame_views_to_cloud_batch): grid (blocks of an image's lanes, jobs), blockIdx.y picks the image's job out of a table in
// device memory.  A job is one image -- its up to four device sources, each in the form image_import_form chose for it (uniform over the workgroup, so
// still a scalar branch; it may differ from job to job), and the arena addresses of its canonical planes.  All jobs share P and cols.  The lane is the
// single kernel's, the rule of this file holds unchanged, and no workgroup waits for another.
__global__ __launch_bounds__(kBlock) void k_image_import_batch(const ImageJob *__restrict__ table) {
    image_import_lane(table[blockIdx.y], blockIdx.x * kBlock + threadIdx.x);
}

bool image_job_ok(const ImageJob &job) {
    if (job.P <= 0 || job.cols <= 0 || job.P % job.cols) return false;
    for (int r = 0; r < 4; ++r)
        if (job.src[r].data && (!job.dst[r] || ((uintptr_t)job.dst[r] & 7u))) return false;
    return true;
}

}  // namespace

// jobs: the table as the host wrote it (checked here), table_dev: the same bytes in device memory, uploaded by the caller on stream s before this call
hipError_t launch_image_import_batch(const ImageJob *jobs, int J, const void *table_dev, hipStream_t s) {
    if (!jobs || !table_dev || J < 1 || J > 65535) return hipErrorInvalidValue;
    for (int j = 0; j < J; ++j)
        if (!image_job_ok(jobs[j]) || jobs[j].P != jobs[0].P || jobs[j].cols != jobs[0].cols) return hipErrorInvalidValue;
    const long long lanes = ((long long)jobs[0].P + 3) / 4;
    const dim3 grid((unsigned)((lanes + kBlock - 1) / kBlock), (unsigned)J), block(kBlock);
    hipLaunchKernelGGL(k_image_import_batch, grid, block, 0, s, (const ImageJob *)table_dev);
    return hipGetLastError();
}

hipError_t launch_image_import(const ImageJob &job, hipStream_t s) {
    if (!image_job_ok(job)) return hipErrorInvalidValue;
    const long long lanes = ((long long)job.P + 3) / 4;
    const dim3 grid((unsigned)((lanes + kBlock - 1) / kBlock)), block(kBlock);
    hipLaunchKernelGGL(k_image_import, grid, block, 0, s, job);
    return hipGetLastError();
}

}  // namespace tdlo
