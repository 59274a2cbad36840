// tdlo_align_host.cpp -- the host half of depth alignment (tdlo_align_depth; include/trackdlo_hip.h has the statement): the argument check, and the aligned
// plane formed on the host through tdlo_align_lane.h -- lane by lane over the (workgroup, lane) grids of k_align_splat and k_align_pack, so that the code the
// GPU runs is the code that runs here.  Pure C++: no HIP, no device, so that a stand-alone program can exercise every line of it under a sanitizer
// (tests/cpp/align_lane_host_test.cpp); built with -ffp-contract=off like tdlo_rig_host.cpp: every product, quotient and sum is rounded on its own.
#include "tdlo_align_host.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>

namespace tdlo {

const char *align_fault(const tdlo_align_params *p) {
    if (!p) return "align: null params";
    if (p->rows_d <= 0 || p->cols_d <= 0 || (long long)p->rows_d * p->cols_d > (1ll << 26)) return "align: bad depth image shape (rows x cols must be 1 .. 2^26)";
    if (p->rows_c <= 0 || p->cols_c <= 0 || (long long)p->rows_c * p->cols_c > (1ll << 26)) return "align: bad colour image shape (rows x cols must be 1 .. 2^26)";
    const double f[4] = {p->fx_d, p->fy_d, p->fx_c, p->fy_c}, c[4] = {p->cx_d, p->cy_d, p->cx_c, p->cy_c};
    for (int i = 0; i < 4; ++i) {
        if (!std::isfinite(f[i]) || !(f[i] > 0.0)) return "align: a focal length that is not finite and positive";
        if (!std::isfinite(c[i])) return "align: a principal point that is not finite";
    }
    if (p->depth_to_colour)
        for (int q = 0; q < 12; ++q)
            if (!std::isfinite(p->depth_to_colour[q])) return "align: depth_to_colour has an entry that is not finite";
    if (p->max_footprint != 0 && (p->max_footprint < 1 || p->max_footprint > kAlignMaxFootprintLimit)) return "align: max_footprint must be 0 (16) or 1 .. 64";
    return nullptr;
}

void align_job(const tdlo_image_view *depth, const tdlo_align_params *p, AlignJob &job) {
    job = AlignJob{};
    job.depth = (const unsigned char *)depth->data; job.row_stride = depth->row_stride; job.format = depth->format;
    job.rows_d = p->rows_d; job.cols_d = p->cols_d; job.rows_c = p->rows_c; job.cols_c = p->cols_c;
    job.has_T = p->depth_to_colour ? 1 : 0;
    job.max_fp = p->max_footprint ? p->max_footprint : kAlignMaxFootprintDefault;
    job.fx_d = p->fx_d; job.fy_d = p->fy_d; job.cx_d = p->cx_d; job.cy_d = p->cy_d;
    job.fx_c = p->fx_c; job.fy_c = p->fy_c; job.cx_c = p->cx_c; job.cy_c = p->cy_c;
    if (p->depth_to_colour) std::memcpy(job.T, p->depth_to_colour, sizeof job.T);
}

void align_depth_host(const AlignJob &job, unsigned *scratch, unsigned short *aligned_out, long long counts[4]) {
    const int Pd = job.rows_d * job.cols_d, Pc = job.rows_c * job.cols_c, block = 256;
    for (int i = 0; i < Pc; ++i) scratch[i] = kAlignEmpty;
    long long n[4] = {0, 0, 0, 0};
    for (int b = 0; b < (Pd + block - 1) / block; ++b)
        for (int t = 0; t < block; ++t) {                                  // the lanes of the workgroup, those of a partly filled last one included
            const int verdict = align_splat_lane(job, b * block + t, [scratch](int i, unsigned k) { if (k < scratch[i]) scratch[i] = k; });
            if (verdict != kAlignZero) { ++n[0]; ++n[verdict]; }
        }
    const int lanes = (Pc + 3) / 4;
    for (int b = 0; b < (lanes + block - 1) / block; ++b)
        for (int t = 0; t < block; ++t) align_pack_lane(scratch, aligned_out, Pc, b * block + t);
    if (counts) std::memcpy(counts, n, sizeof n);
}

}  // namespace tdlo

extern "C" {

int tdlo_align_check(const tdlo_align_params *p) { return tdlo::align_fault(p) ? TDLO_E_INVALID : TDLO_OK; }

int tdlo_align_depth_host(const tdlo_image_view *depth, const tdlo_align_params *p, unsigned short *aligned_out, long long counts[4]) {
    if (!aligned_out || tdlo::align_fault(p) || tdlo::image_view_fault(depth, p->rows_d, p->cols_d, tdlo::kRoleDepth)) return TDLO_E_INVALID;
    const size_t Pc = (size_t)p->rows_c * p->cols_c;
    // the scratch plane at exactly its extent, 16-byte aligned (the pack's 16-byte access); the output may be aligned to 2 bytes only, so the pack writes a
    // plane of its own alignment when it is not
    unsigned *scratch = static_cast<unsigned *>(::operator new(Pc * sizeof(unsigned), std::align_val_t(16), std::nothrow));
    if (!scratch) return TDLO_E_INVALID;
    unsigned short *plane = aligned_out;
    if ((uintptr_t)aligned_out % 8) {
        plane = static_cast<unsigned short *>(::operator new(Pc * sizeof(unsigned short), std::align_val_t(16), std::nothrow));
        if (!plane) { ::operator delete(scratch, std::align_val_t(16)); return TDLO_E_INVALID; }
    }
    tdlo::AlignJob job;
    tdlo::align_job(depth, p, job);
    tdlo::align_depth_host(job, scratch, plane, counts);
    if (plane != aligned_out) { std::memcpy(aligned_out, plane, Pc * sizeof(unsigned short)); ::operator delete(plane, std::align_val_t(16)); }
    ::operator delete(scratch, std::align_val_t(16));
    return TDLO_OK;
}

}  // extern "C"
