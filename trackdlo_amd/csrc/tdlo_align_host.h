// tdlo_align_host.h -- the host half of depth alignment (tdlo_align_host.cpp, no HIP): the argument check, the job a lane takes, the statement on the host.
#pragma once
#include "tdlo_align_lane.h"

namespace tdlo {

// nullptr: p describes two cameras; otherwise what is wrong with it
const char *align_fault(const tdlo_align_params *p);
// a checked (depth view, params) as a lane takes it
void align_job(const tdlo_image_view *depth, const tdlo_align_params *p, AlignJob &job);
// the statement, lane by lane over the kernels' (workgroup, lane) grids: scratch = rows_c x cols_c words (filled here), aligned_out the packed plane
void align_depth_host(const AlignJob &job, unsigned *scratch, unsigned short *aligned_out, long long counts[4]);

}  // namespace tdlo
