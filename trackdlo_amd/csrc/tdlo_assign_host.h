// tdlo_assign_host.h -- the host half of "one cloud dealt out among F ropes" (tdlo_assign_host.cpp; no HIP): what the driver and a stand-alone program share
#pragma once
#include <stddef.h>
#include <vector>
#include "../../include/trackdlo_hip.h"
#include "tdlo_assign_lane.h"

namespace tdlo {

// what refuses the ropes or the gate (include/trackdlo_hip.h lists it), nullptr when nothing does
const char *assign_fault(const tdlo_assign_rope *ropes, int F, double d_max);
// the flat node list of checked ropes: off[F + 1], and the three coordinate arrays of off[F] entries each
void assign_flatten(const tdlo_assign_rope *ropes, int F, int *off, double *Yx, double *Yy, double *Yz);
// the lane, point by point, over tiles of `tile` nodes: owner (gated) and g per point (either may be NULL); X is n x 3 column-major
void assign_points_host(const double *X, int n, const int *off, int F, const double *Yx, const double *Yy, const double *Yz, double dmax2, int tile,
                        int *owner, double *owner_d2);

}  // namespace tdlo
