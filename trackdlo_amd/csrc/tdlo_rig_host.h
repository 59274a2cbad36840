// tdlo_rig_host.h -- the host half of a rig (tdlo_rig_host.cpp; no HIP): what the driver and a stand-alone program share
#pragma once
#include <stddef.h>
#include "../../include/trackdlo_hip.h"
#include "tdlo_rig_point.h"

namespace tdlo {

// tdlo_colour_params as the kernels take it (packed lower bounds and spans, the ranges that can pass, the byte order); false: bad params
bool colour_ranges_pack(const tdlo_colour_params *p, unsigned lo_out[4], unsigned span_out[4], int *n_out, int *rgb_out);
// what refuses a rig call as a whole (include/trackdlo_hip.h lists it), nullptr when nothing does
const char *rig_fault(const tdlo_rig_camera *cams, int K, int rows, int cols, double leaf_size);
// a camera of a checked rig is segmented by colour (it brings no mask)
bool rig_camera_colour(const tdlo_rig_camera &cam);
// a camera of a checked rig as the camera table holds it, the plane pointers as the caller gave them
void rig_camera_record(const tdlo_rig_camera &cam, RigCam &rc);
// R of a checked rig whose planes lie in host memory: up to `capacity` points as x y z floats; *n_raw_out = the length of R.  TDLO_E_INVALID: R_out is too short
int rig_points_host(const tdlo_rig_camera *cams, int K, int rows, int cols, float *R_out, int capacity, int *n_raw_out);

}  // namespace tdlo
