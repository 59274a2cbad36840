// tdlo_painter_host.h -- the host half of the self-occlusion test under a rig (tdlo_painter_host.cpp; no HIP): what the driver and a stand-alone program share
#pragma once
#include <stddef.h>
#include <vector>
#include "../../include/trackdlo_hip.h"
#include "tdlo_painter_lane.h"

namespace tdlo {

// what refuses a frame of the test (include/trackdlo_hip.h lists it), nullptr when nothing does
const char *rig_painter_fault(const double *Y, int M, const tdlo_rig_camera *cams, const double *rig_to_cam, int K, int rows, int cols, int dlo_pixel_width,
                              const double *node_dist);
// camera k of a checked frame as the camera table holds it (rig_to_cam: NULL, or K x 12 with a camera's 12 entries all NaN for "none")
void rig_painter_camera(const tdlo_rig_camera &cam, const double *rig_to_cam_k, PainterCam &pc);
// the lane, camera by camera: seen / hidden words of K cameras, K x ceil(M / 32) each
void rig_painter_host(const double *Y, int M, const PainterCam *cams, int K, int rows, int cols, int dlo_pixel_width, unsigned *seen_words, unsigned *hidden_words);
// the rig's verdict from the words: node_dist[m] <= visibility_threshold and some camera sees m and does not hide it; ascending
void rig_painter_verdict(const unsigned *seen_words, const unsigned *hidden_words, int K, int M, const double *node_dist, double visibility_threshold,
                         std::vector<int> &vis);

}  // namespace tdlo
