// tdlo_cell_painter_host.h -- the host half of the painter test over a cell of ropes (tdlo_cell_painter_host.cpp; no HIP): what the driver and a stand-alone
// program share
#pragma once
#include <stddef.h>
#include <vector>
#include "../../include/trackdlo_hip.h"
#include "tdlo_cell_painter_lane.h"
#include "tdlo_painter_host.h"

namespace tdlo {

// what refuses a cell (include/trackdlo_hip.h lists it), nullptr when nothing does.  need_dist: the ropes' node_dist must be there (the tracker call brings
// its own later)
const char *cell_painter_fault(const tdlo_cell_rope *ropes, int F, const tdlo_rig_camera *cams, const double *rig_to_cam, int K, int rows, int cols,
                               int dlo_pixel_width, bool need_dist = true);
// the number of flat nodes of a checked cell
int cell_painter_nodes(const tdlo_cell_rope *ropes, int F);
// the nodes of a checked cell as three arrays of N doubles and the link bits (ceil(N / 32) words)
void cell_painter_flatten(const tdlo_cell_rope *ropes, int F, double *X, double *Y, double *Z, unsigned *link);
// the lane, camera by camera: seen / hidden words of K cameras, K x ceil(N / 32) each
void cell_painter_host(const double *X, const double *Y, const double *Z, const unsigned *link, int N, const PainterCam *cams, int K, int rows, int cols,
                       int dlo_pixel_width, unsigned *seen_words, unsigned *hidden_words);
// the verdict on ONE rope from the cell's words: its nodes are the flat nodes off .. off + M - 1; rope-local indices, ascending
void cell_painter_verdict(const unsigned *seen_words, const unsigned *hidden_words, int K, int N, int off, int M, const double *node_dist,
                          double visibility_threshold, std::vector<int> &vis);

}  // namespace tdlo
