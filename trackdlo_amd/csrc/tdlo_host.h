// tdlo_host.h -- host-side helpers of the path (see tdlo_host.cpp).
#pragma once
#include <stddef.h>
#include <vector>
#include "../../include/trackdlo_hip.h"

namespace tdlo {

struct Vec3 { double x, y, z; };

// trackdlo::calc_LLE_weights (trackdlo.cpp:119-159); Y is M x 3 column-major, L is M x M column-major.
void lle_weights(int k, const double *Y, int M, double *L);
// H = (I - L)^T (I - L) (trackdlo.cpp:237)
void lle_regulariser(const double *L, int M, double *H);
// the same H for k = 6 as its 13 diagonals, Hb[13 i + u] = H(i, i - 6 + u) (bit for bit the dense routines' values), in O(M)
void lle_regulariser_band(const double *Y, int M, double *Hb);
// line_sphere_intersection (utils.cpp:185-241)
int line_sphere(const Vec3 &A, const Vec3 &B, const Vec3 &C, double radius, Vec3 out[2]);
// trackdlo::traverse_euclidean (trackdlo.cpp:584-898); out receives rows [idx, x, y, z].
// Returns the number of rows or -1 where the reference would index out of bounds.
int traverse_euclidean(const std::vector<double> &coord, const double *guide, int Mg,
                       const std::vector<int> &vis, int alignment, int anchor, std::vector<double> &out);

// The callback's self-occlusion test (trackdlo_node.cpp:279-343): indices of the nodes that are within visibility_threshold of the cloud AND whose
// projected pixel is not under an edge nearer the camera (edges = thick lines of dlo_pixel_width pixels).  proj: 3 x 4 row-major.  Ascending.
void self_occlusion_visible(const double *Y, int M, const double proj[12], int dlo_pixel_width, const double *node_dist, double visibility_threshold, std::vector<int> &vis);

// The primitives of the tracking-result image (trackdlo_node.cpp:377-444) in drawing order: 3 (M - 1) records of eight ints, see tdlo_host.cpp.
// Returns 0, or -1 when something cannot be drawn (prims is untouched then).
int render_primitives(const double *Y, int M, const double proj[12], const int *vis, int n_vis, int line_width, int node_radius,
                      const unsigned char node_visible[3], const unsigned char node_hidden[3], const unsigned char edge_visible[3],
                      const unsigned char edge_hidden[3], int *prims);

// The table k_render_batch reads (tdlo_render_batch_table, include/trackdlo_hip.h): the ropes ordered stably by image, a head record per rope, the ropes'
// primitive records one after the other.  order[j]: the list index of the rope at position j.  Returns -1 when every rope can be drawn, else the list index
// of the first rope that cannot (its image outside 0 .. K - 1, its node count outside 1 .. 1024, or refused by render_primitives).  dflt: the parameters
// of a rope that brings none.
int render_batch_table(const tdlo_render_rope *ropes, int R, int K, const tdlo_render_params &dflt, std::vector<int> &order, std::vector<int> &heads, std::vector<int> &prims,
                       std::vector<int> &rope_first);

// evaluator::get_piecewise_error (evaluator.cpp:258-283); chains are n x 3 column-major.
double piecewise_error(const double *Ytrack, int n1, const double *Ytrue, int n2);

// sort_pts (utils.cpp:95-170) with the chain coordinate of trackdlo_node.cpp:135-141, the host twin of k_sort_pts: Y is M x 3 column-major, M >= 2;
// Y_sorted (3 M, may be Y), perm (M: perm[i] = the row of Y at place i) and coord (M) may each be null.  Returns 0, or 1 a non-finite coordinate,
// 2 two equal nodes, 3 a round that finds no edge -- the outputs are untouched then.
int sort_pts_host(const double *Y, int M, double *Y_sorted, int *perm, double *coord);

}  // namespace tdlo
