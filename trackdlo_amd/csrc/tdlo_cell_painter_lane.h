// tdlo_cell_painter_lane.h -- the painter test over a cell of ropes (include/trackdlo_hip.h, "ropes that hide one another", has the statement): what ONE camera
// says about the N nodes of ALL ropes of a cell, as functions over plain arrays.  No HIP type: the very code k_cell_project / k_cell_cover run per lane
// (tdlo_cell_painter.hip) compiles for the host (tdlo_cell_painter_host.cpp: tdlo_cell_occlusion_visible) and runs over a whole (node block, camera, edge tile)
// grid under a sanitizer (tests/cpp/cell_painter_lane_host_test.cpp).
//
// Steps 1 and 2 are tdlo_painter_lane.h's painter_cam_node / painter_pixel, unchanged, and the key is its painter_edge_key: the units that include this header
// are built with contraction off.  What is new is the cell: nodes and edges carry FLAT indices n = off_f + m, an edge n exists where node n + 1 is in node n's
// rope (a bit per flat node: cell_link_words), "before" compares (key, flat index) pairs directly (painter_before), so nothing is ever ranked or sorted.
#pragma once
#include "tdlo_painter_lane.h"

namespace tdlo {

constexpr int kCellPainterMaxNodes = 16384;   // flat nodes of a cell: every node meets every edge, a call's time must stay bounded
constexpr int kCellPainterMaxCells = 1024;    // cells of a batch call
constexpr int kCellBlock = 256;               // nodes of a workgroup (lane = flat node)
constexpr int kCellTile = 512;                // edges of a tile staged through LDS: 513 records of 16 bytes = 8 KB a workgroup

// flag bit beside kPainterDrawable / kPainterSeen / kPainterPainted: edge n exists (node n + 1 is in node n's rope)
constexpr unsigned kCellLink = 8u;

// one record of a camera's table: flat node n and the edge that starts at it.  px: the pixel as two int16 (column low, row high; a pixel lies in [-8192, 8191])
struct CellRec { double key; int px; unsigned flag; };

TDLO_HD inline int cell_pack_px(int pc, int pr) { return (int)(((unsigned)pc & 0xffffu) | (((unsigned)pr & 0xffffu) << 16)); }
TDLO_HD inline int cell_px_c(int px) { return (int)(short)((unsigned)px & 0xffffu); }
TDLO_HD inline int cell_px_r(int px) { return (int)(short)(((unsigned)px >> 16) & 0xffffu); }

// the rope offset table as a bit per flat node: bit n is set when node n + 1 is in node n's rope.  words: ceil(N / 32), N the sum of the M_f
inline void cell_link_words(const int *M_each, int F, unsigned *words) {
    int N = 0;
    for (int f = 0; f < F; ++f) N += M_each[f];
    for (int q = 0; q < (N + 31) / 32; ++q) words[q] = 0u;
    int off = 0;
    for (int f = 0; f < F; ++f) {
        for (int m = 0; m + 1 < M_each[f]; ++m) words[(off + m) >> 5] |= 1u << ((off + m) & 31);
        off += M_each[f];
    }
}
TDLO_HD inline bool cell_link(const unsigned *words, int n) { return (words[n >> 5] >> (n & 31)) & 1u; }

// steps 1 - 2 for flat node n of a cell whose nodes lie as three arrays of N doubles, and the edge that starts at it when there is one (the camera-frame node
// n + 1 is formed again here: the same expressions, the same bits)
TDLO_HD inline CellRec cell_project(const PainterCam &c, const double *X, const double *Y, const double *Z, int n, bool link, int rows, int cols) {
    double ax, ay, az;
    int pc, pr;
    painter_cam_node(c, X[n], Y[n], Z[n], ax, ay, az);
    unsigned flag = painter_pixel(c, ax, ay, az, rows, cols, pc, pr);
    double key = 0.0;
    if (link) {
        flag |= kCellLink;
        double bx, by, bz;
        int qc, qr;
        painter_cam_node(c, X[n + 1], Y[n + 1], Z[n + 1], bx, by, bz);
        if ((flag & kPainterDrawable) && (painter_pixel(c, bx, by, bz, rows, cols, qc, qr) & kPainterDrawable)) {
            flag |= kPainterPainted;
            key = painter_edge_key(ax, ay, az, bx, by, bz);
        }
    }
    return CellRec{key, cell_pack_px(pc, pr), flag};
}

// step 4: the earlier of node n's painted incident edges as a (key, flat index) pair; has = 0: it has none and stands after every painted edge.  A painted
// edge n - 1 is an edge of n's rope (painted implies the link bit)
struct CellFirst { double key; int idx, has; };
TDLO_HD inline CellFirst cell_first(const CellRec *tab, int n) {
    CellFirst f{0.0, 0, 0};
    if (n > 0 && (tab[n - 1].flag & kPainterPainted)) f = CellFirst{tab[n - 1].key, n - 1, 1};
    if ((tab[n].flag & kPainterPainted) && (!f.has || painter_before(tab[n].key, n, f.key, f.idx))) f = CellFirst{tab[n].key, n, 1};
    return f;
}

// step 5, one test: edge e (record r, the pixel of node e + 1 in next_px, read only behind the painted test) is painted, stands strictly before the node's
// first, and covers its pixel.  The box reject is exact: a covered pixel lies within w / 2 of a point of the segment, so within w / 2 of the ends' box
TDLO_HD inline bool cell_edge_hides(const CellRec &r, int e, const CellRec *next, const CellFirst &f, int pc, int pr, int w) {
    if (!(r.flag & kPainterPainted)) return false;
    if (f.has && !painter_before(r.key, e, f.key, f.idx)) return false;
    const int ac = cell_px_c(r.px), ar = cell_px_r(r.px), bc = cell_px_c(next->px), br = cell_px_r(next->px);
    const int c0 = ac < bc ? ac : bc, c1 = ac < bc ? bc : ac, r0 = ar < br ? ar : br, r1 = ar < br ? br : ar;
    if (2 * (c0 - pc) > w || 2 * (pc - c1) > w || 2 * (r0 - pr) > w || 2 * (pr - r1) > w) return false;
    return within_half_width(Px{pc, pr}, Px{ac, ar}, Px{bc, br}, (long long)w);
}

// step 5 over one tile of edges e0 .. e0 + cnt - 1: tile[i] is the record of flat node e0 + i; tile[cnt] is read only for a painted last edge, whose end
// node e0 + cnt then exists.  This is what a lane of k_cell_cover does with a tile in LDS
TDLO_HD inline bool cell_tile_hides(const CellRec *tile, int e0, int cnt, const CellFirst &f, int pc, int pr, int w) {
    for (int i = 0; i < cnt; ++i)
        if (cell_edge_hides(tile[i], e0 + i, tile + i + 1, f, pc, pr, w)) return true;
    return false;
}

// One (camera, cell) job on one thread: the table of N records, seen / hidden bits of the N flat nodes into ceil(N / 32) words each.  A node that is not
// drawable is neither seen nor hidden; a drawable node outside the image may be hidden.  The kernels run the same steps with a lane per node
inline void cell_job(const PainterCam &c, const double *X, const double *Y, const double *Z, const unsigned *link, int N, int rows, int cols, int w,
                     CellRec *tab, unsigned *seen_words, unsigned *hidden_words) {
    const int W = (N + 31) / 32;
    for (int q = 0; q < W; ++q) { seen_words[q] = 0u; hidden_words[q] = 0u; }
    for (int n = 0; n < N; ++n) {
        tab[n] = cell_project(c, X, Y, Z, n, cell_link(link, n), rows, cols);
        if (tab[n].flag & kPainterSeen) seen_words[n >> 5] |= 1u << (n & 31);
    }
    for (int n = 0; n < N; ++n) {
        if (!(tab[n].flag & kPainterDrawable)) continue;
        const CellFirst f = cell_first(tab, n);
        const int pc = cell_px_c(tab[n].px), pr = cell_px_r(tab[n].px);
        bool hidden = false;
        for (int e0 = 0; e0 < N && !hidden; e0 += kCellTile) hidden = cell_tile_hides(tab + e0, e0, N - e0 < kCellTile ? N - e0 : kCellTile, f, pc, pr, w);
        if (hidden) hidden_words[n >> 5] |= 1u << (n & 31);
    }
}

}  // namespace tdlo
