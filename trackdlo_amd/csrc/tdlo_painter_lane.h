// tdlo_painter_lane.h -- the self-occlusion test under a rig (include/trackdlo_hip.h, "self-occlusion under a rig", has the statement): what ONE camera says
// about the nodes of ONE rope, as functions over plain arrays.  No HIP type: the very code k_rig_painter_batch runs per (camera, frame) job (tdlo_painter.hip)
// compiles for the host (tdlo_painter_host.cpp: tdlo_rig_self_occlusion_visible) and runs job by job under a sanitizer (tests/cpp/rig_painter_test.cpp).
//
// THE ARITHMETIC of steps 1 - 3 is double, every product and every sum rounded on its own in the order written (rig_mul / rig_add of tdlo_rig_point.h: plain
// operators under the contraction pragma; the units that include this header are built with contraction off as well).  Division and square root are IEEE's.
// Steps 4 - 5 are integers: ranks by counting, coverage by within_half_width (tdlo_thick_line.h, unchanged).
#pragma once
#include "tdlo_rig_point.h"
#include "tdlo_thick_line.h"

namespace tdlo {

constexpr int kPainterMaxNodes = 1024;   // nodes of a rope (render_batch_table's limit)
constexpr int kPainterMaxCams = 64;      // cameras of a rig (kRigMaxCams)

// one record of the camera table: the intrinsics and rig_to_cam = [A | b] (has_T = 0: the camera frame is the rig frame)
struct PainterCam {
    double fx, fy, cx, cy;
    double T[12];
    int has_T, pad_;
};

// flag bits of a node in one camera
constexpr unsigned kPainterDrawable = 1u, kPainterSeen = 2u;

// step 1: the node in the camera's frame
TDLO_HD inline void painter_cam_node(const PainterCam &c, double x, double y, double z, double &xc, double &yc, double &zc) {
    if (!c.has_T) { xc = x; yc = y; zc = z; return; }
    xc = rig_add(rig_add(rig_add(rig_mul(c.T[0], x), rig_mul(c.T[1], y)), rig_mul(c.T[2], z)), c.T[3]);
    yc = rig_add(rig_add(rig_add(rig_mul(c.T[4], x), rig_mul(c.T[5], y)), rig_mul(c.T[6], z)), c.T[7]);
    zc = rig_add(rig_add(rig_add(rig_mul(c.T[8], x), rig_mul(c.T[9], y)), rig_mul(c.T[10], z)), c.T[11]);
}

// step 2: the node's pixel and flags.  Drawable: z_c > 0 and both quotients in (-8193, 8192) (render_primitives' rule; NaN and infinities fail it), the pixel
// then lies in [-8192, 8191]; seen: drawable and inside the rows x cols image.  A node that is not drawable gets pixel (0, 0), which nothing reads
TDLO_HD inline unsigned painter_pixel(const PainterCam &c, double xc, double yc, double zc, int rows, int cols, int &pc, int &pr) {
    pc = 0; pr = 0;
    if (!(zc > 0)) return 0u;
    const double u = rig_add(rig_mul(c.fx, xc), rig_mul(c.cx, zc)), v = rig_add(rig_mul(c.fy, yc), rig_mul(c.cy, zc));
    const double qc = u / zc, qr = v / zc;
    if (!(qc > -8193.0 && qc < 8192.0 && qr > -8193.0 && qr < 8192.0)) return 0u;
    pc = (int)qc; pr = (int)qr;
    return kPainterDrawable | ((pc >= 0 && pc < cols && pr >= 0 && pr < rows) ? kPainterSeen : 0u);
}

// step 3: the key of the edge between two camera-frame nodes (tdlo_host.cpp:440-441)
TDLO_HD inline double painter_edge_key(double ax, double ay, double az, double bx, double by, double bz) {
    const double mx = rig_add(ax, bx) / 2, my = rig_add(ay, by) / 2, mz = rig_add(az, bz) / 2;
    return __builtin_sqrt(rig_add(rig_add(rig_mul(mx, mx), rig_mul(my, my)), rig_mul(mz, mz)));
}

// (key, index) ascending: edge j is painted before edge i.  Keys of painted edges are never NaN (their ends are drawable, so finite)
TDLO_HD inline bool painter_before(double kj, int j, double ki, int i) { return kj < ki || (kj == ki && j < i); }

// steps 1 - 3 for node m of a rope whose nodes lie column-major in Y (x: Y[m], y: Y[M + m], z: Y[2 M + m]): pixel, flags and, when m < M - 1, the key of edge m
// and whether it is painted (the camera-frame node m + 1 is formed again here: the same expressions, the same bits)
TDLO_HD inline void painter_node_edge(const PainterCam &c, const double *Y, int M, int m, int rows, int cols, int &pc, int &pr, unsigned &flag, double &key, bool &painted) {
    double ax, ay, az;
    painter_cam_node(c, Y[m], Y[M + m], Y[2 * (long long)M + m], ax, ay, az);
    flag = painter_pixel(c, ax, ay, az, rows, cols, pc, pr);
    key = 0.0; painted = false;
    if (m + 1 < M) {
        double bx, by, bz;
        int qc, qr;
        painter_cam_node(c, Y[m + 1], Y[M + m + 1], Y[2 * (long long)M + m + 1], bx, by, bz);
        painted = (flag & kPainterDrawable) && (painter_pixel(c, bx, by, bz, rows, cols, qc, qr) & kPainterDrawable);
        if (painted) key = painter_edge_key(ax, ay, az, bx, by, bz);
    }
}

// flag bit of edge m, kept in node m's byte beside the two above
constexpr unsigned kPainterPainted = 4u;

// rank of painted edge i by counting: the painted edges j with (key_j, j) < (key_i, i)
TDLO_HD inline int painter_rank(const double *key, const unsigned char *flag, int nE, int i) {
    int r = 0;
    const double ki = key[i];
    for (int j = 0; j < nE; ++j) r += ((flag[j] & kPainterPainted) && painter_before(key[j], j, ki, i)) ? 1 : 0;
    return r;
}

// step 4: the smaller rank of node m's painted incident edges, nP (the number of painted edges) when it has none.  rank[e] < 0: edge e is not painted
TDLO_HD inline int painter_first(const int *rank, int M, int m, int nP) {
    int f = nP;
    if (m > 0 && rank[m - 1] >= 0 && rank[m - 1] < f) f = rank[m - 1];
    if (m + 1 < M && rank[m] >= 0 && rank[m] < f) f = rank[m];
    return f;
}

// step 5, one test: the painted edge of rank r (order[r]) covers node m's pixel
TDLO_HD inline bool painter_covers(const int *order, const int *pc, const int *pr, int r, int m, int w) {
    const int e = order[r];
    return within_half_width(Px{pc[m], pr[m]}, Px{pc[e], pr[e]}, Px{pc[e + 1], pr[e + 1]}, (long long)w);
}

// One (camera, frame) job on one thread: seen / hidden bits of the M nodes into ceil(M / 32) words each.  A node that is not drawable has no pixel and is
// neither seen nor hidden; a drawable node outside the image may be hidden (it is not seen, so the camera has no say on it either way).  Scratch: pc, pr, rank,
// order: M ints each; key: M doubles; flag: M bytes.  The kernel runs the same steps with a thread per node / edge and a wave per node in the coverage loop
inline void painter_job(const PainterCam &c, const double *Y, int M, int rows, int cols, int w, int *pc, int *pr, int *rank, int *order, double *key,
                        unsigned char *flag, unsigned *seen_words, unsigned *hidden_words) {
    const int nE = M - 1, W = (M + 31) / 32;
    for (int q = 0; q < W; ++q) { seen_words[q] = 0u; hidden_words[q] = 0u; }
    for (int m = 0; m < M; ++m) {
        unsigned f; bool p;
        painter_node_edge(c, Y, M, m, rows, cols, pc[m], pr[m], f, key[m], p);
        flag[m] = (unsigned char)(f | (p ? kPainterPainted : 0u));
        if (f & kPainterSeen) seen_words[m >> 5] |= 1u << (m & 31);
    }
    int nP = 0;
    for (int i = 0; i < nE; ++i) {
        const bool p = (flag[i] & kPainterPainted) != 0;
        rank[i] = p ? painter_rank(key, flag, nE, i) : -1;
        if (p) { order[rank[i]] = i; ++nP; }
    }
    for (int m = 0; m < M; ++m) {
        if (!(flag[m] & kPainterDrawable)) continue;
        const int first = painter_first(rank, M, m, nP);
        bool hidden = false;
        for (int r = 0; r < first && !hidden; ++r) hidden = painter_covers(order, pc, pr, r, m, w);
        if (hidden) hidden_words[m >> 5] |= 1u << (m & 31);
    }
}

}  // namespace tdlo
