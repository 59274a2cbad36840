// rig_painter_test.cpp -- the lane of the self-occlusion test under a rig (csrc/tdlo_painter_lane.h) and its host statement (csrc/tdlo_painter_host.cpp) over a
// whole (camera, frame) grid, as the kernel walks it: every job on heap arrays of exactly the job's extents, so that a sanitizer sees any index beyond them.
// Built by tests/test_rig_painter_ref.py with -fsanitize=address,undefined together with tdlo_painter_host.cpp and run directly: no HIP, no library, no preload.
// Per job the words are formed twice -- painter_job on the thread's own scratch, and the kernel's schedule (nodes in waves of 64 with two seen words per wave, edges
// ranked one by one, a 32-node word per wave with the ranks below `first` walked in strides of 64) -- and compared with the public call's words; the union with
// its visible set.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tdlo_painter_host.h"

using namespace tdlo;

static unsigned long long lcg = 0x9e3779b97f4a7c15ull;
static double uni(double a, double b) {
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    return a + (b - a) * (double)(lcg >> 11) / 9007199254740992.0;
}

// the kernel's schedule for one job on exact-extent heap arrays
static void kernel_schedule(const PainterCam &cam, const double *Y, int M, int rows, int cols, int w, unsigned *seen, unsigned *hidden) {
    const int nE = M - 1, W = (M + 31) / 32;
    std::vector<double> key(M);
    std::vector<int> pc(M), pr(M), rank(M), order(M);
    std::vector<unsigned char> flag(M);
    int nP = 0;
    for (int m0 = 0; m0 < M; m0 += 64) {
        unsigned long long s = 0ull;
        for (int lane = 0; lane < 64; ++lane) {
            const int m = m0 + lane;
            if (m >= M) continue;
            unsigned fl; double ky; bool p;
            painter_node_edge(cam, Y, M, m, rows, cols, pc[m], pr[m], fl, ky, p);
            key[m] = ky;
            flag[m] = (unsigned char)(fl | (p ? kPainterPainted : 0u));
            if (fl & kPainterSeen) s |= 1ull << lane;
        }
        const int q = m0 >> 5;
        seen[q] = (unsigned)s;
        if (q + 1 < W) seen[q + 1] = (unsigned)(s >> 32);
    }
    for (int i = 0; i < nE; ++i) {
        const bool p = (flag[i] & kPainterPainted) != 0;
        rank[i] = p ? painter_rank(key.data(), flag.data(), nE, i) : -1;
        if (p) { order[rank[i]] = i; ++nP; }
    }
    for (int q = 0; q < W; ++q) {
        unsigned word = 0u;
        for (int b = 0; b < 32 && 32 * q + b < M; ++b) {
            const int m = 32 * q + b;
            if (!(flag[m] & kPainterDrawable)) continue;
            const int first = painter_first(rank.data(), M, m, nP);
            bool hit = false;
            for (int r0 = 0; r0 < first && !hit; r0 += 64)
                for (int lane = 0; lane < 64; ++lane) { const int r = r0 + lane; if (r < first && painter_covers(order.data(), pc.data(), pr.data(), r, m, w)) hit = true; }
            if (hit) word |= 1u << b;
        }
        hidden[q] = word;
    }
}

int main() {
    const int Ms[] = {1, 2, 3, 31, 32, 33, 45, 64, 65, 128, 256, 257, 300, 1024};
    const int Ks[] = {1, 2, 3, 64, 1, 4, 3, 2, 1, 5, 2, 1, 3, 1};
    long long jobs = 0, bad = 0, hidden_bits = 0;
    for (int f = 0; f < 14; ++f) {
        const int M = Ms[f], K = Ks[f], W = (M + 31) / 32, rows = 480, cols = 640, w = 1 + (f * 37) % 255;
        double *Y = (double *)std::malloc(sizeof(double) * 3 * M);
        const double a0 = uni(0.5, 3), a1 = uni(0.5, 3), a2 = uni(0.5, 3), p0 = uni(0, 6.28), p1 = uni(0, 6.28), p2 = uni(0, 6.28);
        for (int m = 0; m < M; ++m) {
            const double t = M > 1 ? (double)m / (M - 1) : 0.0;
            Y[m] = 0.25 * std::sin(6.283185307179586 * a0 * t + p0); Y[M + m] = 0.2 * std::sin(6.283185307179586 * a1 * t + p1);
            Y[2 * M + m] = 0.6 + 0.15 * std::sin(6.283185307179586 * a2 * t + p2);
        }
        if (M > 4) { Y[2 * M + 3] = -0.5; Y[1] = NAN; }                       // a node behind the first camera, a node that is nowhere
        tdlo_rig_camera *cams = (tdlo_rig_camera *)std::calloc(K, sizeof(tdlo_rig_camera));
        double *T = (double *)std::malloc(sizeof(double) * 12 * K);
        for (int k = 0; k < K; ++k) {
            cams[k].fx = uni(400, 700); cams[k].fy = uni(400, 700); cams[k].cx = uni(250, 390); cams[k].cy = uni(180, 300);
            const double th = uni(-3.14, 3.14), c = std::cos(th), s = std::sin(th);
            const double R[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
            const double tz = uni(0.5, 0.9);
            for (int r = 0; r < 3; ++r) { for (int q = 0; q < 3; ++q) T[12 * k + 4 * r + q] = R[3 * r + q]; T[12 * k + 4 * r + 3] = -R[3 * r + 2] * 0.6 + (r == 2 ? tz : 0.0); }
            if (k % 3 == 0) for (int q = 0; q < 12; ++q) T[12 * k + q] = NAN;  // "no matrix for this camera"
        }
        double *dist = (double *)std::malloc(sizeof(double) * M);
        for (int m = 0; m < M; ++m) dist[m] = uni(0, 0.016);
        int *vis = (int *)std::malloc(sizeof(int) * M), nv = -1;
        unsigned *seen = (unsigned *)std::malloc(sizeof(unsigned) * K * W), *hidden = (unsigned *)std::malloc(sizeof(unsigned) * K * W);
        if (tdlo_rig_self_occlusion_visible(Y, M, cams, T, K, rows, cols, w, dist, 0.008, vis, &nv, seen, hidden) != TDLO_OK) { std::printf("frame %d refused\n", f); return 2; }
        for (int k = 0; k < K; ++k, ++jobs) {
            PainterCam pcam;
            rig_painter_camera(cams[k], T + 12 * k, pcam);
            unsigned *s1 = (unsigned *)std::malloc(sizeof(unsigned) * W), *h1 = (unsigned *)std::malloc(sizeof(unsigned) * W);
            kernel_schedule(pcam, Y, M, rows, cols, w, s1, h1);
            if (std::memcmp(s1, seen + k * W, sizeof(unsigned) * W) || std::memcmp(h1, hidden + k * W, sizeof(unsigned) * W)) ++bad;
            for (int q = 0; q < W; ++q) hidden_bits += __builtin_popcount(h1[q]);
            std::free(s1); std::free(h1);
        }
        // the union, by hand
        int n = 0;
        for (int m = 0; m < M; ++m) {
            bool ok = false;
            for (int k = 0; k < K; ++k) ok = ok || (((seen[k * W + (m >> 5)] & ~hidden[k * W + (m >> 5)]) >> (m & 31)) & 1u);
            if (ok && dist[m] <= 0.008) { if (n >= nv || vis[n] != m) ++bad; ++n; }
        }
        if (n != nv) ++bad;
        std::free(Y); std::free(cams); std::free(T); std::free(dist); std::free(vis); std::free(seen); std::free(hidden);
    }
    // refusals: nothing is written
    {
        double Y[3] = {0, 0, 1}, d[1] = {0}, T[12];
        for (double &v : T) v = 0.0;
        T[5] = INFINITY;
        tdlo_rig_camera cam; std::memset(&cam, 0, sizeof cam); cam.fx = cam.fy = 500;
        int vis[1] = {-7}, nv = -7;
        int rc = 0;
        rc += tdlo_rig_self_occlusion_visible(Y, 0, &cam, nullptr, 1, 8, 8, 1, d, 1, vis, &nv, nullptr, nullptr) == TDLO_E_INVALID;
        rc += tdlo_rig_self_occlusion_visible(Y, 1025, &cam, nullptr, 1, 8, 8, 1, d, 1, vis, &nv, nullptr, nullptr) == TDLO_E_INVALID;
        rc += tdlo_rig_self_occlusion_visible(Y, 1, &cam, nullptr, 65, 8, 8, 1, d, 1, vis, &nv, nullptr, nullptr) == TDLO_E_INVALID;
        rc += tdlo_rig_self_occlusion_visible(Y, 1, &cam, nullptr, 1, 8, 8, 256, d, 1, vis, &nv, nullptr, nullptr) == TDLO_E_INVALID;
        rc += tdlo_rig_self_occlusion_visible(Y, 1, &cam, nullptr, 1, 8193, 8, 1, d, 1, vis, &nv, nullptr, nullptr) == TDLO_E_INVALID;
        rc += tdlo_rig_self_occlusion_visible(Y, 1, &cam, T, 1, 8, 8, 1, d, 1, vis, &nv, nullptr, nullptr) == TDLO_E_INVALID;
        cam.fx = 0;
        rc += tdlo_rig_self_occlusion_visible(Y, 1, &cam, nullptr, 1, 8, 8, 1, d, 1, vis, &nv, nullptr, nullptr) == TDLO_E_INVALID;
        if (rc != 7 || vis[0] != -7 || nv != -7) { std::printf("refusals: %d of 7\n", rc); return 3; }
    }
    std::printf("%lld jobs, %lld with a differing word, %lld hidden bits\n", jobs, bad, hidden_bits);
    return bad ? 1 : 0;
}
