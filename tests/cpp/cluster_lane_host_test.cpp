// cluster_lane_host_test.cpp -- the lane of csrc/tdlo_cluster_lane.h over a whole (workgroup, tile) grid on the host, under a sanitizer (tests/test_cluster_ref.py
// builds this file with csrc/tdlo_cluster_host.cpp, -fsanitize=address,undefined, and runs it).  Every array is allocated at exactly its extent -- the forest at n
// ints, every staged tile at the points k_cluster_link stages for that workgroup -- so a lane that reads a point beyond its tile or a parent beyond the cloud is
// caught.  The jobs (workgroup, tile at or below its own) run in several visiting orders, the lanes of a job forwards or backwards: the roots must be the same
// for every order -- the smallest index of every component -- and must number the clusters as the C entry point tdlo_cloud_cluster_host numbers them.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../include/trackdlo_hip.h"
#include "tdlo_cluster_lane.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t next() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}
static double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }

int main() {
    const double tol = 0.02, tol2 = tol * tol;
    const int sizes[] = {1, 63, 65, 257, 513, 1025};
    long long runs = 0, differing = 0, clusters = 0, skipped = 0;
    for (int n : sizes) {
        // three ropes interleaved point by point, a chain of points 0.9 tol apart in scrambled order behind them, points that are not finite in between
        std::vector<double> X(3 * (size_t)n);
        const int nr = n - n / 4;
        for (int i = 0; i < n; ++i) {
            if (i < nr) { X[i] = 0.1 + 0.1 * uni(); X[n + i] = 0.2 + 0.05 * (i % 3) + 0.001 * uni(); X[2 * (size_t)n + i] = 0.6; }
            else { const int m = n - nr, k = (int)(((long long)(i - nr) * 7) % m); X[i] = 0.9 * tol * k; X[n + i] = 0.9; X[2 * (size_t)n + i] = 0.6; }
            if (i % 97 == 13) X[i] = NAN;
            if (i % 101 == 17) X[n + i] = INFINITY;
        }
        std::vector<int> want;
        for (int block : {64, 256})
            for (int tile : {block, 2 * block, 512}) {
                if (tile % block) continue;
                const int nb = (n + block - 1) / block;
                std::vector<std::pair<int, int>> jobs;
                for (int b = 0; b < nb; ++b)
                    for (int tl = 0; tl <= b * block / tile; ++tl) jobs.push_back({b, tl});
                for (int order = 0; order < 5; ++order) {
                    std::vector<std::pair<int, int>> seq = jobs;
                    if (order == 1) std::reverse(seq.begin(), seq.end());
                    if (order == 2) std::stable_sort(seq.begin(), seq.end(), [](auto a, auto b) { return a.second > b.second; });
                    if (order >= 3) for (size_t k = seq.size(); k > 1; --k) std::swap(seq[k - 1], seq[next() % k]);
                    std::vector<int> parent((size_t)n), r((size_t)n);
                    for (int i = 0; i < n; ++i) parent[i] = r[i] = i;
                    for (auto [b, tl] : seq) {
                        const int i0 = b * block, end = std::min(i0 + block, n), t0 = tl * tile, cnt = std::min(end - t0, tile);
                        const std::vector<double> Lx(X.begin() + t0, X.begin() + t0 + cnt), Ly(X.begin() + n + t0, X.begin() + n + t0 + cnt),
                            Lz(X.begin() + 2 * (size_t)n + t0, X.begin() + 2 * (size_t)n + t0 + cnt);
                        for (int q = 0; q < end - i0; ++q) {
                            const int i = (order & 1) ? end - 1 - q : i0 + q;
                            const double x = X[i], y = X[n + i], z = X[2 * (size_t)n + i];
                            if (!tdlo::cluster_finite(x, y, z)) { ++skipped; continue; }
                            if (!tdlo::cluster_tile(Lx.data(), Ly.data(), Lz.data(), t0, cnt, i, x, y, z, tol2, parent.data(), r[i])) { printf("gave up\n"); return 1; }
                        }
                    }
                    std::vector<int> root((size_t)n);
                    for (int i = 0; i < n; ++i) root[i] = tdlo::cluster_find(parent.data(), i);
                    if (want.empty()) want = root;
                    ++runs;
                    for (int i = 0; i < n; ++i) differing += root[i] != want[i];
                }
            }
        // the roots against the definition: a linked pair shares its root, a root is the smallest index that has it ...
        for (int i = 0; i < n; ++i) {
            differing += want[i] > i || want[want[i]] != want[i];
            for (int j = 0; j < i; ++j)
                if (tdlo::cluster_link(X[i], X[n + i], X[2 * (size_t)n + i], X[j], X[n + j], X[2 * (size_t)n + j], tol2)) differing += want[i] != want[j];
        }
        // ... and the C entry point numbers the clusters by them (F = n destinations, min_size 1: every cluster is kept and owned)
        std::vector<int> own((size_t)n), each((size_t)n);
        int C = 0, un = 0;
        if (tdlo_cloud_cluster_host(X.data(), n, n, tol, 1, own.data(), &C, each.data(), &un) != TDLO_OK) { printf("refused\n"); return 1; }
        int rank = 0;
        for (int i = 0; i < n; ++i) {
            const bool fin = tdlo::cluster_finite(X[i], X[n + i], X[2 * (size_t)n + i]);
            if (fin && want[i] == i) { differing += own[i] != rank; ++rank; }
            differing += fin ? own[i] != own[want[i]] : own[i] != -1;
        }
        differing += rank != C;
        clusters += C;
    }
    printf("%lld runs, %lld differing, %lld clusters, %lld lanes skipped\n", runs, differing, clusters, skipped);
    return differing ? 1 : 0;
}
