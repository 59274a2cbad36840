// The lane of the painter test over a cell of ropes (csrc/tdlo_cell_painter_lane.h) run the way the kernels run it -- k_cell_project lane by lane, then
// k_cell_cover over the whole (node block, camera, edge tile) grid with every tile copied into an allocation of exactly the records a workgroup stages --
// with every array at its exact extent, under -fsanitize=address,undefined.  No HIP; linked with csrc/tdlo_cell_painter_host.cpp and csrc/tdlo_painter_host.cpp.
// argv[1]: the cells, little-endian: int32 C; per cell int32 F, K, rows, cols, w; int32 M[F]; double cams[K][4]; double rig_to_cam[K][12] (12 NaN: none);
// per rope M x 3 doubles column-major.  Prints the number of (camera, cell) jobs, how many differ from the host statement's words, the hidden bits and an
// FNV-1a hash of all words (per cell the seen words, then the hidden words), which the test compares with the reference's.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "tdlo_cell_painter_host.h"

using namespace tdlo;

template <class T> static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n]); }

static bool rd(FILE *f, void *p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int C = 0;
    if (!rd(f, &C, 4)) return 2;
    long long jobs = 0, differ = 0, hidden_bits = 0;
    unsigned long long h = 1469598103934665603ull;
    auto eat = [&](const unsigned *w, size_t n) {
        for (size_t i = 0; i < 4 * n; ++i) { h ^= ((const unsigned char *)w)[i]; h *= 1099511628211ull; }
    };
    for (int ci = 0; ci < C; ++ci) {
        int hd[5];
        if (!rd(f, hd, sizeof hd)) return 2;
        const int F = hd[0], K = hd[1], rows = hd[2], cols = hd[3], w = hd[4];
        std::vector<int> Ms(F);
        if (!rd(f, Ms.data(), 4 * (size_t)F)) return 2;
        std::vector<tdlo_rig_camera> cams(K);
        std::memset(cams.data(), 0, sizeof(tdlo_rig_camera) * K);
        for (int k = 0; k < K; ++k) { double v[4]; if (!rd(f, v, sizeof v)) return 2; cams[k].fx = v[0]; cams[k].fy = v[1]; cams[k].cx = v[2]; cams[k].cy = v[3]; }
        std::vector<double> T(12 * (size_t)K);
        if (!rd(f, T.data(), 8 * T.size())) return 2;
        std::vector<std::vector<double>> Ys(F);
        std::vector<std::vector<double>> dist(F);
        std::vector<tdlo_cell_rope> ropes(F);
        for (int r = 0; r < F; ++r) {
            Ys[r].resize(3 * (size_t)Ms[r]); dist[r].assign(Ms[r], 0.0);
            if (!rd(f, Ys[r].data(), 8 * Ys[r].size())) return 2;
            ropes[r] = tdlo_cell_rope{Ys[r].data(), Ms[r], dist[r].data(), 1.0};
        }
        if (cell_painter_fault(ropes.data(), F, cams.data(), T.data(), K, rows, cols, w)) { printf("cell %d is refused\n", ci); return 1; }
        const int N = cell_painter_nodes(ropes.data(), F), W = (N + 31) / 32;
        auto X = exact<double>(N), Y = exact<double>(N), Z = exact<double>(N);
        auto link = exact<unsigned>(W);
        cell_painter_flatten(ropes.data(), F, X.get(), Y.get(), Z.get(), link.get());
        std::vector<PainterCam> pc(K);
        for (int k = 0; k < K; ++k) rig_painter_camera(cams[k], T.data() + 12 * (size_t)k, pc[k]);
        // the host statement's words
        auto hs = exact<unsigned>((size_t)K * W), hh = exact<unsigned>((size_t)K * W);
        cell_painter_host(X.get(), Y.get(), Z.get(), link.get(), N, pc.data(), K, rows, cols, w, hs.get(), hh.get());
        // the grid
        auto gs = exact<unsigned>((size_t)K * W), gh = exact<unsigned>((size_t)K * W);
        for (size_t i = 0; i < (size_t)K * W; ++i) gs[i] = gh[i] = 0u;
        for (int k = 0; k < K; ++k) {
            auto tab = exact<CellRec>(N);
            for (int n = 0; n < N; ++n) {                                      // k_cell_project, lane by lane
                tab[n] = cell_project(pc[k], X.get(), Y.get(), Z.get(), n, cell_link(link.get(), n), rows, cols);
                if (tab[n].flag & kPainterSeen) gs[(size_t)k * W + (n >> 5)] |= 1u << (n & 31);
            }
            for (int b0 = 0; b0 < N; b0 += kCellBlock)                         // k_cell_cover: node block x edge tile
                for (int e0 = 0; e0 < N; e0 += kCellTile) {
                    const int cnt = N - e0 < kCellTile ? N - e0 : kCellTile, have = cnt + (e0 + cnt < N ? 1 : 0);
                    auto tile = exact<CellRec>(have);
                    for (int i = 0; i < have; ++i) tile[i] = tab[e0 + i];
                    for (int n = b0; n < b0 + kCellBlock && n < N; ++n) {
                        if (!(tab[n].flag & kPainterDrawable) || ((gh[(size_t)k * W + (n >> 5)] >> (n & 31)) & 1u)) continue;
                        const CellFirst first = cell_first(tab.get(), n);
                        if (cell_tile_hides(tile.get(), e0, cnt, first, cell_px_c(tab[n].px), cell_px_r(tab[n].px), w)) gh[(size_t)k * W + (n >> 5)] |= 1u << (n & 31);
                    }
                }
            ++jobs;
            bool same = true;
            for (int q = 0; q < W; ++q) {
                same = same && gs[(size_t)k * W + q] == hs[(size_t)k * W + q] && gh[(size_t)k * W + q] == hh[(size_t)k * W + q];
                hidden_bits += __builtin_popcount(gh[(size_t)k * W + q]);
            }
            differ += same ? 0 : 1;
        }
        eat(gs.get(), (size_t)K * W); eat(gh.get(), (size_t)K * W);
    }
    fclose(f);
    printf("%lld jobs, %lld with a differing word, %lld hidden bits, hash %016llx\n", jobs, differ, hidden_bits, h);
    return differ ? 1 : 0;
}
