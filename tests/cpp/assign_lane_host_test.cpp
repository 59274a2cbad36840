// assign_lane_host_test.cpp -- the lane of csrc/tdlo_assign_lane.h over a whole (block, tile) grid on the host, under a sanitizer (tests/test_assign_ref.py
// builds this file with csrc/tdlo_assign_host.cpp, -fsanitize=address,undefined, and runs it).  Every array is allocated at exactly its extent, so a lane that
// reads a node beyond its tile, an offset beyond off[F] or a point beyond the cloud is caught.  For every tile size the owners and distances must be the ones of
// the whole list taken as one tile, bit for bit: the lowest rope wins a tie wherever a tile border falls.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "tdlo_assign_host.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uni() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) * (1.0 / 9007199254740992.0);
}

int main() {
    const int Ms[] = {1, 2, 45, 300, 7, 64, 200};
    const int F = 7;
    const double g26 = 1.0 / 67108864.0;
    std::vector<std::vector<double>> Y(F);
    std::vector<tdlo_assign_rope> ropes(F);
    for (int f = 0; f < F; ++f) {
        const int M = Ms[f];
        Y[f].resize(3 * (size_t)M);
        for (int m = 0; m < M; ++m) {      // on the 2^-26 lattice: ties between ropes are exact
            Y[f][m] = std::round((0.1 + 0.01 * m) / g26) * g26;
            Y[f][M + m] = std::round((0.2 + 0.03 * f) / g26) * g26;
            Y[f][2 * M + m] = std::round(0.6 / g26) * g26;
        }
        ropes[f] = tdlo_assign_rope{f, Y[f].data(), M};
    }
    const int sizes[] = {1, 63, 64, 65, 255, 256, 257, 1025};
    long long points = 0, differing = 0, ties = 0, unowned = 0;
    for (int n : sizes) {
        std::vector<double> X(3 * (size_t)n);
        for (int i = 0; i < n; ++i) {
            const int f = i % F, m = (int)(uni() * Ms[f]);
            const bool tie = i % 5 == 0 && f + 1 < F;      // half way between ropes f and f + 1, on the lattice: equidistant from a node of each
            X[i] = Y[f][m] + (tie ? 0.0 : 0.002 * (uni() - 0.5));
            X[n + i] = tie ? 0.5 * (Y[f][Ms[f] + m] + Y[f + 1][Ms[f + 1]]) : Y[f][Ms[f] + m] + 0.002 * (uni() - 0.5);
            X[2 * (size_t)n + i] = Y[f][2 * Ms[f] + m] + (i % 11 == 3 ? 0.5 : 0.0);
            if (i % 97 == 13) X[i] = NAN;
            if (i % 101 == 17) X[n + i] = INFINITY;
        }
        int total = 0;
        for (int f = 0; f < F; ++f) total += Ms[f];
        std::vector<int> off((size_t)F + 1);
        std::vector<double> Yx(total), Yy(total), Yz(total);
        tdlo::assign_flatten(ropes.data(), F, off.data(), Yx.data(), Yy.data(), Yz.data());
        std::vector<int> want(n), got(n);
        std::vector<double> wd(n), gd(n);
        const double dmax2 = 0.02 * 0.02;
        tdlo::assign_points_host(X.data(), n, off.data(), F, Yx.data(), Yy.data(), Yz.data(), dmax2, total, want.data(), wd.data());
        // the C entry point must agree with the whole-list walk
        std::vector<int> own(n), each(F);
        std::vector<double> d2(n);
        int un = 0;
        if (tdlo_cloud_assign_host(X.data(), n, ropes.data(), F, 0.02, own.data(), d2.data(), each.data(), &un) != TDLO_OK) { printf("refused\n"); return 1; }
        for (int i = 0; i < n; ++i) differing += own[i] != want[i] || std::memcmp(&d2[i], &wd[i], 8) != 0;
        for (int tile : {1, 2, 3, 44, 45, 46, 256, 300, 512, 618, 619, 620}) {
            // (the tiles of the flat list as the kernel stages them: every tile a copy of exactly its extent)
            std::fill(got.begin(), got.end(), -7);
            for (int i = 0; i < n; ++i) {
                double g = INFINITY;
                int o = -1, f = 0;
                for (int t0 = 0; t0 < total; t0 += tile) {
                    const int cnt = total - t0 < tile ? total - t0 : tile;
                    std::vector<double> Lx(Yx.begin() + t0, Yx.begin() + t0 + cnt), Ly(Yy.begin() + t0, Yy.begin() + t0 + cnt), Lz(Yz.begin() + t0, Yz.begin() + t0 + cnt);
                    tdlo::assign_tile(Lx.data(), Ly.data(), Lz.data(), t0, cnt, off.data(), F, f, X[i], X[n + i], X[2 * (size_t)n + i], g, o);
                }
                got[i] = tdlo::assign_gate(g, o, dmax2); gd[i] = g;
            }
            for (int i = 0; i < n; ++i) { ++points; differing += got[i] != want[i] || std::memcmp(&gd[i], &wd[i], 8) != 0; }
        }
        for (int i = 0; i < n; ++i) {
            unowned += want[i] < 0;
            if (i % 5 == 0 && i % F + 1 < F && want[i] >= 0 && i % 11 != 3) ties += want[i] == i % F;
        }
    }
    printf("%lld points, %lld differing, %lld ties to the lower rope, %lld unowned\n", points, differing, ties, unowned);
    return differing ? 1 : 0;
}
