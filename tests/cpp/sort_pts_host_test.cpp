// sort_pts_host (csrc/tdlo_host.cpp) in a stand-alone program, built by tests/test_init_ref.py with -fsanitize=address,undefined and run as a
// child process of its own: every case's nodes and outputs are heap blocks of exactly their sizes, so an access outside them is a report.
//   cases file:  int64 count, then per case int64 M and 3 M doubles (column-major)
//   output file: per case int64 status, and for status 0 the sorted nodes (3 M doubles), perm (M int32) and coord (M doubles)
// A second pass sorts every case in place (Y_sorted == Y) and without perm and coord, and must give the same nodes.
#include "tdlo_host.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int64_t count = 0;
    if (std::fread(&count, 8, 1, in) != 1) return 2;
    for (int64_t k = 0; k < count; ++k) {
        int64_t M = 0;
        if (std::fread(&M, 8, 1, in) != 1 || M < 2) return 2;
        double *Y = new double[3 * M], *Ys = new double[3 * M], *coord = new double[M];
        int32_t *perm = new int32_t[M];
        if (std::fread(Y, 8, 3 * M, in) != (size_t)(3 * M)) return 2;
        std::memset(Ys, 0xff, 24 * M); std::memset(coord, 0xff, 8 * M); std::memset(perm, 0xff, 4 * M);
        const int64_t status = tdlo::sort_pts_host(Y, (int)M, Ys, perm, coord);
        std::fwrite(&status, 8, 1, out);
        if (status == 0) {
            std::fwrite(Ys, 8, 3 * M, out); std::fwrite(perm, 4, M, out); std::fwrite(coord, 8, M, out);
            if (tdlo::sort_pts_host(Y, (int)M, Y, nullptr, nullptr) != 0 || std::memcmp(Y, Ys, 24 * M) != 0) { std::printf("case %lld: in place differs\n", (long long)k); return 1; }
        } else {
            // a refused input leaves the outputs untouched
            for (int64_t i = 0; i < 24 * M; ++i) if (((unsigned char *)Ys)[i] != 0xff) { std::printf("case %lld: outputs touched\n", (long long)k); return 1; }
        }
        delete[] Y; delete[] Ys; delete[] coord; delete[] perm;
    }
    std::fclose(in); std::fclose(out);
    std::printf("%lld cases sorted\n", (long long)count);
    return 0;
}
