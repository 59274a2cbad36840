// rig_host_test.cpp -- the host half of a rig (trackdlo_amd/csrc/tdlo_rig_host.cpp) and, through it, the lane of phase A over a rig's images
// (csrc/tdlo_rig_point.h: the very code the GPU runs) in a stand-alone program, built by tests/test_rig_ref.py with -fsanitize=address,undefined and run as
// a child process.  Every plane is allocated at EXACTLY its extent (rows x cols elements, nothing behind it), so a load beyond a plane is a sanitizer report.
//
//   rig_host_test cases.bin out.bin
// cases.bin: int64 count; per case int64 K, rows, cols; per camera int64 has_mask, has_colour, has_occluder, has_T, 4 doubles fx fy cx cy, 12 doubles
//            cam_to_rig, 26 int32 of tdlo_colour_params (n_ranges, lower[4][3], upper[4][3], rgb_order), then the planes that are there: depth, mask,
//            colour, occluder.
// out.bin:   per case int64 rc of tdlo_rig_check, int64 n_raw, 3 n_raw floats (R).
#include "../../trackdlo_amd/csrc/tdlo_rig_host.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: rig_host_test cases.bin out.bin\n"); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int64_t count = 0;
    if (!rd(in, &count, 8)) return 2;
    long long total = 0;
    for (int64_t ci = 0; ci < count; ++ci) {
        int64_t hdr[3];
        if (!rd(in, hdr, sizeof hdr)) return 2;
        const int K = (int)hdr[0], rows = (int)hdr[1], cols = (int)hdr[2];
        const size_t P = (size_t)rows * cols;
        std::vector<tdlo_rig_camera> cams(K);
        std::vector<tdlo_colour_params> cps(K);
        std::vector<std::unique_ptr<double[]>> Ts;
        std::vector<std::unique_ptr<unsigned short[]>> depths;
        std::vector<std::unique_ptr<unsigned char[]>> bytes;
        for (int k = 0; k < K; ++k) {
            int64_t has[4];
            double cam[4], T[12];
            int32_t cp[26];
            if (!rd(in, has, sizeof has) || !rd(in, cam, sizeof cam) || !rd(in, T, sizeof T) || !rd(in, cp, sizeof cp)) return 2;
            tdlo_rig_camera &c = cams[k];
            std::memset(&c, 0, sizeof c);
            c.fx = cam[0]; c.fy = cam[1]; c.cx = cam[2]; c.cy = cam[3];
            if (has[3]) { Ts.emplace_back(new double[12]); std::memcpy(Ts.back().get(), T, sizeof T); c.cam_to_rig = Ts.back().get(); }
            tdlo_colour_params &q = cps[k];
            q.n_ranges = cp[0]; std::memcpy(q.lower, cp + 1, 12 * 4); std::memcpy(q.upper, cp + 13, 12 * 4); q.rgb_order = cp[25];
            depths.emplace_back(new unsigned short[P]);                                   // exactly the plane
            if (!rd(in, depths.back().get(), 2 * P)) return 2;
            c.depth = depths.back().get();
            if (has[0]) { bytes.emplace_back(new unsigned char[P]); if (!rd(in, bytes.back().get(), P)) return 2; c.mask = bytes.back().get(); }
            if (has[1]) { bytes.emplace_back(new unsigned char[3 * P]); if (!rd(in, bytes.back().get(), 3 * P)) return 2; c.colour = bytes.back().get(); c.colour_params = &q; }
            if (has[2]) { bytes.emplace_back(new unsigned char[P]); if (!rd(in, bytes.back().get(), P)) return 2; c.occluder = bytes.back().get(); }
        }
        const int64_t rc = tdlo_rig_check(cams.data(), K, rows, cols, 0.008);
        int n = 0;
        std::vector<float> R;
        if (rc == 0) {
            if (tdlo_rig_points_host(cams.data(), K, rows, cols, nullptr, 0, &n) != 0) { fprintf(stderr, "case %lld: count failed\n", (long long)ci); return 1; }
            R.resize(3 * (size_t)n);                                                      // exactly R
            int n2 = 0;
            if (tdlo_rig_points_host(cams.data(), K, rows, cols, R.data(), n, &n2) != 0 || n2 != n) { fprintf(stderr, "case %lld: points failed\n", (long long)ci); return 1; }
            if (n > 0 && tdlo_rig_points_host(cams.data(), K, rows, cols, R.data(), n - 1, &n2) == 0) { fprintf(stderr, "case %lld: a short R_out was not refused\n", (long long)ci); return 1; }
        }
        const int64_t n64 = n;
        fwrite(&rc, 8, 1, out); fwrite(&n64, 8, 1, out);
        if (n) fwrite(R.data(), 4, R.size(), out);
        total += n;
    }
    fclose(in); fclose(out);
    printf("%lld cases run, %lld points\n", (long long)count, total);
    return 0;
}
