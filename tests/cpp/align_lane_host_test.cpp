// align_lane_host_test.cpp -- the lanes of k_align_splat and k_align_pack (csrc/tdlo_align_lane.h) compiled for the host and run over the kernels' whole
// (workgroup, lane) grids -- the partly filled last workgroup's spare lanes included -- under AddressSanitizer and UBSan, with the depth view, the scratch
// plane and the output allocated at EXACTLY their extents: a load outside the view, an offer outside the plane or a pack access past its end is a report.
// Built from this file, tdlo_align_host.cpp and tdlo_image_host.cpp (no HIP) by tests/test_align_ref.py, which writes the scenes and the values the numpy
// statement gives for them to a file:  int32 scenes, then per scene
//   int32 rows_d, cols_d, rows_c, cols_c, format, has_T, max_footprint, layout (0 packed, 1 pitched, 2 bottom-up)
//   double fx_d, fy_d, cx_d, cy_d, fx_c, fy_c, cx_c, cy_c, T[12]
//   the depth image packed (2 or 4 bytes an element), the expected plane (uint16), int64 counts[4]
#include "tdlo_align_host.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: align_lane_host_test <scene file>\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    int32_t S = 0;
    if (!rd(f, &S, 4)) return 2;
    long long words = 0, differing = 0, lanes = 0;
    for (int s = 0; s < S; ++s) {
        int32_t h[8];
        double g[20];
        if (!rd(f, h, sizeof h) || !rd(f, g, sizeof g)) return 2;
        const int rows_d = h[0], cols_d = h[1], rows_c = h[2], cols_c = h[3], format = h[4], has_T = h[5], layout = h[7];
        const size_t es = format == TDLO_IMG_F32C1 ? 4 : 2, Pd = (size_t)rows_d * cols_d, Pc = (size_t)rows_c * cols_c;
        std::vector<unsigned char> packed(Pd * es);
        std::vector<unsigned short> want(Pc);
        long long want_n[4];
        if (!rd(f, packed.data(), Pd * es) || !rd(f, want.data(), 2 * Pc) || !rd(f, want_n, sizeof want_n)) return 2;
        // the view at exactly its extent: a pitched view ends with its last row's last pixel, a bottom-up view starts at its last row
        const size_t pitch = (layout ? (size_t)cols_d + 3 : (size_t)cols_d) * es, extent = (size_t)(rows_d - 1) * pitch + (size_t)cols_d * es;
        unsigned char *buf = static_cast<unsigned char *>(std::malloc(extent));
        std::memset(buf, 0x11, extent);
        for (int r = 0; r < rows_d; ++r) std::memcpy(buf + (size_t)(layout == 2 ? rows_d - 1 - r : r) * pitch, packed.data() + (size_t)r * cols_d * es, (size_t)cols_d * es);
        tdlo_image_view view{layout == 2 ? buf + (size_t)(rows_d - 1) * pitch : buf, format, TDLO_MEM_HOST, layout == 2 ? -(long long)pitch : (long long)pitch, nullptr};
        tdlo_align_params p{rows_d, cols_d, g[0], g[1], g[2], g[3], rows_c, cols_c, g[4], g[5], g[6], g[7], has_T ? g + 8 : nullptr, h[6]};
        if (tdlo_align_check(&p) || tdlo_image_view_check(&view, rows_d, cols_d, TDLO_ROLE_DEPTH)) { std::fprintf(stderr, "scene %d refused\n", s); return 1; }
        unsigned *scratch = static_cast<unsigned *>(::operator new(Pc * 4, std::align_val_t(16)));
        unsigned short *out = static_cast<unsigned short *>(::operator new(Pc * 2, std::align_val_t(8)));
        long long n[4];
        tdlo::AlignJob job;
        tdlo::align_job(&view, &p, job);
        tdlo::align_depth_host(job, scratch, out, n);                      // the two grids, lane by lane
        lanes += (long long)((Pd + 255) / 256 + ((Pc + 3) / 4 + 255) / 256) * 256;
        for (size_t i = 0; i < Pc; ++i) { differing += out[i] != want[i]; differing += scratch[i] != tdlo::kAlignEmpty; }      // ... and the scratch is armed again
        for (int i = 0; i < 4; ++i) differing += n[i] != want_n[i];
        // the exported call, its output at an address aligned to 2 bytes only
        std::vector<unsigned short> odd(Pc + 1);
        if (tdlo_align_depth_host(&view, &p, odd.data() + 1, n)) return 1;
        for (size_t i = 0; i < Pc; ++i) differing += odd[i + 1] != want[i];
        words += (long long)Pc;
        ::operator delete(out, std::align_val_t(8));
        ::operator delete(scratch, std::align_val_t(16));
        std::free(buf);
    }
    std::fclose(f);
    std::printf("%d scenes, %lld lanes, %lld words, %lld differing\n", (int)S, lanes, words, differing);
    return differing ? 1 : 0;
}
