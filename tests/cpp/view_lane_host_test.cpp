// view_lane_host_test.cpp -- the lane of k_cloud_team's phase A over a cloud view (trackdlo_amd/csrc/tdlo_view_lane.h: the very code the GPU runs) compiled
// for the host and run lane by lane, every lane of every tile of 4096 elements; built with -fsanitize=address,undefined by tests/test_view_team_ref.py and
// run as an ordinary process.  The CPU-side check of the lane's rule -- no load of any width outside the view's extent nor outside [select, select + N),
// every vector load naturally aligned -- and of what it keeps.  The GPU build is checked by tests/test_view_team_gpu.py.
//
// usage: view_lane_host_test cases.bin out.bin
// cases.bin: int64 count, then per case eight int64 {f64, form, N, stride_point, stride_comp, data_off, elems, lead} + {sel_off} (-1: no selection), the
// extent's `elems` elements, and N selection bytes when there is a selection.  The view's block is 16-byte aligned (device allocations are aligned
// likewise): `lead` bytes (0, 4 or 8: what the layout's alignment asks for) in front of the extent, data = extent + data_off elements; poisoned behind the
// extent's last byte, and in front of it when lead is 8 (the granule of the sanitizer's shadow memory; 4 leading bytes hold 0xA5, a finite float that
// changes the output if it is used).  The selection lies at 8 + sel_off bytes into its block, the 8 poisoned, the sel_off bytes in front of it 0xA5 (a set
// byte: an aligned load that reaches below `select` selects an element wrongly), poisoned behind its N-th byte.
// out.bin, per case: N kept flags (bytes), then N x 3 floats (0 where not kept).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <vector>

#include "../../trackdlo_amd/csrc/tdlo_view_lane.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#else
#define ASAN_POISON_MEMORY_REGION(a, n) ((void)(a), (void)(n))
#define ASAN_UNPOISON_MEMORY_REGION(a, n) ((void)(a), (void)(n))
#endif

using namespace tdlo;

static size_t round16(size_t n) { return (n + 15) / 16 * 16; }

template <typename T, int FORM>
static bool run_case(const T *data, long long sp, long long sc, const unsigned char *sel, int N, unsigned char *kept, float *xyz) {
    const int T_ = (N + 4095) / 4096;
    for (int b = 0; b < T_; ++b)
        for (int t = 0; t < 1024; ++t) {
            const int p0 = 4096 * b + 4 * t;
            float x[4], y[4], z[4];
            const unsigned keep = view_lane4<T, FORM>(data, sp, sc, sel, p0, N, x, y, z);
            for (int k = 0; k < 4; ++k) {
                const bool on = (keep >> k) & 1u;
                if (p0 + k >= N) { if (on) return false; continue; }         // nothing beyond the view is kept
                kept[p0 + k] = on ? 1 : 0;
                xyz[3 * (size_t)(p0 + k)] = on ? x[k] : 0.0f; xyz[3 * (size_t)(p0 + k) + 1] = on ? y[k] : 0.0f; xyz[3 * (size_t)(p0 + k) + 2] = on ? z[k] : 0.0f;
            }
            if (keep >> 4) return false;
        }
    return true;
}

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]); return 2; }
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    long long n = 0;
    if (std::fread(&n, 8, 1, in) != 1) return 2;
    long long forms[4] = {0, 0, 0, 0};
    for (long long c = 0; c < n; ++c) {
        long long h[9];
        if (std::fread(h, 8, 9, in) != 9) return 2;
        const bool f64 = h[0] != 0;
        const int form = (int)h[1], N = (int)h[2];
        const long long sp = h[3], sc = h[4], data_off = h[5], elems = h[6], lead = h[7], sel_off = h[8];
        const size_t es = f64 ? 8 : 4, used = (size_t)lead + (size_t)elems * es, room = round16(used);
        unsigned char *block = (unsigned char *)std::aligned_alloc(16, room);
        if (!block) return 2;
        std::memset(block, 0xA5, (size_t)lead);
        if (std::fread(block + lead, es, (size_t)elems, in) != (size_t)elems) return 2;
        if (lead == 8) ASAN_POISON_MEMORY_REGION(block, 8);
        if (room > used) ASAN_POISON_MEMORY_REGION(block + used, room - used);
        const unsigned char *data = block + lead + data_off * (long long)es;
        unsigned char *sblock = nullptr;
        const unsigned char *sel = nullptr;
        size_t sroom = 0;
        if (sel_off >= 0) {
            const size_t sused = 8 + (size_t)sel_off + (size_t)N;
            sroom = round16(sused);
            sblock = (unsigned char *)std::aligned_alloc(16, sroom);
            if (!sblock) return 2;
            std::memset(sblock, 0xA5, 8 + (size_t)sel_off);
            if (std::fread(sblock + 8 + sel_off, 1, (size_t)N, in) != (size_t)N) return 2;
            ASAN_POISON_MEMORY_REGION(sblock, 8);
            if (sroom > sused) ASAN_POISON_MEMORY_REGION(sblock + sused, sroom - sused);
            sel = sblock + 8 + sel_off;
        }
        // the form must be one that the host's rule (cloud_import_form) may choose for this view
        bool ok = form == kGeneric || (!f64 && form == kXyz12 && sc == 1 && (sp == 3 || sp == 4 || sp == 8)) ||
                  (!f64 && form == kCols2 && sp == 1 && sc % 2 == 0 && (uintptr_t)data % 8 == 0);
        if (!ok) { std::fprintf(stderr, "case %lld: form %d does not fit the view\n", c, form); return 3; }
        std::vector<unsigned char> kept((size_t)N, 0xEE);
        std::vector<float> xyz(3 * (size_t)N, -1.0f);
        if (f64) ok = run_case<double, kGeneric>((const double *)data, sp, sc, sel, N, kept.data(), xyz.data());
        else if (form == kXyz12) ok = run_case<float, kXyz12>((const float *)data, sp, sc, sel, N, kept.data(), xyz.data());
        else if (form == kCols2) ok = run_case<float, kCols2>((const float *)data, sp, sc, sel, N, kept.data(), xyz.data());
        else ok = run_case<float, kGeneric>((const float *)data, sp, sc, sel, N, kept.data(), xyz.data());
        if (!ok) { std::fprintf(stderr, "case %lld: an element beyond the view is kept\n", c); return 3; }
        ++forms[f64 ? 3 : form];
        if (std::fwrite(kept.data(), 1, kept.size(), out) != kept.size() || std::fwrite(xyz.data(), 4, xyz.size(), out) != xyz.size()) return 2;
        ASAN_UNPOISON_MEMORY_REGION(block, room);
        std::free(block);
        if (sblock) { ASAN_UNPOISON_MEMORY_REGION(sblock, sroom); std::free(sblock); }
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    std::printf("%lld cases run; forms generic / xyz12 / cols2 / f64: %lld %lld %lld %lld\n", n, forms[0], forms[1], forms[2], forms[3]);
    return 0;
}
