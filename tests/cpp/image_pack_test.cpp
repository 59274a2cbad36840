// image_pack_test.cpp -- the host half of image views (trackdlo_amd/csrc/tdlo_image_host.cpp: check, extent, pack and convert) driven from a stand-alone
// program, so that it can be built with -fsanitize=address,undefined and run as an ordinary process (tests/test_image_view.py builds and runs it; it
// links nothing but that one translation unit: no HIP, no GPU).
//
// usage: image_pack_test cases.bin out.bin
// cases.bin: int64 n, then per case eight int64 {format, role, rows, cols, row_stride, off, lo, hi} followed by the hi - lo bytes of the view's extent.
// Every source is a heap block of exactly off + (hi - lo) bytes with data = block + off - lo: `off` (0, 1, 2, 4, 8) sets data's alignment; the extent
// ends where the block ends and, for off 0 and 8 (the granule of the sanitizer's shadow memory), starts where the addressable bytes start, so a load
// outside the extent is a report.  For off 1, 2 and 4 the bytes in front hold 0xA5, which changes the output if it is used.  The destination is a heap
// block of exactly the canonical size.  out.bin: the canonical images, one behind the other.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/trackdlo_hip.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#else
#define ASAN_POISON_MEMORY_REGION(a, n) ((void)(a), (void)(n))
#define ASAN_UNPOISON_MEMORY_REGION(a, n) ((void)(a), (void)(n))
#endif

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]); return 2; }
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    long long n = 0;
    if (std::fread(&n, 8, 1, in) != 1) return 2;
    for (long long k = 0; k < n; ++k) {
        long long h[8];
        if (std::fread(h, 8, 8, in) != 8) return 2;
        const int format = (int)h[0], role = (int)h[1], rows = (int)h[2], cols = (int)h[3];
        const long long stride = h[4], off = h[5], lo = h[6], hi = h[7];
        unsigned char *block = (unsigned char *)std::malloc((size_t)(off + hi - lo));
        if (!block) return 2;
        std::memset(block, 0xA5, (size_t)off);
        if (std::fread(block + off, 1, (size_t)(hi - lo), in) != (size_t)(hi - lo)) return 2;
        if (off && off % 8 == 0) ASAN_POISON_MEMORY_REGION(block, (size_t)off);
        tdlo_image_view v;
        v.data = block + off - lo; v.format = format; v.location = TDLO_MEM_HOST; v.row_stride = stride; v.ready_stream = nullptr;
        long long lo2 = 1, hi2 = -1;
        if (tdlo_image_view_check(&v, rows, cols, role) != 0 || tdlo_image_view_extent(&v, rows, cols, &lo2, &hi2) != 0 || lo2 != lo || hi2 != hi) {
            std::fprintf(stderr, "case %lld: check / extent disagree: [%lld, %lld) against [%lld, %lld)\n", k, lo2, hi2, lo, hi);
            return 1;
        }
        const size_t bytes = (size_t)rows * cols * (role == TDLO_ROLE_DEPTH ? 2 : role == TDLO_ROLE_COLOUR ? 3 : 1);
        unsigned char *canon = (unsigned char *)std::malloc(bytes);
        if (!canon) return 2;
        if (tdlo_image_view_pack(&v, rows, cols, role, canon) != 0) { std::fprintf(stderr, "case %lld: pack refused\n", k); return 1; }
        if (std::fwrite(canon, 1, bytes, out) != bytes) return 2;
        std::free(canon);
        if (off && off % 8 == 0) ASAN_UNPOISON_MEMORY_REGION(block, (size_t)off);
        std::free(block);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    std::printf("%lld cases packed\n", n);
    return 0;
}
