// image_lane_host_test.cpp -- the lane of k_image_import (trackdlo_amd/csrc/tdlo_image_lane.h: the very code the GPU runs) compiled for the host and run
// lane by lane, built with -fsanitize=address,undefined by tests/test_image_view.py and run as an ordinary process: the CPU-side check of the kernel's
// rule -- no load outside a view's extent, every vector load naturally aligned, no store outside the canonical image -- and of its bytes.  The GPU
// build is checked by tests/test_image_view_gpu.py.
//
// usage: image_lane_host_test cases.bin out.bin        (cases.bin as for image_pack_test.cpp)
// Every source is a 16-byte aligned heap block (device allocations are aligned likewise) holding `off` leading bytes and the view's extent, with
// data = block + off - lo; what lies behind the extent up to the block's rounded end is poisoned, and so are the leading bytes when off is 8 (the
// granule of the sanitizer's shadow memory; 1, 2 and 4 leading bytes hold 0xA5, which changes the output if it is used).  The destination is poisoned
// behind the canonical image's last byte.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../trackdlo_amd/csrc/tdlo_image_lane.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#else
#define ASAN_POISON_MEMORY_REGION(a, n) ((void)(a), (void)(n))
#define ASAN_UNPOISON_MEMORY_REGION(a, n) ((void)(a), (void)(n))
#endif

using namespace tdlo;

static size_t round16(size_t n) { return (n + 15) / 16 * 16; }

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]); return 2; }
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    long long n = 0;
    if (std::fread(&n, 8, 1, in) != 1) return 2;
    long long forms[3] = {0, 0, 0};
    for (long long k = 0; k < n; ++k) {
        long long h[8];
        if (std::fread(h, 8, 8, in) != 8) return 2;
        const int format = (int)h[0], role = (int)h[1], rows = (int)h[2], cols = (int)h[3];
        const long long stride = h[4], off = h[5], lo = h[6], hi = h[7];
        const size_t used = (size_t)(off + hi - lo), room = round16(used);
        unsigned char *block = (unsigned char *)std::aligned_alloc(16, room);
        if (!block) return 2;
        std::memset(block, 0xA5, (size_t)off);
        if (std::fread(block + off, 1, (size_t)(hi - lo), in) != (size_t)(hi - lo)) return 2;
        if (off && off % 8 == 0) ASAN_POISON_MEMORY_REGION(block, (size_t)off);
        if (room > used) ASAN_POISON_MEMORY_REGION(block + used, room - used);
        const int P = rows * cols;
        const size_t bytes = (size_t)P * (role == kRoleDepth ? 2 : role == kRoleColour ? 3 : 1);
        unsigned char *canon = (unsigned char *)std::aligned_alloc(16, round16(bytes));
        if (!canon) return 2;
        if (round16(bytes) > bytes) ASAN_POISON_MEMORY_REGION(canon + bytes, round16(bytes) - bytes);
        ImageJob job{};
        job.P = P; job.cols = cols;
        const unsigned char *data = block + off - lo;
        const int form = image_import_form(data, stride, cols, format);
        ++forms[form];
        job.src[role] = ImageSrc{data, stride, format, form};
        job.dst[role] = canon;
        const int lanes = ((P + 3) / 4 + 255) / 256 * 256;          // whole workgroups, as launched: the spare lanes return
        for (int t = 0; t < lanes; ++t) image_import_lane(job, t);
        if (std::fwrite(canon, 1, bytes, out) != bytes) return 2;
        ASAN_UNPOISON_MEMORY_REGION(canon, round16(bytes));
        std::free(canon);
        ASAN_UNPOISON_MEMORY_REGION(block, room);
        std::free(block);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    std::printf("%lld cases imported; forms element / dwords / wide: %lld %lld %lld\n", n, forms[0], forms[1], forms[2]);
    return 0;
}
