// image_batch_lane_host_test.cpp -- what k_image_import_batch (trackdlo_amd/csrc/tdlo_image.hip) does with its table, on the host: workgroup (x, y) runs
// image_import_lane(table[y], x * 256 + thread) -- the very lane the GPU runs (tdlo_image_lane.h).  Built with -fsanitize=address,undefined by
// tests/test_frame_view_batch_cpu.py and run as an ordinary process; nothing of it is loaded into python.
//
// usage: image_batch_lane_host_test table.bin out.bin
// table.bin: K, rows, cols (int64 each), then per job: its number of planes, and per plane eight int64 {format, role, row_stride, off, lo, hi, 0, 0} and
// the hi - lo bytes of the view's extent.  Every source is a 16-byte aligned heap block holding `off` leading bytes and the extent, data = block + off - lo;
// the bytes behind the extent up to the block's rounded end are poisoned for the sanitizer, and so are the leading bytes when off is a multiple of 8.
// Every destination stands between 16 canary bytes in front and at least 16 behind its last byte.  The whole grid runs -- every y, every lane of whole
// workgroups -- then each plane is compared with image_pack_host on the same view, the canaries are checked, and the bytes go to out.bin (job by job,
// plane by plane) for the numpy statement.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../trackdlo_amd/csrc/tdlo_image_lane.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#else
#define ASAN_POISON_MEMORY_REGION(a, n) ((void)(a), (void)(n))
#define ASAN_UNPOISON_MEMORY_REGION(a, n) ((void)(a), (void)(n))
#endif

using namespace tdlo;

static size_t round16(size_t n) { return (n + 15) / 16 * 16; }
constexpr unsigned char kCanary = 0xC3;
constexpr int kLanesPerGroup = 256;          // kBlock

struct Plane { unsigned char *block, *dst_block; size_t room, bytes, dst_room; tdlo_image_view view; int role, form; };

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s table.bin out.bin\n", argv[0]); return 2; }
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    long long head[3];
    if (std::fread(head, 8, 3, in) != 3) return 2;
    const int K = (int)head[0], rows = (int)head[1], cols = (int)head[2], P = rows * cols;
    std::vector<ImageJob> table(K);
    std::vector<std::vector<Plane>> planes(K);
    long long forms[3] = {0, 0, 0};
    for (int k = 0; k < K; ++k) {
        long long np = 0;
        if (std::fread(&np, 8, 1, in) != 1) return 2;
        table[k] = ImageJob{};
        table[k].P = P; table[k].cols = cols;
        for (long long q = 0; q < np; ++q) {
            long long h[8];
            if (std::fread(h, 8, 8, in) != 8) return 2;
            Plane pl{};
            const int format = (int)h[0];
            pl.role = (int)h[1];
            const long long stride = h[2], off = h[3], lo = h[4], hi = h[5];
            const size_t used = (size_t)(off + hi - lo);
            pl.room = round16(used);
            pl.block = (unsigned char *)std::aligned_alloc(16, pl.room);
            if (!pl.block) return 2;
            std::memset(pl.block, 0xA5, (size_t)off);
            if (std::fread(pl.block + off, 1, (size_t)(hi - lo), in) != (size_t)(hi - lo)) return 2;
            if (off && off % 8 == 0) ASAN_POISON_MEMORY_REGION(pl.block, (size_t)off);
            if (pl.room > used) ASAN_POISON_MEMORY_REGION(pl.block + used, pl.room - used);
            pl.bytes = (size_t)P * (pl.role == kRoleDepth ? 2 : pl.role == kRoleColour ? 3 : 1);
            pl.dst_room = 16 + round16(pl.bytes) + 16;
            pl.dst_block = (unsigned char *)std::aligned_alloc(16, pl.dst_room);
            if (!pl.dst_block) return 2;
            std::memset(pl.dst_block, kCanary, pl.dst_room);
            const unsigned char *data = pl.block + off - lo;
            pl.view = tdlo_image_view{data, format, TDLO_MEM_HOST, stride, nullptr};
            pl.form = image_import_form(data, stride, cols, format);
            ++forms[pl.form];
            if (table[k].src[pl.role].data) { std::fprintf(stderr, "job %d: role %d twice\n", k, pl.role); return 2; }
            table[k].src[pl.role] = ImageSrc{data, stride, format, pl.form};
            table[k].dst[pl.role] = pl.dst_block + 16;
            planes[k].push_back(pl);
        }
    }
    std::fclose(in);
    // the grid as launched: x over whole workgroups of the image's lanes, y over the jobs
    const int groups = ((P + 3) / 4 + kLanesPerGroup - 1) / kLanesPerGroup;
    for (int y = 0; y < K; ++y)
        for (int x = 0; x < groups; ++x)
            for (int t = 0; t < kLanesPerGroup; ++t) image_import_lane(table[y], x * kLanesPerGroup + t);
    int bad = 0;
    for (int k = 0; k < K; ++k)
        for (Plane &pl : planes[k]) {
            std::vector<unsigned char> want(pl.bytes);
            image_pack_host(&pl.view, rows, cols, want.data());
            if (std::memcmp(want.data(), pl.dst_block + 16, pl.bytes)) { std::fprintf(stderr, "job %d role %d: differs from image_pack_host\n", k, pl.role); ++bad; }
            for (size_t b = 0; b < pl.dst_room; ++b)
                if ((b < 16 || b >= 16 + pl.bytes) && pl.dst_block[b] != kCanary) { std::fprintf(stderr, "job %d role %d: canary byte %zu written\n", k, pl.role, b); ++bad; break; }
            if (std::fwrite(pl.dst_block + 16, 1, pl.bytes, out) != pl.bytes) return 2;
            ASAN_UNPOISON_MEMORY_REGION(pl.block, pl.room);
            std::free(pl.block);
            std::free(pl.dst_block);
        }
    if (std::fclose(out) != 0) return 2;
    if (bad) return 1;
    std::printf("%d jobs imported over a grid of %d x %d workgroups; forms element / dwords / wide: %lld %lld %lld\n", K, groups, K, forms[0], forms[1], forms[2]);
    return 0;
}
