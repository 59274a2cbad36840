// tdlo_image_lane.h -- what one lane of k_image_import (tdlo_image.hip) does: its four pixels of every image of the frame, loaded in the form the host
// chose and stored as canonical bytes.  A header of its own so that the very code the GPU runs can be compiled for the host and run lane by lane
// under a sanitizer, on sources allocated at exactly their extents (tests/cpp/image_lane_host_test.cpp) -- the rule of tdlo_image.hip, no load outside
// a view's extent and every vector load naturally aligned, is checked there without a GPU.
#pragma once
#include "tdlo_image.h"

namespace tdlo {

struct alignas(8) ImgU2 { unsigned x, y; };                  // one 8-byte / 16-byte access
struct alignas(16) ImgU4 { unsigned x, y, z, w; };

TDLO_HD inline unsigned ld32(const unsigned char *p) { return *reinterpret_cast<const unsigned *>(p); }

// three bytes of each of four 4-channel pixels -> 12 packed bytes
TDLO_HD inline void drop_alpha(unsigned a, unsigned b, unsigned c, unsigned d, unsigned o[3]) {
    a &= 0xffffffu; b &= 0xffffffu; c &= 0xffffffu; d &= 0xffffffu;
    o[0] = a | (b << 24); o[1] = (b >> 8) | (c << 16); o[2] = (c >> 16) | (d << 8);
}

TDLO_HD inline unsigned mm_of_bits(unsigned w) { float d; __builtin_memcpy(&d, &w, 4); return (unsigned)image_f32_to_mm(d); }

// one image's four pixels p0 .. p0 + 3 (those below P) as little-endian canonical bytes in o[0 .. words): U8C1 1 word, U16C1 / F32C1 2, U8C3 / U8C4 3
TDLO_HD inline void load4(const ImageSrc &s, int p0, int P, int cols, int i0, int j0, unsigned o[3]) {
    const int bpp = image_bpp(s.format);
    if (s.form != kImgElem) {                                    // the four pixels lie in row i0, at a 4-byte aligned address (cols % 4 == 0)
        const unsigned char *q = s.data + (long long)i0 * s.row_stride + (long long)j0 * bpp;
        switch (s.format) {
        case TDLO_IMG_U8C1: o[0] = ld32(q); break;
        case TDLO_IMG_U8C3: o[0] = ld32(q); o[1] = ld32(q + 4); o[2] = ld32(q + 8); break;
        case TDLO_IMG_U16C1:
            if (s.form == kImgWide) { const ImgU2 v = *reinterpret_cast<const ImgU2 *>(q); o[0] = v.x; o[1] = v.y; }
            else { o[0] = ld32(q); o[1] = ld32(q + 4); }
            break;
        default: {                                               // U8C4, F32C1: 16 bytes
            ImgU4 v;
            if (s.form == kImgWide) v = *reinterpret_cast<const ImgU4 *>(q);
            else { v.x = ld32(q); v.y = ld32(q + 4); v.z = ld32(q + 8); v.w = ld32(q + 12); }
            if (s.format == TDLO_IMG_U8C4) drop_alpha(v.x, v.y, v.z, v.w, o);
            else { o[0] = mm_of_bits(v.x) | (mm_of_bits(v.y) << 16); o[1] = mm_of_bits(v.z) | (mm_of_bits(v.w) << 16); }
        }
        }
        return;
    }
    unsigned px[4] = {0u, 0u, 0u, 0u};                           // per pixel: its canonical bytes (1, 2 or 3 of them)
    int i = i0, j = j0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (p0 + k < P) {
            const unsigned char *q = s.data + (long long)i * s.row_stride + (long long)j * bpp;
            switch (s.format) {
            case TDLO_IMG_U8C1: px[k] = q[0]; break;
            case TDLO_IMG_U16C1: px[k] = *reinterpret_cast<const unsigned short *>(q); break;
            case TDLO_IMG_F32C1: px[k] = mm_of_bits(*reinterpret_cast<const unsigned *>(q)); break;
            default: px[k] = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16); break;      // U8C3, U8C4: the pixel's first three bytes
            }
        }
        if (++j == cols) { j = 0; ++i; }
    }
    if (bpp == 1) o[0] = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
    else if (s.format == TDLO_IMG_U16C1 || s.format == TDLO_IMG_F32C1) { o[0] = px[0] | (px[1] << 16); o[1] = px[2] | (px[3] << 16); }
    else drop_alpha(px[0], px[1], px[2], px[3], o);
}

// canonical bytes of pixels p0 .. p0 + 3 (those below P), `bytes` per pixel, at dst + p0 * bytes
TDLO_HD inline void store4(unsigned char *dst, int p0, int P, int bytes, const unsigned o[3]) {
    unsigned char *q = dst + (size_t)p0 * bytes;
    if (p0 + 4 <= P) {
        unsigned *w = reinterpret_cast<unsigned *>(q);
        if (bytes == 2) *reinterpret_cast<ImgU2 *>(q) = ImgU2{o[0], o[1]};
        else { w[0] = o[0]; if (bytes == 3) { w[1] = o[1]; w[2] = o[2]; } }
        return;
    }
    const int n = (P - p0) * bytes;                              // the image's last 1 .. 3 pixels: nothing behind them is written
#pragma unroll
    for (int b = 0; b < 9; ++b)
        if (b < n) q[b] = (unsigned char)(o[b >> 2] >> (8 * (b & 3)));
}

// lane t of the launch: pixels 4 t .. 4 t + 3 of every image the job holds
TDLO_HD inline void image_import_lane(const ImageJob &job, int t) {
    if (t >= (job.P + 3) / 4) return;                            // (before 4 t: P is up to 2^26, 4 t of a spare lane could pass 2^31)
    const int p0 = 4 * t, i0 = p0 / job.cols, j0 = p0 - i0 * job.cols;
    unsigned o[3];
    for (int r = kRoleDepth; r <= kRoleMask; ++r)
        if (job.src[r].data) { load4(job.src[r], p0, job.P, job.cols, i0, j0, o); store4(job.dst[r], p0, job.P, r == kRoleDepth ? 2 : r == kRoleColour ? 3 : 1, o); }
}

}  // namespace tdlo
