// tdlo_image.h -- image views (tdlo_image_view): what the host pieces (tdlo_image_host.cpp, no HIP) and the import kernel (tdlo_image.hip) share.
#pragma once
#include <stddef.h>
#include "../../include/trackdlo_hip.h"

#if defined(__HIPCC__)
#define TDLO_HD __host__ __device__
#else
#define TDLO_HD
#endif

namespace tdlo {

enum ImageRole { kRoleDepth = 0, kRoleColour = 1, kRoleOccluder = 2, kRoleMask = 3 };
// how a lane of k_image_import loads its four pixels of one image (image_import_form)
enum ImageForm { kImgElem = 0,       // element by element; each pixel computes its own (row, column)
                 kImgDwords = 1,     // cols % 4 == 0, data and row_stride multiples of 4: the four pixels as 1 (U8C1), 2 (U16C1), 3 (U8C3) or 4 (U8C4, F32C1) dword loads
                 kImgWide = 2 };     // ... multiples of 8 (U16C1) / 16 (U8C4, F32C1): ONE 8- / 16-byte load

// bytes per pixel and per element; 0: no such format
TDLO_HD inline int image_bpp(int format) {
    return format == TDLO_IMG_U8C1 ? 1 : format == TDLO_IMG_U8C3 ? 3 : format == TDLO_IMG_U8C4 ? 4 : format == TDLO_IMG_U16C1 ? 2 : format == TDLO_IMG_F32C1 ? 4 : 0;
}
TDLO_HD inline int image_elem(int format) { return format == TDLO_IMG_U16C1 ? 2 : format == TDLO_IMG_F32C1 ? 4 : format >= TDLO_IMG_U8C1 && format <= TDLO_IMG_U8C4 ? 1 : 0; }

// 32FC1 metres -> uint16 millimetres (the rule of include/trackdlo_hip.h): floor(1000 d + 1/2) where that lies in [0, 65536), else 0.  The product and
// the sum are exact in fp64 wherever the result can depend on them, so a fused multiply-add gives the same bits.
TDLO_HD inline unsigned short image_f32_to_mm(float d) {
    const double x = (double)d * 1000.0 + 0.5;
    return (x >= 0.0 && x < 65536.0) ? (unsigned short)(int)x : (unsigned short)0;      // (x >= 0: truncation is floor; NaN fails both comparisons)
}

// One launch of k_image_import (tdlo_image.hip): per role a device source (data == nullptr: that image is not imported) and the canonical image it
// becomes (8-byte aligned device memory of P x {2, 3, 1, 1} bytes); P = rows x cols
struct ImageSrc { const unsigned char *data; long long row_stride; int format, form; };
struct ImageJob { ImageSrc src[4]; unsigned char *dst[4]; int P, cols; };

// nullptr: (v, rows, cols, role) describes an image; otherwise what is wrong with it
const char *image_view_fault(const tdlo_image_view *v, int rows, int cols, int role);
// [lo, hi): the bytes a checked view addresses, relative to v->data
void image_view_span(const tdlo_image_view *v, int rows, int cols, long long *lo, long long *hi);
// ImageForm, from the address, the pitch, the width and the format only
int image_import_form(const void *data, long long row_stride, int cols, int format);
// a checked HOST view -> the packed canonical image at dst (uint16 depth, 3 bytes a pixel of colour, one byte of occluder / mask), row by row
void image_pack_host(const tdlo_image_view *v, int rows, int cols, void *dst);

}  // namespace tdlo
