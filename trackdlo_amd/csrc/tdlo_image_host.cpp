// tdlo_image_host.cpp -- the host pieces of image views (tdlo_image_view): check, extent, the import kernel's form chooser, and the pack-and-convert
// of a host view into the packed canonical image.  Pure C++: no HIP, no device, so that a stand-alone program can exercise every line of it (built
// with -ffp-contract=off like tdlo_host.cpp, although the float rule below does not depend on it).
//
// THE RULE (as in tdlo_image.hip): no load touches a byte outside the view's extent (tdlo_image_view_extent) -- every row is read from its first
// pixel's first byte to its last pixel's last byte, element by element or with memcpy of exactly that range.
#include "tdlo_image.h"

#include <cstdint>
#include <cstring>

namespace tdlo {

static bool role_takes(int role, int format) {
    switch (role) {
    case kRoleDepth: return format == TDLO_IMG_U16C1 || format == TDLO_IMG_F32C1;
    case kRoleColour: return format == TDLO_IMG_U8C3 || format == TDLO_IMG_U8C4;
    case kRoleOccluder: case kRoleMask: return format == TDLO_IMG_U8C1;
    }
    return false;
}

const char *image_view_fault(const tdlo_image_view *v, int rows, int cols, int role) {
    if (!v) return "image view: null view";
    if (!v->data) return "image view: null data";
    if (role < kRoleDepth || role > kRoleMask) return "image view: unknown role";
    if (!image_bpp(v->format)) return "image view: unknown format";
    if (v->location != TDLO_MEM_AUTO && v->location != TDLO_MEM_HOST && v->location != TDLO_MEM_DEVICE) return "image view: unknown location";
    if (!role_takes(role, v->format)) return "image view: a format this image does not take (depth U16C1 / F32C1, colour U8C3 / U8C4, occluder and mask U8C1)";
    if (rows <= 0 || cols <= 0 || (long long)rows * cols > (1ll << 26)) return "image view: bad shape (rows x cols must be 1 .. 2^26)";
    const int es = image_elem(v->format);
    if ((uintptr_t)v->data % (uintptr_t)es) return "image view: data is not aligned to its element size";
    if (v->row_stride % es) return "image view: row_stride is no multiple of the element size";
    const long long row_bytes = (long long)cols * image_bpp(v->format);
    if (rows > 1 && v->row_stride < row_bytes && v->row_stride > -row_bytes) return "image view: rows overlap (|row_stride| < cols x bytes per pixel)";
    const __int128 a = (__int128)(rows - 1) * v->row_stride, lim = (__int128)1 << 62;
    if (a <= -lim || a + row_bytes >= lim) return "image view: the extent does not fit 64-bit byte offsets";
    return nullptr;
}

void image_view_span(const tdlo_image_view *v, int rows, int cols, long long *lo, long long *hi) {
    const long long a = (long long)(rows - 1) * v->row_stride;
    *lo = a < 0 ? a : 0;
    *hi = (a > 0 ? a : 0) + (long long)cols * image_bpp(v->format);
}

// A vector load is legal only at a naturally aligned address that lies wholly inside one row of the view.  A lane's four pixels lie in one row when
// cols % 4 == 0; they start at data + row * row_stride + (4 k) * bpp, so the alignment of data and of row_stride decides (4 k bpp is a multiple of 4,
// 8 or 16 for bpp 1 and 3, 2, 4).
int image_import_form(const void *data, long long row_stride, int cols, int format) {
    if (cols % 4) return kImgElem;
    const uintptr_t a = (uintptr_t)data;
    const unsigned long long s = (unsigned long long)row_stride;           // (two's complement: the low bits of a negative pitch are its alignment)
    if (a % 4 || s % 4) return kImgElem;
    const unsigned wide = format == TDLO_IMG_U16C1 ? 8 : (format == TDLO_IMG_U8C4 || format == TDLO_IMG_F32C1) ? 16 : 0;
    return wide && a % wide == 0 && s % wide == 0 ? kImgWide : kImgDwords;
}

void image_pack_host(const tdlo_image_view *v, int rows, int cols, void *dst) {
    const unsigned char *src = (const unsigned char *)v->data;
    const size_t n = (size_t)cols;
    for (int i = 0; i < rows; ++i) {
        const unsigned char *row = src + (long long)i * v->row_stride;
        switch (v->format) {
        case TDLO_IMG_U8C1: std::memcpy((unsigned char *)dst + i * n, row, n); break;
        case TDLO_IMG_U8C3: std::memcpy((unsigned char *)dst + 3 * i * n, row, 3 * n); break;
        case TDLO_IMG_U16C1: std::memcpy((unsigned char *)dst + 2 * i * n, row, 2 * n); break;
        case TDLO_IMG_U8C4: {
            unsigned char *o = (unsigned char *)dst + 3 * i * n;
            for (size_t j = 0; j < n; ++j) { o[3 * j] = row[4 * j]; o[3 * j + 1] = row[4 * j + 1]; o[3 * j + 2] = row[4 * j + 2]; }
            break;
        }
        case TDLO_IMG_F32C1: {
            unsigned short *o = (unsigned short *)dst + i * n;
            for (size_t j = 0; j < n; ++j) { float d; std::memcpy(&d, row + 4 * j, 4); o[j] = image_f32_to_mm(d); }
            break;
        }
        }
    }
}

}  // namespace tdlo

extern "C" {

int tdlo_image_view_check(const tdlo_image_view *v, int rows, int cols, int role) { return tdlo::image_view_fault(v, rows, cols, role) ? TDLO_E_INVALID : TDLO_OK; }

int tdlo_image_view_extent(const tdlo_image_view *v, int rows, int cols, long long *lo_bytes, long long *hi_bytes) {
    if (!v || !lo_bytes || !hi_bytes || !tdlo::image_bpp(v->format)) return TDLO_E_INVALID;
    const int role = v->format == TDLO_IMG_U8C1 ? tdlo::kRoleMask : (v->format == TDLO_IMG_U8C3 || v->format == TDLO_IMG_U8C4) ? tdlo::kRoleColour : tdlo::kRoleDepth;
    if (tdlo::image_view_fault(v, rows, cols, role)) return TDLO_E_INVALID;
    tdlo::image_view_span(v, rows, cols, lo_bytes, hi_bytes);
    return TDLO_OK;
}

int tdlo_image_view_form(const tdlo_image_view *v, int cols) {
    if (!v || !v->data || !tdlo::image_bpp(v->format) || cols <= 0) return TDLO_E_INVALID;
    return tdlo::image_import_form(v->data, v->row_stride, cols, v->format);
}

int tdlo_image_view_pack(const tdlo_image_view *v, int rows, int cols, int role, void *canonical_out) {
    if (!canonical_out || tdlo::image_view_fault(v, rows, cols, role)) return TDLO_E_INVALID;
    tdlo::image_pack_host(v, rows, cols, canonical_out);
    return TDLO_OK;
}

}  // extern "C"
