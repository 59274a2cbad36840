// tdlo_estep_body.h -- what the kernels that carry the E-step (trackdlo.cpp:278-389) share: k_estep (tdlo_device.hip) and the kernel that runs an M-step and
// the E-step behind it in one launch (tdlo_iter_fused.hip, k_iter_fused).  The E-step's statements themselves are tdlo_estep_body.inc, included INTO the
// kernel's body: as a device function the same statements came out of the compiler as different code for every k_estep instantiation (a few instructions
// more or fewer each), and k_estep is to stay the kernel it was.
#pragma once
#include "tdlo_devcommon.h"
#include "tdlo_estep_wide.h"
#include "tdlo_mstep_generic.h"
#include <type_traits>

namespace tdlo {

// FUSED: what the M-step half of the same launch hands over instead of memory
template <typename T> struct EstepHand {
    T x, y, z;                  // this lane's first point, requested at the top of the kernel
    const IterState *st;        // LDS: the state the M-step half has just formed (N, k2, c_norm, sh_boost, rwin32); the nodes are in the E-step's LDS copy already
    int acc_buf;                // which of the accumulator buffers this E-step adds into
    int err_w;                  // which of the loop's two error words (kFusedErrWord) a refused contribution is reported in
    int acc_rows;               // acc_rows_used(f), taken from the kernel's first batch of arguments (k_iter_fused)
};

// dynamic LDS of the E-step's statements (the carve at their head)
template <typename T, int EB> static size_t estep_lds_bytes(int M, bool single) {
    const int rt = (M <= kChunk && single) ? kChunk : tile_rows<T>(M <= kChunk ? 1 : 2);
    const int rows = M < rt ? M : rt;
    constexpr int NWE = EB / 64;
    const size_t tile = sizeof(T) * (((size_t)NWE * rows * kPStride + 7) & ~(size_t)3);
    const size_t red = (size_t)NWE * 64 * 4 * sizeof(double);
    size_t b = sizeof(V4<T>) * (size_t)M + sizeof(V4<T>) * NWE * kPtsStride + sizeof(T) * (size_t)((M + 3) & ~3);
    b += (tile > red ? tile : red) + 16 * sizeof(double) + 64;
    b += sizeof(double) * (size_t)(M <= kChunk ? NWE : 1) * M * 4;     // [M][4] 64-bit accumulators: per wave up to 64 nodes, per workgroup beyond
    return b;
}

}  // namespace tdlo
