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
// FRONT (k_iter_fused_w0): the kernel has run the part of the E-step's front that does not depend on the new state -- zeroing the wave's accumulators -- ahead of
// the M-step half's closing barrier, and nothing is written to LDS between that barrier and the E-step's first one, which is therefore left out
template <typename T, bool FRONT = false> struct EstepHand {
    static constexpr bool kFront = FRONT;
    T x, y, z;                  // this lane's first point, requested at the top of the kernel
    const IterState *st;        // LDS: the state the M-step half has just formed (N, k2, c_norm, sh_boost, rwin32); the nodes are in the E-step's LDS copy already
    int acc_buf;                // which of the accumulator buffers this E-step adds into
    int err_w;                  // which of the loop's two error words (kFusedErrWord) a refused contribution is reported in
    int acc_rows;               // acc_rows_used(f), taken from the kernel's first batch of arguments (k_iter_fused)
};

// The LDS carve of the E-step's statements (every offset a multiple of 16 bytes) for a kernel that touches the carve ahead of the statements (k_iter_fused_w0 zeroes
// the accumulators there, EstepHand::kFront): on that route tdlo_estep_body.inc takes every pointer from HERE, so what was zeroed is what is used.  The other
// instantiations keep the expressions written out at the head of tdlo_estep_body.inc (shared, they compiled to different code); they are the same.
// rows: the tile's rows (tdlo_estep_body.inc)
template <typename T> struct EstepCarve {
    V4<T> *nodesL;      // M
    V4<T> *pts;         // NWE x kPtsStride: point i of a wave at i + (i >> 4), see the column sums
    T *lvL;             // M rounded up to 4
    T *pbase;           // the waves' membership tiles
    double *scratch;    // 16-byte aligned, stays an LDS pointer
};
template <typename T, int NWE> __device__ __forceinline__ EstepCarve<T> estep_carve(char *smem, int M, int rows) {
    EstepCarve<T> c;
    c.nodesL = (V4<T> *)smem;
    c.pts = c.nodesL + M;
    c.lvL = (T *)(c.pts + NWE * kPtsStride);
    c.pbase = c.lvL + ((M + 3) & ~3);
    c.scratch = (double *)(c.pbase + (((size_t)NWE * rows * kPStride + 7) & ~(size_t)3));
    return c;
}
// [M][4] 64-bit accumulators behind the scratch words: one set per wave up to 64 nodes (per_wave), one per workgroup beyond
__device__ __forceinline__ long long *estep_accL(double *scratch, int M, int wave, bool per_wave) {
    return (long long *)(scratch + 16) + (per_wave ? (size_t)wave * M * 4 : (size_t)0);
}
// ... of wave `wave` of the one-frame E-step on up to 64 nodes (NCH == 1, SINGLE: the whole window in the tile)
template <typename T, int EB> __device__ __forceinline__ long long *estep_single_accL(char *smem, int M, int wave) {
    return estep_accL(estep_carve<T, EB / 64>(smem, M, M < kChunk ? M : kChunk).scratch, M, wave, true);
}

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
