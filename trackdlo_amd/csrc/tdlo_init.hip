// tdlo_init.hip -- `sort_pts` on the device: the chain order of `reg`'s centroids, and the chain coordinate.
//
// trackdlo/src/utils.cpp:95-170 puts M unordered nodes into chain order: node 0 first, then a minimum spanning tree grown from it -- each of
// the M - 1 rounds takes the pair (a selected, b unselected) of smallest non-zero squared distance G(a, b), the first such pair in a ascending,
// then b ascending order (:120-132, `minimum > G` is strict) -- and b enters the output list where the reverse / reverse_on /
// insertion_counter / last_visited_b bookkeeping of :134-157 says.  The reference's first-frame initialiser is reg + sort_pts + the cumulative
// segment lengths (utils/tracking_test.py:523-541; the lengths as trackdlo_node.cpp:135-141): k_sort_pts runs behind tdlo_reg.hip's loop on the
// centroids where they lie, so a cloud born on the device becomes a tracker's nodes and coordinates without visiting the host.
//
// One workgroup, thread = node, 2 <= M <= 1024; one wave for M <= 64.  Not a hot loop (once per tracker): the plain form throughout.
//   state   a node's smallest distance to the selected set and the smallest selected index attaining it, in registers (no M x M matrix: distances
//           are formed on the fly from the coordinates in LDS); the round's pair is the minimum by (distance, parent, node): shuffles within
//           the wave, one LDS step across the waves.  An infinite distance is no edge either (`INFINITY > G` is false, :116 / :124).
//   list    a place per selected node; an insertion at place p moves every node at a place >= p up by one, all threads at once.
//   output  [sigma2 (copied from reg's state, or 0) | status | Y sorted (3 M, column-major) | coord (M)] doubles, then perm (M ints).
//   status  0; 1 a non-finite coordinate; 2 two nodes with equal coordinates (compared as values: -0.0 equals 0.0, as the reference's
//           G != 0); 3 a round that finds no edge (distances that underflow to 0 or overflow).  Non-zero: only the two header words are written.
// The decisions compare fp64 values that the host twin (tdlo_host.cpp, sort_pts_host) forms with the same roundings -- (dx dx + dy dy) + dz dz,
// each product and sum rounded, no contraction (the pragma below; the Makefile passes -ffp-contract=off as well) -- so the permutation and the
// coordinate's bits are the twin's exactly.
#include "tdlo_internal.h"

#include <climits>

namespace tdlo {
namespace {

__device__ __forceinline__ double dist2(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const double s = xx + yy;
    return s + zz;
}

// (g, a, b) orders before (h, c, d): the pair the reference's scan meets first among equal distances has the smaller a, then the smaller b
__device__ __forceinline__ bool pair_before(double g, int a, int b, double h, int c, int d) {
    return g < h || (g == h && (a < c || (a == c && b < d)));
}

// one workgroup's whole job on one node set; k_sort_pts and k_sort_pts_batch below are this text
template <bool kOneWave>
__device__ __forceinline__ void sort_pts_body(const double *__restrict__ Yin, const double *__restrict__ state, int M, double *__restrict__ out) {
    constexpr int kCap = kOneWave ? kWave : kMaxNodes;
    __shared__ double xs[kCap], ys[kCap], zs[kCap], seg[kCap];
    __shared__ int place[kCap], order[kCap];      // place[node] (selected nodes), order[place] = node
    __shared__ double red_g[16];
    __shared__ int red_a[16], red_b[16], flag[2];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, nw = blockDim.x >> 6;
    const bool live = t < M;
    const double inf = __builtin_huge_val();
    double x = 0.0, y = 0.0, z = 0.0;
    if (live) {
        x = Yin[t]; y = Yin[M + t]; z = Yin[2 * M + t];
        xs[t] = x; ys[t] = y; zs[t] = z;
        place[t] = t == 0 ? 0 : -1;
    }
    if (t < 2) flag[t] = 0;
    __syncthreads();
    if (live) {
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) flag[0] = 1;
        bool twin = false;
        for (int j = 0; j < M; ++j) twin = twin || (j != t && xs[j] == x && ys[j] == y && zs[j] == z);
        if (twin) flag[1] = 1;
    }
    __syncthreads();
    int status = flag[0] ? 1 : (flag[1] ? 2 : 0);

    bool sel = !live || t == 0;                   // (threads beyond M never stand for a node)
    int pos = t == 0 ? 0 : -1;
    double best = inf;
    int parent = INT_MAX;
    if (!sel) {
        const double g = dist2(xs[0], ys[0], zs[0], x, y, z);
        if (g != 0.0 && g < inf) { best = g; parent = 0; }
    }
    int reverse = 0, reverse_on = 0, insertion_counter = 0, last_visited_b = 0;
    for (int counter = 0; status == 0 && counter < M - 1; ++counter) {      // (status is the same in every thread: the barriers inside are met by all)
        // the round's pair: minimum over the unselected nodes by (distance, parent, node)
        double cg = sel ? inf : best;
        int ca = sel ? INT_MAX : parent, cb = sel ? INT_MAX : t;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double og = __shfl_xor(cg, o);
            const int oa = __shfl_xor(ca, o), ob = __shfl_xor(cb, o);
            if (pair_before(og, oa, ob, cg, ca, cb)) { cg = og; ca = oa; cb = ob; }
        }
        if (!kOneWave) {
            // across the waves: every thread walks the (at most 16) waves' records.  (One LDS read per lane and four more shuffle steps instead were
            // measured: 2.96 against 3.52 ms at 1024 nodes, but 538 against 465 us at 300 -- five records are walked sooner than four steps are taken)
            if (lane == 0) { red_g[w] = cg; red_a[w] = ca; red_b[w] = cb; }
            __syncthreads();
            cg = red_g[0]; ca = red_a[0]; cb = red_b[0];
            for (int i = 1; i < nw; ++i)
                if (pair_before(red_g[i], red_a[i], red_b[i], cg, ca, cb)) { cg = red_g[i]; ca = red_a[i]; cb = red_b[i]; }
        }
        if (!(cg < inf)) { status = 3; break; }
        const int a = ca, b = cb;
        // where b enters the list (:134-157; the reference finds a and reverse_on in the list by value, which for distinct nodes is by index)
        int p;
        if (counter == 0) p = 1;
        else {
            if (last_visited_b != a) { reverse += 1; reverse_on = a; insertion_counter = 1; }
            if (reverse % 2 == 1) p = place[a];
            else if (reverse != 0) { p = place[reverse_on] + insertion_counter; insertion_counter += 1; }
            else p = counter + 1;
        }
        __syncthreads();                          // every thread has read place[] and red_*[] of this round
        if (t == b) { sel = true; pos = p; place[t] = p; }
        else if (sel && pos >= p) { pos += 1; place[t] = pos; }
        last_visited_b = b;
        if (!sel) {
            const double g = dist2(xs[b], ys[b], zs[b], x, y, z);
            if (g != 0.0 && (g < best || (g == best && b < parent))) { best = g; parent = b; }
        }
        __syncthreads();                          // place[] is this round's before the next one reads it
    }

    if (status != 0) {
        if (t == 0) { out[0] = state ? state[0] : 0.0; out[1] = (double)status; }
        return;
    }
    if (live && (unsigned)pos < (unsigned)M) order[pos] = t;
    __syncthreads();
    double *Ys = out + 2, *coord = Ys + 3 * (size_t)M;
    int *perm = reinterpret_cast<int *>(coord + M);
    if (live) {
        const int n = order[t];
        Ys[t] = xs[n]; Ys[M + t] = ys[n]; Ys[2 * M + t] = zs[n];
        perm[t] = n;
        if (t > 0) { const int q = order[t - 1]; seg[t] = __dsqrt_rn(dist2(xs[n], ys[n], zs[n], xs[q], ys[q], zs[q])); }
    }
    __syncthreads();
    if (t == 0) {
        // added up serially in chain order, as trackdlo_node.cpp:135-141 does: the sum's bits are part of the contract
        double cur = 0.0;
        coord[0] = 0.0;
        for (int i = 1; i < M; ++i) { cur = __dadd_rn(cur, seg[i]); coord[i] = cur; }
        out[0] = state ? state[0] : 0.0;
        out[1] = 0.0;
    }
}

template <bool kOneWave>
__global__ __launch_bounds__(kOneWave ? 64 : 1024) void k_sort_pts(const double *__restrict__ Yin, const double *__restrict__ state, int M,
                                                                  double *__restrict__ out) {
    sort_pts_body<kOneWave>(Yin, state, M, out);
}

// F node sets in one launch, blockIdx.x = frame: frame f's nodes at Yin + f in_stride and its output block at out + f out_stride; with_state: the nodes
// are those of a reg state block, where reg left them, and the block begins 8 doubles before them.  A kernel of its own beside k_sort_pts, whose
// arguments, registers and LDS stay as they were.
template <bool kOneWave>
__global__ __launch_bounds__(kOneWave ? 64 : 1024) void k_sort_pts_batch(const double *__restrict__ Yin, long long in_stride, int with_state, int M,
                                                                        double *__restrict__ out, long long out_stride) {
    const double *Y = Yin + (size_t)blockIdx.x * in_stride;
    sort_pts_body<kOneWave>(Y, with_state ? Y - 8 : nullptr, M, out + (size_t)blockIdx.x * out_stride);
}

}  // namespace

size_t sort_pts_out_doubles(int M) { return 2 + 4 * (size_t)M + ((size_t)M + 1) / 2; }

hipError_t launch_sort_pts(const double *Y, const double *state, int M, double *out, hipStream_t s) {
    if (M <= kWave) hipLaunchKernelGGL(k_sort_pts<true>, dim3(1), dim3(kWave), 0, s, Y, state, M, out);
    else hipLaunchKernelGGL(k_sort_pts<false>, dim3(1), dim3((M + kWave - 1) / kWave * kWave), 0, s, Y, state, M, out);
    return hipGetLastError();
}

hipError_t launch_sort_pts_batch(const double *Y, long long in_stride, bool with_state, int F, int M, double *out, long long out_stride, hipStream_t s) {
    if (M <= kWave) hipLaunchKernelGGL(k_sort_pts_batch<true>, dim3(F), dim3(kWave), 0, s, Y, in_stride, with_state ? 1 : 0, M, out, out_stride);
    else hipLaunchKernelGGL(k_sort_pts_batch<false>, dim3(F), dim3((M + kWave - 1) / kWave * kWave), 0, s, Y, in_stride, with_state ? 1 : 0, M, out, out_stride);
    return hipGetLastError();
}

}  // namespace tdlo
