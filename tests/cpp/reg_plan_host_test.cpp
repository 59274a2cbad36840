// The per-frame plan of a batched start (csrc/tdlo_reg_plan.h) in a stand-alone program, built by tests/test_init_batch_cpu.py with
// -fsanitize=address,undefined and run as a child process of its own: every table is a heap block of exactly F entries, and every frame's blocks are
// then WRITTEN into a heap workspace of exactly `total` doubles with a value of their own and read back -- a block outside the workspace is a report,
// two blocks that overlap are a mismatch.
//   arguments: M, then the F cloud sizes
//   output:    "F=<F> M=<M> total=<total>" and per frame "nblk state_off part_off out_off"
#include "tdlo_reg_plan.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const int M = std::atoi(argv[1]), F = argc - 2;
    int *N = new int[F], *nblk = new int[F];
    long long *so = new long long[F], *po = new long long[F], *oo = new long long[F], total = -1;
    for (int f = 0; f < F; ++f) N[f] = std::atoi(argv[2 + f]);
    if (tdlo::reg_batch_plan(N, F, M, nblk, so, po, oo, &total) != 0) {
        std::printf("refused\n");
        delete[] N; delete[] nblk; delete[] so; delete[] po; delete[] oo;
        return 3;
    }
    // every output is optional
    long long total2 = -1;
    if (tdlo::reg_batch_plan(N, F, M, nullptr, nullptr, nullptr, nullptr, &total2) != 0 || total2 != total) return 1;
    if (tdlo::reg_batch_plan(N, F, M, nblk, so, po, oo, nullptr) != 0) return 1;
    // what is refused
    if (tdlo::reg_batch_plan(nullptr, F, M, nblk, so, po, oo, &total2) == 0 || tdlo::reg_batch_plan(N, 0, M, nblk, so, po, oo, &total2) == 0 ||
        tdlo::reg_batch_plan(N, F, 0, nblk, so, po, oo, &total2) == 0) return 1;
    double *ws = new double[total];
    for (long long i = 0; i < total; ++i) ws[i] = -1.0;
    const long long ns = 8 + 3LL * M, no = tdlo::reg_plan_out_doubles(M);
    for (int f = 0; f < F; ++f) {
        const long long np = tdlo::reg_plan_part_doubles(M, nblk[f]);
        for (long long i = 0; i < ns; ++i) ws[so[f] + i] = 3.0 * f;
        for (long long i = 0; i < np; ++i) ws[po[f] + i] = 3.0 * f + 1;
        for (long long i = 0; i < no; ++i) ws[oo[f] + i] = 3.0 * f + 2;
    }
    for (int f = 0; f < F; ++f) {
        const long long np = tdlo::reg_plan_part_doubles(M, nblk[f]);
        for (long long i = 0; i < ns; ++i) if (ws[so[f] + i] != 3.0 * f) { std::printf("frame %d: state overwritten\n", f); return 1; }
        for (long long i = 0; i < np; ++i) if (ws[po[f] + i] != 3.0 * f + 1) { std::printf("frame %d: partials overwritten\n", f); return 1; }
        for (long long i = 0; i < no; ++i) if (ws[oo[f] + i] != 3.0 * f + 2) { std::printf("frame %d: output overwritten\n", f); return 1; }
        if ((oo[f] & 1) || (so[f] & 1)) { std::printf("frame %d: not on 16 bytes\n", f); return 1; }
    }
    std::printf("F=%d M=%d total=%lld\n", F, M, total);
    for (int f = 0; f < F; ++f) std::printf("%d %lld %lld %lld\n", nblk[f], so[f], po[f], oo[f]);
    delete[] N; delete[] nblk; delete[] so; delete[] po; delete[] oo; delete[] ws;
    return 0;
}
