// The arena plan of a batched voxel grid on cloud views (csrc/tdlo_view_batch_plan.h) in a stand-alone program, built by tests/test_view_batch_cpu.py with
// -fsanitize=address,undefined and run as a child process of its own: every table is a heap block of exactly F entries, and every frame's blocks -- and
// the descriptor table -- are then WRITTEN into a heap arena of exactly `total` bytes with a value of their own and read back: a block outside the arena
// is a report, two blocks that overlap are a mismatch.
//   arguments: Fcap, desc_bytes, then the F element counts
//   output:    "F=<F> Fcap=<Fcap> table=<table_off> total=<total>" and per frame "state_off tiles_off pts_off cnt_off"
#include "tdlo_view_batch_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    const int Fcap = std::atoi(argv[1]), F = argc - 3;
    const long long desc = std::atoll(argv[2]);
    int *N = new int[F];
    long long *so = new long long[F], *to = new long long[F], *po = new long long[F], *co = new long long[F], table = -1, total = -1;
    for (int f = 0; f < F; ++f) N[f] = std::atoi(argv[3 + f]);
    auto done = [&](int rc) { delete[] N; delete[] so; delete[] to; delete[] po; delete[] co; return rc; };
    if (tdlo::view_batch_plan(N, F, Fcap, desc, so, to, po, co, &table, &total) != 0) {
        std::printf("refused\n");
        return done(3);
    }
    // every output is optional
    long long total2 = -1, table2 = -1;
    if (tdlo::view_batch_plan(N, F, Fcap, desc, nullptr, nullptr, nullptr, nullptr, &table2, &total2) != 0 || total2 != total || table2 != table) return done(1);
    if (tdlo::view_batch_plan(N, F, Fcap, desc, so, to, po, co, nullptr, nullptr) != 0) return done(1);
    // what is refused
    if (tdlo::view_batch_plan(nullptr, F, Fcap, desc, so, to, po, co, &table2, &total2) == 0 || tdlo::view_batch_plan(N, 0, Fcap, desc, so, to, po, co, &table2, &total2) == 0 ||
        tdlo::view_batch_plan(N, Fcap + 1, Fcap, desc, nullptr, nullptr, nullptr, nullptr, &table2, &total2) == 0 ||
        tdlo::view_batch_plan(N, F, Fcap, 0, so, to, po, co, &table2, &total2) == 0) return done(1);
    unsigned char *arena = new unsigned char[total];
    std::memset(arena, 0xff, (size_t)total);
    struct Block { long long off, bytes; };
    auto blocks = [&](int f, Block b[4]) {
        b[0] = Block{so[f], tdlo::kViewBatchState};
        b[1] = Block{to[f], 3ll * N[f] * 4};
        b[2] = Block{po[f], 3ll * tdlo::kViewBatchPts * 4};
        b[3] = Block{co[f], 4ll * tdlo::view_plan_tiles(N[f])};
    };
    std::memset(arena + table, 0xfe, (size_t)(desc * F));
    for (int f = 0; f < F; ++f) {
        Block b[4];
        blocks(f, b);
        for (int k = 0; k < 4; ++k) std::memset(arena + b[k].off, (4 * f + k) % 250, (size_t)b[k].bytes);
    }
    int bad = 0;
    for (long long i = 0; i < desc * F; ++i) if (arena[table + i] != 0xfe) bad = 1;
    if (bad) std::printf("the table was overwritten\n");
    if (table & 255) { std::printf("the table is not on 256 bytes\n"); bad = 1; }
    for (int f = 0; f < F && !bad; ++f) {
        Block b[4];
        blocks(f, b);
        for (int k = 0; k < 4; ++k) {
            for (long long i = 0; i < b[k].bytes; ++i) if (arena[b[k].off + i] != (4 * f + k) % 250) { std::printf("frame %d: block %d overwritten\n", f, k); bad = 1; break; }
            if (b[k].off & 255) { std::printf("frame %d: block %d not on 256 bytes\n", f, k); bad = 1; }
        }
        if (so[f] != tdlo::kViewBatchState * f) { std::printf("frame %d: its state block moved\n", f); bad = 1; }
    }
    delete[] arena;
    if (bad) return done(1);
    std::printf("F=%d Fcap=%d table=%lld total=%lld\n", F, Fcap, table, total);
    for (int f = 0; f < F; ++f) std::printf("%lld %lld %lld %lld\n", so[f], to[f], po[f], co[f]);
    return done(0);
}
