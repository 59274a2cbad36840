// The arena plan of a batched rig call (csrc/tdlo_rig_batch_plan.h) in a stand-alone program, built by tests/test_rig_batch_cpu.py with
// -fsanitize=address,undefined and run as a child process of its own: every table is a heap block of exactly its entries; the fixed part -- frame table,
// camera table, every distinct plane -- and then, launch by launch, the blocks of that launch's frames are WRITTEN into a heap arena of exactly `total` bytes
// with a value of their own and read back: a block outside the arena is a report, two blocks that overlap are a mismatch.  (Blocks of different launches
// share their place by design: a launch's frames are written and checked before the next launch's.)
//   arguments: Fcap, P, desc_bytes, cam_bytes, budget, then per frame "slot K" and 4 K plane keys (0: none)
//   output:    "F=<F> table=<table_off> total=<total> planes=<distinct> launches=<n>", per frame "state cams tiles pts cnt launch", then one line of plane offsets
#include "tdlo_rig_batch_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    const int Fcap = std::atoi(argv[1]), P = std::atoi(argv[2]);
    const long long desc = std::atoll(argv[3]), camb = std::atoll(argv[4]), budget = std::atoll(argv[5]);
    std::vector<int> slot, K;
    std::vector<unsigned long long> plane;
    for (int a = 6; a < argc;) {
        if (a + 2 > argc) return 2;
        slot.push_back(std::atoi(argv[a])); K.push_back(std::atoi(argv[a + 1]));
        a += 2;
        const int nk = K.back() > 0 && K.back() <= 64 ? 4 * K.back() : 0;
        if (a + nk > argc) return 2;
        for (int k = 0; k < nk; ++k) plane.push_back(std::strtoull(argv[a + k], nullptr, 10));
        a += nk;
    }
    const int F = (int)slot.size();
    // heap blocks of exactly the entries the plan may write
    long long *so = new long long[F], *co = new long long[F], *to = new long long[F], *po = new long long[F], *no = new long long[F];
    long long *plo = new long long[plane.size() + 1];
    int *lo = new int[F], npl = -1, nl = -1;
    long long table = -1, total = -1;
    unsigned long long *keys = new unsigned long long[plane.size() + 1];
    for (size_t e = 0; e < plane.size(); ++e) keys[e] = plane[e];
    auto done = [&](int rc) { delete[] so; delete[] co; delete[] to; delete[] po; delete[] no; delete[] plo; delete[] lo; delete[] keys; return rc; };
    if (tdlo::rig_batch_plan(slot.data(), K.data(), F, Fcap, P, keys, desc, camb, budget, so, co, plo, to, po, no, lo, &table, &total, &npl, &nl) != 0) {
        std::printf("refused\n");
        return done(3);
    }
    // every output is optional
    long long total2 = -1, table2 = -1;
    if (tdlo::rig_batch_plan(slot.data(), K.data(), F, Fcap, P, keys, desc, camb, budget, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &table2, &total2,
                             nullptr, nullptr) != 0 || total2 != total || table2 != table) return done(1);
    // what is refused
    if (tdlo::rig_batch_plan(nullptr, K.data(), F, Fcap, P, keys, desc, camb, budget, so, co, plo, to, po, no, lo, &table2, &total2, &npl, &nl) == 0 ||
        tdlo::rig_batch_plan(slot.data(), K.data(), 0, Fcap, P, keys, desc, camb, budget, so, co, plo, to, po, no, lo, &table2, &total2, &npl, &nl) == 0 ||
        tdlo::rig_batch_plan(slot.data(), K.data(), F, F - 1, P, keys, desc, camb, budget, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &table2, &total2, nullptr, nullptr) == 0 ||
        tdlo::rig_batch_plan(slot.data(), K.data(), F, Fcap, 0, keys, desc, camb, budget, so, co, plo, to, po, no, lo, &table2, &total2, &npl, &nl) == 0 ||
        tdlo::rig_batch_plan(slot.data(), K.data(), F, Fcap, P, keys, 0, camb, budget, so, co, plo, to, po, no, lo, &table2, &total2, &npl, &nl) == 0) return done(1);
    if (tdlo::rig_batch_plan(slot.data(), K.data(), F, Fcap, P, keys, desc, camb, budget, so, co, plo, to, po, no, lo, &table, &total, &npl, &nl) != 0) return done(1);
    unsigned char *arena = new unsigned char[total];
    std::memset(arena, 0xff, (size_t)total);
    struct Block { long long off, bytes; int tag; };
    std::vector<Block> fixed;
    fixed.push_back(Block{table, desc * F, 1});
    {
        long long cams = 0;
        for (int f = 0; f < F; ++f) { fixed.push_back(Block{co[f], camb * K[f], 2 + f % 50}); cams += K[f]; }
        std::vector<long long> seen;
        for (size_t e = 0; e < plane.size(); ++e) {
            if (plo[e] < 0) continue;
            bool had = false;
            for (long long s : seen) had = had || s == plo[e];
            if (had) continue;
            seen.push_back(plo[e]);
            const int kind = (int)(e & 3);
            fixed.push_back(Block{plo[e], (long long)(kind == 0 ? 2 : kind == 2 ? 3 : 1) * P + (kind >= 2 ? 9 : 0), 60 + (int)(seen.size() % 100)});      // (+ 9: how far a colour lane reads)
        }
        if ((int)seen.size() != npl) { std::printf("distinct planes: %d counted, %d reported\n", (int)seen.size(), npl); delete[] arena; return done(1); }
    }
    for (int f = 0; f < F; ++f) fixed.push_back(Block{so[f], tdlo::kRigBatchState, 170 + f % 50});
    int bad = 0;
    const int Tc = tdlo::rig_plan_tiles(P);
    for (int l = 0; l < nl && !bad; ++l) {
        std::vector<Block> b = fixed;
        for (int f = 0; f < F; ++f)
            if (lo[f] == l) {
                b.push_back(Block{to[f], 3ll * K[f] * Tc * tdlo::kRigBatchTile * 4, 220 + (3 * f) % 30});
                b.push_back(Block{po[f], 3ll * tdlo::kRigBatchPts * 4, 221 + (3 * f) % 30});
                b.push_back(Block{no[f], 4ll * K[f] * Tc, 222 + (3 * f) % 30});
            }
        for (const Block &k : b) std::memset(arena + k.off, k.tag, (size_t)k.bytes);
        for (size_t i = 0; i < b.size() && !bad; ++i) {
            for (long long j = 0; j < b[i].bytes; ++j) if (arena[b[i].off + j] != (unsigned char)b[i].tag) { std::printf("launch %d: block %zu overwritten\n", l, i); bad = 1; break; }
            if (b[i].off & 7) { std::printf("launch %d: block %zu not on 8 bytes\n", l, i); bad = 1; }
        }
    }
    for (int f = 0; f < F; ++f) {
        if (so[f] != tdlo::kRigBatchState * slot[f]) { std::printf("frame %d: its state block is not its slot's\n", f); bad = 1; }
        if ((to[f] | po[f] | no[f] | so[f]) & 255) { std::printf("frame %d: a block is not on 256 bytes\n", f); bad = 1; }
    }
    delete[] arena;
    if (bad) return done(1);
    std::printf("F=%d table=%lld total=%lld planes=%d launches=%d\n", F, table, total, npl, nl);
    for (int f = 0; f < F; ++f) std::printf("%lld %lld %lld %lld %lld %d\n", so[f], co[f], to[f], po[f], no[f], lo[f]);
    for (size_t e = 0; e < plane.size(); ++e) std::printf("%lld ", plo[e]);
    std::printf("\n");
    return done(0);
}
