// align_batch_host_test.cpp -- the grids of k_align_splat_batch and k_align_pack_batch (csrc/tdlo_align_batch.hip) walked on the host under AddressSanitizer and
// UBSan: for every (workgroup, job) of every job list the lanes of csrc/tdlo_align_lane.h run through the offsets of csrc/tdlo_align_batch_plan.h and a host
// copy of the job table, exactly as the kernels index them -- a workgroup beyond its job's pixels leaves, the pack's first four lanes of a job hand its counts
// over and zero them.  ONE arena serves all calls, under the library's rule: its scratch region is filled only where it was not yet ([armed, scratch_bytes)
// when a layout's region is longer than what is armed; a shorter layout leaves only its own region counted as armed).  Every list is called TWICE in a row, in
// the given and in the reversed order of its jobs -- two different layouts with the same scratch region -- WITHOUT a fill in between, and after every call every
// word of the scratch region must be armed.  The depth views are allocated at exactly their extents.
// Built from this file, tdlo_align_host.cpp and tdlo_image_host.cpp (no HIP) by tests/test_align_batch_cpu.py.  Input:  int32 lists, then per list int32 J and
// per job   int32 rows_d, cols_d, rows_c, cols_c, format, has_T, max_footprint, layout (0 packed, 1 pitched, 2 bottom-up)
//           double fx_d, fy_d, cx_d, cy_d, fx_c, fy_c, cx_c, cy_c, T[12];  the depth image packed (2 or 4 bytes an element)
// Output: per call (list 0 forward, list 0 reversed, list 1 forward, ...) and per job IN THE CALL'S ORDER: the plane (uint16), int64 counts[4].
#include "tdlo_align_batch_plan.h"
#include "tdlo_align_host.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

using namespace tdlo;

struct HostJob {
    int32_t h[8];
    double g[20];
    unsigned char *buf = nullptr;      // the view at exactly its extent
    tdlo_image_view view{};
    tdlo_align_params p{};
};

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
static bool wr(FILE *f, const void *p, size_t n) { return n == 0 || std::fwrite(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: align_batch_host_test <lists> <out>\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb"), *o = std::fopen(argv[2], "wb");
    if (!f || !o) { std::perror("open"); return 2; }
    int32_t L = 0;
    if (!rd(f, &L, 4)) return 2;
    std::vector<std::vector<HostJob>> lists(L);
    long long most = 0;
    for (auto &jobs : lists) {
        int32_t J = 0;
        if (!rd(f, &J, 4)) return 2;
        jobs.resize(J);
        std::vector<int> rows(J), cols(J);
        for (int j = 0; j < J; ++j) {
            HostJob &q = jobs[j];
            if (!rd(f, q.h, sizeof q.h) || !rd(f, q.g, sizeof q.g)) return 2;
            const int rows_d = q.h[0], cols_d = q.h[1], format = q.h[4], layout = q.h[7];
            const size_t es = format == TDLO_IMG_F32C1 ? 4 : 2, Pd = (size_t)rows_d * cols_d;
            std::vector<unsigned char> packed(Pd * es);
            if (!rd(f, packed.data(), Pd * es)) return 2;
            const size_t pitch = (layout ? (size_t)cols_d + 3 : (size_t)cols_d) * es, extent = (size_t)(rows_d - 1) * pitch + (size_t)cols_d * es;
            q.buf = static_cast<unsigned char *>(std::malloc(extent));
            std::memset(q.buf, 0x11, extent);
            for (int r = 0; r < rows_d; ++r) std::memcpy(q.buf + (size_t)(layout == 2 ? rows_d - 1 - r : r) * pitch, packed.data() + (size_t)r * cols_d * es, (size_t)cols_d * es);
            q.view = tdlo_image_view{layout == 2 ? q.buf + (size_t)(rows_d - 1) * pitch : q.buf, format, TDLO_MEM_HOST, layout == 2 ? -(long long)pitch : (long long)pitch, nullptr};
            q.p = tdlo_align_params{rows_d, cols_d, q.g[0], q.g[1], q.g[2], q.g[3], q.h[2], q.h[3], q.g[4], q.g[5], q.g[6], q.g[7], q.h[5] ? q.g + 8 : nullptr, q.h[6]};
            if (tdlo_align_check(&q.p) || tdlo_image_view_check(&q.view, rows_d, cols_d, TDLO_ROLE_DEPTH)) { std::fprintf(stderr, "a job is refused\n"); return 1; }
            rows[j] = q.h[2]; cols[j] = q.h[3];
        }
        long long total = 0;
        if (align_batch_plan(rows.data(), cols.data(), J, kAlignBatchBudget, nullptr, nullptr, nullptr, nullptr, nullptr, &total)) { std::fprintf(stderr, "no plan\n"); return 1; }
        most = std::max(most, total);
    }
    std::fclose(f);
    unsigned char *arena = static_cast<unsigned char *>(::operator new((size_t)most, std::align_val_t(256)));
    std::memset(arena, 0x5a, (size_t)most);                      // (nothing is armed yet: whatever a call relies on it must have filled by the rule)
    long long armed = 0, calls = 0, lanes = 0, fills = 0, bad = 0;
    for (auto &fwd : lists) {
        for (int pass = 0; pass < 2; ++pass) {
            std::vector<const HostJob *> jobs;
            for (const HostJob &q : fwd) jobs.push_back(&q);
            if (pass) std::reverse(jobs.begin(), jobs.end());
            const int J = (int)jobs.size();
            std::vector<int> rows(J), cols(J);
            for (int j = 0; j < J; ++j) { rows[j] = jobs[j]->h[2]; cols[j] = jobs[j]->h[3]; }
            std::vector<long long> so(J), po(J), co(J);
            long long tab = 0, sb = 0, total = 0;
            if (align_batch_plan(rows.data(), cols.data(), J, kAlignBatchBudget, so.data(), po.data(), co.data(), &tab, &sb, &total)) return 1;
            // ---- the library's rule for the scratch region
            armed = std::min(armed, sb);
            if (armed < sb) {
                if (pass) { std::fprintf(stderr, "the reversed list needs a fill: the two layouts do not share their scratch region\n"); return 1; }
                std::memset(arena + armed, 0xff, (size_t)(sb - armed));
                ++fills;
            }
            // ---- the count words zeroed and the table written, as the one copy of the call does
            std::memset(arena + co[0], 0, (size_t)(tab - co[0]));
            AlignBatchRec *table = reinterpret_cast<AlignBatchRec *>(arena + tab);
            int most_Pd = 0, most_Pc = 0;
            for (int j = 0; j < J; ++j) {
                AlignBatchRec r{};
                align_job(&jobs[j]->view, &jobs[j]->p, r.job);
                r.scratch = reinterpret_cast<unsigned *>(arena + so[j]);
                r.plane = reinterpret_cast<unsigned short *>(arena + po[j]);
                r.counts = reinterpret_cast<unsigned long long *>(arena + co[j]);
                std::memcpy(&table[j], &r, sizeof r);
                most_Pd = std::max(most_Pd, jobs[j]->h[0] * jobs[j]->h[1]);
                most_Pc = std::max(most_Pc, rows[j] * cols[j]);
            }
            std::vector<unsigned long long> counts_out(4 * (size_t)J, ~0ull);
            // ---- k_align_splat_batch: grid (blocks of the job with the most depth pixels, J)
            const int gx = (most_Pd + 255) / 256;
            for (int y = 0; y < J; ++y)
                for (int bx = 0; bx < gx; ++bx) {
                    const AlignBatchRec &rec = table[y];
                    if (bx * 256 >= rec.job.rows_d * rec.job.cols_d) continue;
                    unsigned *scratch = rec.scratch;
                    for (int t = 0; t < 256; ++t) {
                        const int verdict = align_splat_lane(rec.job, bx * 256 + t, [scratch](int i, unsigned k) { scratch[i] = std::min(scratch[i], k); });
                        if (verdict != kAlignZero) { ++rec.counts[0]; ++rec.counts[verdict]; }
                        ++lanes;
                    }
                }
            // ---- k_align_pack_batch: grid (blocks of the job with the most colour pixels / 4, J)
            const int gp = ((most_Pc + 3) / 4 + 255) / 256;
            for (int y = 0; y < J; ++y)
                for (int bx = 0; bx < gp; ++bx) {
                    const AlignBatchRec &rec = table[y];
                    const int P = rec.job.rows_c * rec.job.cols_c;
                    if (bx * 256 >= (P + 3) / 4) continue;
                    for (int t = bx * 256; t < bx * 256 + 256; ++t) {
                        align_pack_lane(rec.scratch, rec.plane, P, t);
                        if (t < 4) { counts_out[4 * (size_t)y + t] = rec.counts[t]; rec.counts[t] = 0; }
                        ++lanes;
                    }
                }
            armed = sb;
            // ---- every word of the scratch region is armed, the count words are zero
            for (long long w = 0; w < sb / 4; ++w) bad += reinterpret_cast<const unsigned *>(arena)[w] != kAlignEmpty;
            for (long long w = 0; w < 4ll * J; ++w) bad += reinterpret_cast<const unsigned long long *>(arena + co[0])[w] != 0ull;
            for (int j = 0; j < J; ++j) {
                const long long n[4] = {(long long)counts_out[4 * j], (long long)counts_out[4 * j + 1], (long long)counts_out[4 * j + 2], (long long)counts_out[4 * j + 3]};
                if (!wr(o, arena + po[j], 2 * (size_t)rows[j] * cols[j]) || !wr(o, n, sizeof n)) return 2;
            }
            ++calls;
        }
    }
    std::fclose(o);
    ::operator delete(arena, std::align_val_t(256));
    for (auto &jobs : lists) for (HostJob &q : jobs) std::free(q.buf);
    std::printf("%lld calls, %lld lanes, %lld fills, %lld words not armed\n", calls, lanes, fills, bad);
    return bad ? 1 : 0;
}
