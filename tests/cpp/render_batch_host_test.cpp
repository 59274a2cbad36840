// The per-lane code of k_render_batch (csrc/tdlo_render_search.h: loads, the two-level search, blend, stores) compiled for the host and run one "lane" at a
// time in a stand-alone program, built by tests/test_render_batch_ref.py with -fsanitize=address,undefined and run as a child process of its own (nothing
// preloaded).  Images and tables are allocated at exactly their sizes, so a load or store beyond an image, a head or a primitive record is reported.
// Every image is compared with a literal blend-then-paint loop of this program: blend every byte, then rope after rope, primitive after primitive, every
// pixel of the image tested and overwritten.  Prints "<n> pictures, 0 differing bytes".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../trackdlo_amd/csrc/tdlo_render_search.h"

using namespace tdlo;

static unsigned long long g_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(g_state >> 33); }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (unsigned)(hi - lo + 1)); }

struct Rope { std::vector<int> prims; };       // eight ints per primitive, drawing order

static Rope random_rope(int n_prims, int rows, int cols) {
    Rope r;
    for (int i = 0; i < n_prims; ++i) {
        const int kind = rnd() % 3 == 0 ? 0 : 1;
        const int c0 = rnd_in(-12, cols + 12), r0 = rnd_in(-12, rows + 12);
        const int c1 = kind ? c0 : rnd_in(-12, cols + 12), r1 = kind ? r0 : rnd_in(-12, rows + 12);
        const int size = rnd_in(1, kind ? 9 : 7);
        const int colour = (int)(rnd() & 0xffffffu);
        const int rec[8] = {kind, c0, r0, c1, r1, size, colour, 0};
        r.prims.insert(r.prims.end(), rec, rec + 8);
    }
    return r;
}

static bool covers_literal(const int *rec, int pc, int pr) {
    if (rec[0]) { const long long dx = pc - rec[1], dy = pr - rec[2]; return dx * dx + dy * dy <= (long long)rec[5] * rec[5]; }
    return within_half_width(Px{pc, pr}, Px{rec[1], rec[2]}, Px{rec[3], rec[4]}, rec[5]);
}

static long long picture(int rows, int cols, const std::vector<Rope> &ropes, bool with_occluder) {
    const int P = rows * cols, R = (int)ropes.size();
    // ---- images at exactly their sizes
    unsigned char *colour = (unsigned char *)malloc(3 * (size_t)P), *occ = with_occluder ? (unsigned char *)malloc((size_t)P) : nullptr;
    unsigned char *out = (unsigned char *)malloc(3 * (size_t)P), *want = (unsigned char *)malloc(3 * (size_t)P);
    for (int i = 0; i < 3 * P; ++i) colour[i] = (unsigned char)rnd();
    const unsigned char kinds[6] = {0, 255, 255, 255, 0x5a, 1};
    for (int i = 0; occ && i < P; ++i) occ[i] = kinds[rnd() % 6];
    std::memset(out, 0xa5, 3 * (size_t)P);
    // ---- the table at exactly its size
    size_t n_prims = 0;
    for (const Rope &r : ropes) n_prims += r.prims.size() / 8;
    int *heads = R ? (int *)aligned_alloc(16, 32 * (size_t)R) : nullptr, *prims = n_prims ? (int *)aligned_alloc(16, 32 * n_prims) : nullptr;
    size_t at = 0;
    for (int j = 0; j < R; ++j) {
        const std::vector<int> &p = ropes[j].prims;
        int h[8] = {0, 0, -1, -1, (int)at, (int)(p.size() / 8), 0, 0};
        for (size_t i = 0; i < p.size() / 8; ++i) {
            const int *rec = p.data() + 8 * i;
            const int ext = rec[0] ? rec[5] : (rec[5] + 1) >> 1;
            const int x0 = std::min(rec[1], rec[3]) - ext, x1 = std::max(rec[1], rec[3]) + ext, y0 = std::min(rec[2], rec[4]) - ext, y1 = std::max(rec[2], rec[4]) + ext;
            if (i == 0) { h[0] = x0; h[1] = y0; h[2] = x1; h[3] = y1; }
            else { h[0] = std::min(h[0], x0); h[1] = std::min(h[1], y0); h[2] = std::max(h[2], x1); h[3] = std::max(h[3], y1); }
        }
        std::memcpy(heads + 8 * (size_t)j, h, sizeof h);
        if (!p.empty()) std::memcpy(prims + 8 * at, p.data(), 4 * p.size());
        at += p.size() / 8;
    }
    // ---- the lanes, wave after wave
    for (int wave_first = 0; wave_first < P; wave_first += 256) {
        const RenderSpan sp = render_span(wave_first, P, cols);
        for (int lane = 0; lane < 64; ++lane) {
            const int p0 = wave_first + 4 * lane, n = std::min(4, P - p0);
            unsigned c0, c1, c2, o4, col[4] = {0u, 0u, 0u, 0u}, hit = 0u;
            render_load4(colour, occ, p0, n, c0, c1, c2, o4);
            if (R > 0) hit = render_search4(sp, heads, 0, R, prims, p0, n, cols, lane, col);
            render_store4(out, p0, n, c0, c1, c2, o4, hit, col);
        }
    }
    // ---- the literal statement
    for (int p = 0; p < P; ++p)
        for (int ch = 0; ch < 3; ++ch) {
            const int a = colour[3 * p + ch], s = a + (a & (occ ? occ[p] : 255));
            want[3 * p + ch] = (unsigned char)((s >> 1) + ((s & 1) & ((s >> 1) & 1)));
        }
    for (const Rope &r : ropes)
        for (size_t i = 0; i < r.prims.size() / 8; ++i) {
            const int *rec = r.prims.data() + 8 * i;
            for (int p = 0; p < P; ++p)
                if (covers_literal(rec, p % cols, p / cols)) { want[3 * p] = (unsigned char)rec[6]; want[3 * p + 1] = (unsigned char)(rec[6] >> 8); want[3 * p + 2] = (unsigned char)(rec[6] >> 16); }
        }
    long long bad = 0;
    for (int i = 0; i < 3 * P; ++i) bad += out[i] != want[i];
    if (bad) std::printf("%d x %d, %d ropes: %lld differing bytes\n", rows, cols, R, bad);
    free(colour); free(occ); free(out); free(want); free(heads); free(prims);
    return bad;
}

int main() {
    const int shapes[5][2] = {{1, 1}, {1, 3}, {7, 9}, {33, 65}, {64, 64}};
    long long bad = 0;
    int n = 0;
    for (const auto &s : shapes) {
        const int rows = s[0], cols = s[1];
        for (int variant = 0; variant < 6; ++variant) {
            std::vector<Rope> ropes;
            if (variant == 1) ropes.push_back(random_rope(6, rows, cols));
            if (variant == 2) { ropes.push_back(random_rope(3, rows, cols)); ropes.push_back(random_rope(0, rows, cols)); ropes.push_back(random_rope(9, rows, cols)); }
            if (variant == 3) for (int j = 0; j < 70; ++j) ropes.push_back(random_rope(j % 7 == 3 ? 0 : 3, rows, cols));      // the rope level's round of 64
            if (variant == 4) { ropes.push_back(random_rope(3, rows, cols)); ropes.push_back(random_rope(130, rows, cols)); ropes.push_back(random_rope(3, rows, cols)); }      // the primitive level's rounds
            if (variant == 5) for (int j = 0; j < 129; ++j) ropes.push_back(random_rope(1 + j % 3, rows, cols));
            bad += picture(rows, cols, ropes, variant % 2 == 0);
            ++n;
        }
    }
    std::printf("%d pictures, %lld differing bytes\n", n, bad);
    return bad ? 1 : 0;
}
