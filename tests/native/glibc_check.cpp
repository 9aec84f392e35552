// The device generator's host-built tables (kb2e_amd/csrc/glibc_rand.hpp) against
// plainly stepping GlibcRand::next_raw:
//   * words 0..L-1 of glibc_jump_table(L, .) applied to a window;
//   * glibc_pow_table's squares M^(2^k), k <= 15, applied to the window: the
//     window after L * 2^k words;
//   * composite block numbers p, multiplied up from p's set bits in ascending
//     order exactly as glibc_starts_pow_kernel (kernels_glibc.hpp) does;
//   * window / set_window / commit round trips.
// argv[1] = seed.  Prints "ok <checks>" and returns 0, or the first mismatch and 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "glibc_rand.hpp"

using kb2e::GlibcRand;

constexpr int D = GlibcRand::kDeg;
constexpr int L = 4096;     // kGlibcBlock (engine.hip)
constexpr int kLevels = 16;  // k <= 15: every level the 16M-sample epoch uses

static long checks = 0;

static bool same(const uint32_t* a, const uint32_t* b, int n, const char* what, long tag) {
    ++checks;
    for (int i = 0; i < n; ++i)
        if (a[i] != b[i]) {
            printf("%s %ld: word %d is %u, stepping gives %u\n", what, tag, i, a[i], b[i]);
            return false;
        }
    return true;
}

// out = A x (A row-major 31 x 31, mod 2^32)
static void apply(const uint32_t* A, const uint32_t* x, uint32_t* out) {
    for (int l = 0; l < D; ++l) {
        uint32_t v = 0;
        for (int m = 0; m < D; ++m) v += A[l * D + m] * x[m];
        out[l] = v;
    }
}

// commit(vals, m) and set_window(window()) leave a generator that goes on as the stepped one
static bool round_trips(const GlibcRand& start, const char* what) {
    const long ms[] = {0, 1, 30, 31, 32, 4097};
    for (long m : ms) {
        GlibcRand stepped = start, committed = start;
        std::vector<uint32_t> vals((size_t)m + 1);
        for (long q = 0; q < m; ++q) vals[q] = stepped.next_raw();
        committed.commit(vals.data(), m);
        uint32_t ws[D], wc[D];
        stepped.window(ws);
        committed.window(wc);
        if (!same(wc, ws, D, what, m)) return false;
        GlibcRand rebuilt(1);
        rebuilt.set_window(ws);
        uint32_t a[100], b[100], c[100];
        for (int q = 0; q < 100; ++q) {
            a[q] = stepped.next_raw();
            b[q] = committed.next_raw();
            c[q] = rebuilt.next_raw();
        }
        if (!same(b, a, 100, "words after commit", m) || !same(c, a, 100, "words after set_window", m)) return false;
    }
    return true;
}

int main(int argc, char** argv) {
    const uint32_t seed = argc > 1 ? (uint32_t)strtoul(argv[1], nullptr, 10) : 1u;
    std::vector<uint32_t> C((size_t)D * L), P((size_t)kLevels * D * D);
    kb2e::glibc_jump_table(L, C.data());
    kb2e::glibc_pow_table(L, kLevels, C.data(), P.data());

    GlibcRand g(seed);
    for (int q = 0; q < 5; ++q) (void)g.next();  // (not the state srandom leaves: f = 8)
    uint32_t w0[D];
    g.window(w0);

    // the jump table's words
    {
        GlibcRand s = g;
        std::vector<uint32_t> got(L), want(L);
        for (int t = 0; t < L; ++t) {
            uint32_t v = 0;
            for (int m = 0; m < D; ++m) v += C[(size_t)m * L + t] * w0[m];
            got[t] = v;
            want[t] = s.next_raw();
        }
        if (!same(got.data(), want.data(), L, "jump table, seed", seed)) return 1;
    }

    // windows before block p: the squares and the composite block numbers, one stepping run
    std::vector<long> blocks;
    for (int k = 0; k < kLevels; ++k) blocks.push_back(1l << k);
    for (long p : {1l, 2l, 3l, 1099l, 19531l, 0x5A5Al}) blocks.push_back(p);
    std::sort(blocks.begin(), blocks.end());
    blocks.erase(std::unique(blocks.begin(), blocks.end()), blocks.end());
    GlibcRand s = g;
    long at = 0;
    for (long p : blocks) {
        for (; at < p * L; ++at) (void)s.next_raw();
        uint32_t want[D], cur[D], nxt[D];
        s.window(want);
        for (int m = 0; m < D; ++m) cur[m] = w0[m];
        for (int k = 0; (p >> k) != 0; ++k) {  // glibc_starts_pow_kernel's loop
            if (!((p >> k) & 1)) continue;
            apply(P.data() + (size_t)k * D * D, cur, nxt);
            for (int m = 0; m < D; ++m) cur[m] = nxt[m];
        }
        if (!same(cur, want, D, "window before block", p)) return 1;
    }

    if (!round_trips(g, "commit from the seeded state")) return 1;
    GlibcRand h(1);
    h.set_window(w0);  // f = 0
    if (!round_trips(h, "commit after set_window")) return 1;
    printf("ok %ld\n", checks);
    return 0;
}
