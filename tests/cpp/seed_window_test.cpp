// TEST-ONLY host program (tests/test_cpu_seed_window.py):
//   * the closed form of srand(seed)'s window (rsc_core.h rng_seed_word, the code the kernels run)
//     against the Schrage loop (rsc_engine.h rng_seed_window), all 31 words, for the edge seeds and
//     2^20 stratified ones;
//   * RngStream's seed mark and lazily worked-out window: seed() stores no words; reading the
//     window gives the eager one; a copy of an unread stream reads its own; ensure() moving the
//     window clears the mark and leaves the window the eager stream's rebase gives; draws continue.
// Prints one JSON line; exit status 0 when nothing mismatched.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../orb-slam2-optimized_amd/csrc/rsc_core.h"
#include "../../orb-slam2-optimized_amd/csrc/rsc_engine.h"

using namespace rsc;

static long checks = 0, mismatches = 0;

static void check(bool ok, const char* what, uint32_t seed) {
    ++checks;
    if (!ok) {
        if (mismatches < 20) std::fprintf(stderr, "mismatch: %s, seed %u\n", what, seed);
        ++mismatches;
    }
}

static void closed_form(uint32_t seed) {
    uint32_t loop[31];
    rng_seed_window(seed, loop);
    bool same = true;
    for (int j = 0; j < 31; ++j) same = same && rng_seed_word(seed, j) == loop[j];
    check(same, "closed form vs Schrage loop", seed);
}

int main() {
    const uint32_t edges[] = {0u, 1u, 2u, 127773u, 2147483646u, 2147483647u, 2147483648u, 2147483649u, 4294967295u};
    for (uint32_t s : edges) closed_form(s);
    // 2^20 strata of 4096 seeds, one seed each (a multiplicative hash picks the offset)
    long stratified = 0;
    for (uint32_t k = 0; k < (1u << 20); ++k) {
        closed_form(k * 4096u + ((k * 2654435761u) >> 20));
        ++stratified;
    }

    RngTable tab;
    tab.build();
    long moved = 0;
    for (uint32_t s : edges) {
        uint32_t eager[31];
        rng_seed_window(s, eager);
        RngStream r;
        r.seed(s);
        check(r.on_seed_window && !r.have_words && r.seed_value == s && r.g == 310, "seed() stores seed and mark only", s);
        RngStream copy = r;  // an unread stream's copy reads its own words
        check(std::memcmp(copy.window, eager, sizeof(eager)) == 0 && copy.have_words && !r.have_words,
              "copy of an unread stream", s);
        // within the table's reach nothing moves and nothing is read
        r.ensure(tab, kRngTableRows - 310);
        check(r.on_seed_window && !r.have_words && r.g == 310, "ensure() within reach", s);
        check(std::memcmp(r.window, eager, sizeof(eager)) == 0 && r.have_words && r.on_seed_window,
              "materialised window equals the eager one", s);
        // one draw more than the table reaches: the window moves
        for (int used : {0, 1, 5, 1200, kRngTableRows - 310}) {
            RngStream m;
            m.seed(s);
            m.g += used;
            const int g = m.g;
            uint32_t want[31];
            for (int j = 0; j < 31; ++j) {
                const int x = g - 31 + j;
                want[j] = (x >= 0) ? tab.word(eager, x) : eager[31 + x];
            }
            m.ensure(tab, kRngTableRows - g + 1);
            check(!m.on_seed_window && m.have_words && m.g == 0, "ensure() beyond reach clears the mark", s);
            check(std::memcmp(m.window, want, sizeof(want)) == 0, "moved window equals the eager stream's", s);
            bool cont = true;
            for (int k = 0; k < 64 && g + k < kRngTableRows; ++k) cont = cont && tab.word(m.window, k) == tab.word(eager, g + k);
            check(cont, "draws continue across the move", s);
            ++moved;
        }
        RngStream a;
        a.seed(s);
        a.advance(tab, 3 * (int64_t)kRngTableRows + 17);
        check(!a.on_seed_window, "advance() past the reach clears the mark", s);
        RngStream d;
        d.seed(s);
        d.drop_seed_mark();
        check(!d.on_seed_window && d.have_words && std::memcmp(d.window, eager, sizeof(eager)) == 0 && d.g == 310,
              "drop_seed_mark() keeps the words", s);
    }
    std::printf("{\"checks\": %ld, \"mismatches\": %ld, \"edge_seeds\": %zu, \"stratified_seeds\": %ld, \"moved_windows\": %ld}\n",
                checks, mismatches, sizeof(edges) / sizeof(edges[0]), stratified, moved);
    return mismatches ? 1 : 0;
}
