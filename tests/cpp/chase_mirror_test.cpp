// TEST-ONLY host program: tridiag_qr<double, 12> (rsc_core.h) with a rotation sink that has none of
// the optional hooks against sinks that opt into mirror() and / or any_lane() — the forms the split
// eigen stage's chase wave runs — on the same inputs.  diag, sub, perm, the return value and the
// full list of (k, c, s, apply) calls must agree bit for bit.  Prints one JSON line with the number
// of matrices per input class; exit status 1 on the first mismatch.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "../../orb-slam2-optimized_amd/csrc/rsc_core.h"

using namespace rsc;

struct Call {
    int k;
    double c, s;
    bool apply;
};

struct PlainSink {
    std::vector<Call>* log;
    void operator()(int k, double c, double s, bool apply) { log->push_back({k, c, s, apply}); }
};
// the mirror is a plain array of 23 doubles, poisoned before the run (tridiag_qr fills it)
struct MirrorSink : PlainSink {
    double* m;
    long* reads;
    double* mirror() const {
        ++*reads;
        return m;
    }
};
struct TrimSink : PlainSink {
    bool any_lane(bool p) const { return p; }
};
struct MirrorTrimSink : MirrorSink {
    bool any_lane(bool p) const { return p; }
};
// another lane of the wave may still need a range this lane has left: any_lane() answers true more
// often than p alone
struct MirrorTrimWaveSink : MirrorSink {
    uint64_t* rng;
    bool any_lane(bool p) const {
        *rng = *rng * 6364136223846793005ull + 1442695040888963407ull;
        return p | ((*rng >> 62) == 0);
    }
};
static_assert(!qr_has_mirror<PlainSink>::value && !qr_has_any_lane<PlainSink>::value, "plain sink");
static_assert(qr_has_mirror<MirrorSink>::value && !qr_has_any_lane<MirrorSink>::value, "mirror sink");
static_assert(!qr_has_mirror<TrimSink>::value && qr_has_any_lane<TrimSink>::value, "trim sink");
static_assert(qr_has_mirror<MirrorTrimSink>::value && qr_has_any_lane<MirrorTrimSink>::value, "both hooks");
static_assert(RSC_QR_MIRROR && RSC_QR_TRIM, "the hooks are compiled in");

struct Result {
    double diag[12], sub[11];
    int perm[12];
    bool ok;
    std::vector<Call> calls;
};

template <class Sink>
static void run(const double* d, const double* s, Sink sink, Result& r) {
    std::memcpy(r.diag, d, sizeof(r.diag));
    std::memcpy(r.sub, s, sizeof(r.sub));
    r.calls.clear();
    sink.log = &r.calls;
    r.ok = tridiag_qr<double, 12>(r.diag, r.sub, sink, r.perm);
}

static bool same(const Result& a, const Result& b) {
    if (a.ok != b.ok || std::memcmp(a.diag, b.diag, sizeof(a.diag)) || std::memcmp(a.sub, b.sub, sizeof(a.sub)) ||
        std::memcmp(a.perm, b.perm, sizeof(a.perm)) || a.calls.size() != b.calls.size())
        return false;
    for (size_t i = 0; i < a.calls.size(); ++i) {
        const Call &x = a.calls[i], &y = b.calls[i];
        if (x.k != y.k || x.apply != y.apply || std::memcmp(&x.c, &y.c, 8) || std::memcmp(&x.s, &y.s, 8)) return false;
    }
    return true;
}

struct Rng {
    uint64_t s;
    uint64_t next() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return s;
    }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }  // [0, 1)
    double sym() { return 2.0 * uni() - 1.0; }
    int below(int n) { return (int)(next() % (uint64_t)n); }
    double scale() { return std::pow(10.0, 16.0 * uni() - 8.0); }  // 1e-8 .. 1e8
};

static long g_reads = 0, g_rotations = 0, g_not_converged = 0;

static bool check(const char* cls, long idx, const double* d, const double* s, uint64_t seed) {
    Result ref, r;
    run(d, s, PlainSink{}, ref);
    g_rotations += (long)ref.calls.size();
    g_not_converged += !ref.ok;
    double m[23];
    const double poison = std::numeric_limits<double>::signaling_NaN();
    const char* form = nullptr;
    for (int i = 0; i < 23; ++i) m[i] = poison;
    MirrorSink ms;
    ms.m = m;
    ms.reads = &g_reads;
    run(d, s, ms, r);
    if (!same(ref, r)) form = "mirror";
    run(d, s, TrimSink{}, r);
    if (!form && !same(ref, r)) form = "any_lane";
    for (int i = 0; i < 23; ++i) m[i] = poison;
    MirrorTrimSink mt;
    mt.m = m;
    mt.reads = &g_reads;
    run(d, s, mt, r);
    if (!form && !same(ref, r)) form = "mirror + any_lane";
    for (int i = 0; i < 23; ++i) m[i] = poison;
    MirrorTrimWaveSink mw;
    mw.m = m;
    mw.reads = &g_reads;
    mw.rng = &seed;
    run(d, s, mw, r);
    if (!form && !same(ref, r)) form = "mirror + any_lane (wave)";
    if (form) {
        std::fprintf(stderr, "MISMATCH class %s matrix %ld form %s\n", cls, idx, form);
        return false;
    }
    return true;
}

static void random_tridiag(Rng& g, double* d, double* s) {
    // one scale for the matrix, or one per entry (graded matrices deflate in the middle)
    const bool graded = g.below(4) == 0;
    const double sc = g.scale();
    for (int i = 0; i < 12; ++i) d[i] = g.sym() * (graded ? g.scale() : sc);
    for (int i = 0; i < 11; ++i) s[i] = g.sym() * (graded ? g.scale() : sc);
}

int main() {
    Rng g{0x9E3779B97F4A7C15ull};
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double d[12], s[11];
    long n_random = 0, n_mid = 0, n_multi = 0, n_conv = 0, n_nan_all = 0, n_nan_above = 0, n_nan_below = 0;
    // random symmetric tridiagonals, scales 1e-8 .. 1e8
    for (; n_random < 12000; ++n_random) {
        random_tridiag(g, d, s);
        if (!check("random", n_random, d, s, g.next())) return 1;
    }
    // one exactly zero sub-diagonal entry in the middle: start > 0 from the first step
    for (; n_mid < 2000; ++n_mid) {
        random_tridiag(g, d, s);
        s[1 + g.below(9)] = (g.below(2) ? 0.0 : -0.0);
        if (!check("mid_zero", n_mid, d, s, g.next())) return 1;
    }
    // several zero entries
    for (; n_multi < 2000; ++n_multi) {
        random_tridiag(g, d, s);
        const int nz = 2 + g.below(6);
        for (int j = 0; j < nz; ++j) s[g.below(11)] = 0.0;
        if (!check("multi_zero", n_multi, d, s, g.next())) return 1;
    }
    // already converged
    for (; n_conv < 200; ++n_conv) {
        random_tridiag(g, d, s);
        for (int i = 0; i < 11; ++i) s[i] = (n_conv & 1) ? -0.0 : 0.0;
        if (!check("converged", n_conv, d, s, g.next())) return 1;
    }
    // the block start..end all NaN (the Q4 exit): the whole matrix, or the bottom block below a zero
    for (; n_nan_all < 400; ++n_nan_all) {
        random_tridiag(g, d, s);
        const int st = (n_nan_all & 1) ? 1 + g.below(10) : 0;
        for (int i = st; i < 12; ++i) d[i] = nan;
        for (int i = st; i < 11; ++i) s[i] = nan;
        if (st > 0) s[st - 1] = 0.0;
        if (!check("nan_block", n_nan_all, d, s, g.next())) return 1;
    }
    // a NaN block above a finite block (rows 0..j NaN, rows j+1..11 finite): the finite block
    // converges first, then the NaN block ends the iteration
    for (; n_nan_above < 400; ++n_nan_above) {
        random_tridiag(g, d, s);
        const int j = 1 + g.below(9);
        for (int i = 0; i <= j; ++i) d[i] = nan;
        for (int i = 0; i < j; ++i) s[i] = nan;
        s[j] = 0.0;
        if (!check("nan_above_finite", n_nan_above, d, s, g.next())) return 1;
    }
    // a NaN block in the middle, finite blocks on both sides
    for (; n_nan_below < 400; ++n_nan_below) {
        random_tridiag(g, d, s);
        const int a = 1 + g.below(5), b = a + 1 + g.below(4);  // NaN rows a..b, b <= 10
        for (int i = a; i <= b; ++i) d[i] = nan;
        for (int i = a; i < b; ++i) s[i] = nan;
        s[a - 1] = 0.0;
        s[b] = 0.0;
        if (!check("nan_middle", n_nan_below, d, s, g.next())) return 1;
    }
    std::printf("{\"random\": %ld, \"mid_zero\": %ld, \"multi_zero\": %ld, \"converged\": %ld, \"nan_block\": %ld, "
                "\"nan_above_finite\": %ld, \"nan_middle\": %ld, \"mirror_runs\": %ld, \"rotations\": %ld, "
                "\"not_converged\": %ld, \"mismatches\": 0}\n",
                n_random, n_mid, n_multi, n_conv, n_nan_all, n_nan_above, n_nan_below, g_reads, g_rotations,
                g_not_converged);
    return 0;
}
