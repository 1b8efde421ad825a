// TEST-ONLY host program: the view-image builder (rsc_viewimage.h) against the offset arithmetic the seven
// image builders of the C ABI carried before they shared it, and the two argument checks that live beside it.
// Each builder is laid out twice per shape: `former` restates what the entry point did (the S3Blob sequence of
// rsc_kfview_create, rsc_frameview_create, rsc_mpview_create and rsc_lastframe_create: a piece at the
// 256-byte boundary behind the previous one, the image ending where the last piece ends; the al256 chain of
// rsc_bow_create, rsc_kfview_set_triangulation and rsc_voc_create: the same, the image closed on a boundary), `now`
// puts the same pieces into a ViewImage with each builder's element types.  Every offset must agree, the new image is
// at least as long as the former one and never empty, the bytes at every offset are the source's, and at()
// on two bases differs by the bases' distance, as do the pointer fields bind() sets (the sanitizer build catches a
// piece that leaves the image).
// Then check_grid_csr on a valid grid and on each way a grid can be wrong, and grid_radius_ok at its bound.
// Prints one JSON line; exit status 1 when anything differed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <new>
#include "../../orb-slam2-optimized_amd/csrc/rsc_viewimage.h"

using namespace rsc;

// The `now` side restates each builder's put sequence by hand with stand-in types: this program pins the builder's
// arithmetic, not the entry points.  That the entry points place and fill every piece as before is pinned on the
// device, by tests/test_gpu_view_sizes.py and the matcher suites.

// stand-ins with the sizes of the device types (rsc_sim3match.h, rsc_projcore.h); the arithmetic under test
// does not depend on them being current
struct F2 { float x, y; };
struct U4 { uint32_t w[4]; };
struct D32 { uint32_t w[8]; };
struct HdrKF { char b[192]; };
struct HdrFrame { char b[112]; };
enum : size_t { kCells = 64 * 48 };

static long g_bad = 0, g_cases = 0, g_pieces = 0;
static std::vector<unsigned char> g_src;  // the pieces' sources: distinct windows of one pseudo-random block

namespace {
struct Was { size_t off, bytes; };
struct Now { size_t off, bytes; const void* src; void* field; };  // field: the pointer bind() sets
struct Former {
    std::vector<Was> p;
    size_t size = 0;                              // the image's length so far
    static size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
    void add(size_t bytes) {                      // S3Blob::add / reserve, and a link of an al256 chain
        const size_t off = al(size);
        p.push_back({off, bytes});
        size = off + bytes;
    }
};
struct Built {
    ViewImage img;
    std::vector<Now> p;
    const void* next_src() const { return g_src.data() + 4099 * p.size(); }
    template <class T>
    const T*& field() { return *new (std::malloc(sizeof(const T*))) const T*(nullptr); }
    template <class T>
    void put(size_t count) {
        const void* s = next_src();
        const T*& f = field<T>();
        p.push_back({img.put(f, s, count).off, sizeof(T) * count, s, &f});
    }
    // a held piece is filled afterwards through at(), as the header structs and the gathered descriptors are
    template <class T>
    void hold(size_t count) {
        const void* s = next_src();
        const T*& f = field<T>();
        const Piece<T> piece = img.hold(f, count);
        p.push_back({piece.off, sizeof(T) * count, s, &f});
        if (count) std::memcpy(at(img.h.data(), piece), s, sizeof(T) * count);
        if ((char*)at(img.h.data(), piece) != img.h.data() + piece.off) ++g_bad;
    }
};
}  // namespace

static void fail(const char* name, const char* what, size_t i) {
    ++g_bad;
    std::fprintf(stderr, "%s: %s (piece %zu)\n", name, what, i);
}

static void check(const char* name, const Former& was, size_t former_bytes, Built& now) {
    ++g_cases;
    const size_t bytes = now.img.finish();
    if (bytes != now.img.h.size() || bytes == 0 || bytes < former_bytes) fail(name, "image length", 0);
    if (was.p.size() != now.p.size()) return fail(name, "piece count", 0);
    char* base = now.img.h.data();
    std::vector<char> two(bytes + 4096);  // a second and a third base, 4096 bytes apart
    for (size_t i = 0; i < now.p.size(); ++i) {
        ++g_pieces;
        const Now& q = now.p[i];
        if (q.off != was.p[i].off || q.bytes != was.p[i].bytes) fail(name, "offset differs", i);
        if (q.off % 256 || q.off + q.bytes > bytes) fail(name, "alignment / end", i);
        if (q.bytes && std::memcmp(base + q.off, q.src, q.bytes) != 0) fail(name, "bytes differ from the source", i);
        const Piece<D32> piece{q.off};
        if ((char*)at(two.data() + 4096, piece) - (char*)at(two.data(), piece) != 4096 ||
            (char*)at(two.data(), piece) != two.data() + q.off)
            fail(name, "at() on two bases", i);
    }
    for (char* d : {two.data(), two.data() + 4096}) {  // and the fields bind() sets
        now.img.bind(d);
        for (size_t i = 0; i < now.p.size(); ++i) {
            char* got;
            std::memcpy(&got, now.p[i].field, sizeof(got));
            if (got != d + now.p[i].off) fail(name, "bind()", i);
        }
    }
    for (const Now& q : now.p) std::free(q.field);
}

// ---- rsc_kfview_create: header | kp | octave | desc | cell_begin | cell_feat | scale | mp_state | mp_pos |
// mp_dmax | mp_dmin | mp_desc ----
static void kfview(size_t n, size_t nf, size_t nl) {
    Former f;
    f.add(sizeof(HdrKF));
    for (size_t b : {8 * n, 4 * n, 32 * n, 4 * (kCells + 1), 4 * nf, 4 * nl, n, 12 * n, 4 * n, 4 * n, 32 * n}) f.add(b);
    Built b;
    b.hold<HdrKF>(1);
    b.put<F2>(n); b.put<int32_t>(n); b.put<U4>(2 * n); b.put<int32_t>(kCells + 1); b.put<int32_t>(nf);
    b.put<float>(nl); b.put<uint8_t>(n); b.put<float>(3 * n); b.put<float>(n); b.put<float>(n); b.put<U4>(2 * n);
    check("kfview", f, f.size, b);
}
// ---- rsc_frameview_create: header | kp | octave | angle | desc | cell_begin | cell_feat | scale ----
static void frameview(size_t n, size_t nf, size_t nl) {
    Former f;
    f.add(sizeof(HdrFrame));
    for (size_t b : {8 * n, 4 * n, 4 * n, 32 * n, 4 * (kCells + 1), 4 * nf, 4 * nl}) f.add(b);
    Built b;
    b.hold<HdrFrame>(1);
    b.put<F2>(n); b.put<int32_t>(n); b.put<float>(n); b.put<D32>(n); b.put<int32_t>(kCells + 1);
    b.put<int32_t>(nf); b.put<float>(nl);
    check("frameview", f, f.size, b);
}
// ---- rsc_mpview_create: state | pos | normal | dmax | dmin | desc | a spare 256-byte block ----
static void mpview(size_t n) {
    Former f;
    for (size_t b : {n, 12 * n, 12 * n, 4 * n, 4 * n, 32 * n, (size_t)256}) f.add(b);
    Built b;
    b.put<uint8_t>(n); b.put<float>(3 * n); b.put<float>(3 * n); b.put<float>(n); b.put<float>(n); b.put<D32>(n);
    b.hold<char>(256);
    check("mpview", f, f.size, b);
}
// ---- rsc_lastframe_create: octave | angle | mp_state | mp_pos | mp_desc | mp_has_obs | a spare block ----
static void lastframe(size_t n) {
    Former f;
    for (size_t b : {4 * n, 4 * n, n, 12 * n, 32 * n, n, (size_t)256}) f.add(b);
    Built b;
    b.put<int32_t>(n); b.put<float>(n); b.put<uint8_t>(n); b.put<float>(3 * n); b.put<D32>(n); b.put<uint8_t>(n);
    b.hold<char>(256);
    check("lastframe", f, f.size, b);
}
// ---- rsc_bow_create: desc | desc_fv (gathered) | angle | node_id | node_begin | feat; the chain's total
// closes on a boundary ----
static void bow(size_t n, size_t nf, size_t nn) {
    Former f;
    for (size_t b : {32 * n, 32 * nf, 4 * n, 4 * nn, 4 * (nn + 1), 4 * nf}) f.add(b);
    Built b;
    b.put<U4>(2 * n); b.hold<U4>(2 * nf); b.put<float>(n); b.put<uint32_t>(nn); b.hold<int32_t>(nn + 1);
    b.put<uint32_t>(nf);
    check("bow", f, Former::al(f.size), b);
}
// ---- rsc_kfview_set_triangulation: kp_raw | u_right | depth | cos_stereo; at least 256 bytes ----
static void triangulation(size_t n) {
    Former f;
    for (size_t b : {8 * n, 4 * n, 4 * n, 4 * n}) f.add(b);
    Built b;
    b.put<float>(2 * n); b.put<float>(n); b.put<float>(n); b.put<float>(n);
    check("triangulation", f, std::max(Former::al(f.size), (size_t)256), b);
}

// ---- rsc_voc_create: desc | rec | orig | word | weight, each filled node by node; the chain's total closes on a
// boundary ----
static void vocabulary(size_t nn) {
    Former f;
    for (size_t b : {32 * nn, 8 * nn, 4 * nn, 4 * nn, 8 * nn}) f.add(b);
    Built b;
    b.hold<U4>(2 * nn); b.hold<F2>(nn); b.hold<uint32_t>(nn); b.hold<uint32_t>(nn); b.hold<double>(nn);
    check("vocabulary", f, Former::al(f.size), b);
}

static long grid_checks() {
    long done = 0;
    auto expect = [&](const char* what, const std::vector<int32_t>& cb, const int32_t* cf, int n, int want,
                      const char* want_err) {
        std::string err;
        const int got = check_grid_csr(cb.data(), cf, (int)cb.size() - 1, n, err);
        if (got != want || err != want_err) fail("check_grid_csr", what, 0);
        ++done;
    };
    const std::vector<int32_t> feat = {2, 0, 1, 2};
    expect("a valid grid", {0, 1, 1, 4}, feat.data(), 3, 0, "");
    expect("cell_begin[0] != 0", {1, 1, 1, 4}, feat.data(), 3, RSC_ERR_ARG, "");
    expect("a decreasing offset", {0, 2, 1, 4}, feat.data(), 3, RSC_ERR_ARG, "");
    const std::vector<int32_t> at_n = {2, 0, 3, 1};
    expect("an index equal to n", {0, 1, 1, 4}, at_n.data(), 3, RSC_ERR_ARG, "mGrid index out of range");
    const std::vector<int32_t> neg = {2, -1, 1, 0};
    expect("a negative index", {0, 1, 1, 4}, neg.data(), 3, RSC_ERR_ARG, "mGrid index out of range");
    expect("nf > 0 with a null cell_feat", {0, 1, 1, 4}, nullptr, 3, RSC_ERR_ARG, "");
    return done;
}

static long radius_checks() {
    const float bound = 1073741824.0f;  // 2^30
    const float below = std::nextafter(bound, 0.0f);
    long done = 0;
    auto expect = [&](const char* what, float r, bool want) {
        if (grid_radius_ok(r, 1.0f, 1.0f, 0.5f) != want || grid_radius_ok(r, 1.0f, 0.5f, 1.0f) != want)
            fail("grid_radius_ok", what, 0);
        ++done;
    };
    expect("the largest float below 2^30", below, true);
    expect("2^30", bound, false);
    expect("NaN", std::numeric_limits<float>::quiet_NaN(), false);
    return done;
}

int main() {
    g_src.resize(4099 * 16 + 64 * 8192 + 4096);
    uint32_t x = 12345;
    for (unsigned char& c : g_src) c = (unsigned char)((x = x * 1664525u + 1013904223u) >> 24);
    const size_t ns[] = {0, 1, 7, 255, 256, 257, 8192};
    for (size_t n : ns) {
        for (size_t nf : {(size_t)0, (size_t)1, (size_t)257, (size_t)8192})
            for (size_t nl : {(size_t)0, (size_t)1, (size_t)8, (size_t)64}) {
                kfview(n, nf, nl);
                frameview(n, nf, nl);
            }
        for (size_t nf : {(size_t)0, (size_t)1, (size_t)257, n})
            for (size_t nn : {(size_t)0, (size_t)1, (size_t)257}) bow(n, nf, nn);
        mpview(n);
        lastframe(n);
        triangulation(n);
        vocabulary(n + 2);  // a vocabulary has at least two nodes
    }
    const long grids = grid_checks(), radii = radius_checks();
    std::printf("{\"cases\": %ld, \"pieces\": %ld, \"grid_checks\": %ld, \"radius_checks\": %ld, \"mismatches\": %ld}\n",
                g_cases, g_pieces, grids, radii, g_bad);
    return g_bad ? 1 : 0;
}
