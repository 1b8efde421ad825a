// TEST-ONLY host program: the staging-arena cursor (rsc_arena.h) against the offset arithmetic the six
// batched matchers (now in rsc_matchers.cpp) carried before they shared it.  Each layout is built twice for a few
// tiny shapes: `was_*` restates the former three loops (own `al`, own running `off`), `now_*` takes the
// same pieces from an Arena in the order the entry point takes them.  Every offset, up, back and bytes must
// agree; two shapes are also checked against numbers worked out by hand.  Then, per layout:
// up <= back <= bytes, every piece lies in its section, a piece starts on a 256-byte boundary unless it
// follows a problem's packed count words (then it starts where they end, on a multiple of its element's
// alignment), the count words end at or before the next piece, and no two pieces overlap: each piece is
// memset to its index in a heap block of `bytes` and read back (the sanitizer build catches a piece that
// leaves the block).  Prints one JSON line; exit status 1 when anything differed.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../orb-slam2-optimized_amd/csrc/rsc_arena.h"

using rsc::Arena;

// element and table sizes of the device structs (rsc_*proj.h, rsc_sim3match.h); the arithmetic under test
// does not depend on them being current
enum : size_t { kSim3Pair = 112, kFrameProb = 192, kKfProb = 296, kFuseProb = 192, kLocalProb = 216, kLastProb = 192,
                kProjRec = 16, kProjCand = 16, kLpRec = 32, kLpTrack = 24 };

enum Section { UP = 0, SCRATCH = 1, BACK = 2 };
struct Piece {
    const char* name;
    int c;  // problem, -1: the table
    size_t off, size;
    Section sec;
    size_t align;  // of the element type
    bool packed;
};
struct Layout {
    std::vector<Piece> p;
    size_t up = 0, back = 0, bytes = 0;
    void add(const char* name, int c, size_t off, size_t size, Section sec, size_t align = 1, bool packed = false) {
        p.push_back({name, c, off, size, sec, align, packed});
    }
};
struct Shape { int a, b; };  // the two sizes of one problem
typedef std::vector<Shape> Shapes;

static size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
static size_t m1(int n) { return (size_t)std::max(n, 1); }

// ---- rsc_search_by_sim3_many: a = kf1->n, b = kf2->n ----
static Layout was_sim3(const Shapes& s) {
    Layout L;
    const int count = (int)s.size();
    L.add("table", -1, 0, kSim3Pair * count, UP, 8);
    size_t off = al(kSim3Pair * count);
    for (int c = 0; c < count; ++c) {
        L.add("a1", c, off, m1(s[c].a), UP); off = al(off + m1(s[c].a));
        L.add("a2", c, off, m1(s[c].b), UP); off = al(off + m1(s[c].b));
    }
    L.up = off;
    for (int c = 0; c < count; ++c) {
        L.add("m1", c, off, 4 * m1(s[c].a), SCRATCH, 4); off = al(off + 4 * m1(s[c].a));
        L.add("m2", c, off, 4 * m1(s[c].b), SCRATCH, 4); off = al(off + 4 * m1(s[c].b));
    }
    L.back = off;
    for (int c = 0; c < count; ++c) {
        L.add("out", c, off, 4 * m1(s[c].a), BACK, 4); off = al(off + 4 * m1(s[c].a));
        L.add("nf", c, off, 4, BACK, 4, true); off += 4;
    }
    L.bytes = al(off);
    return L;
}
static Layout now_sim3(const Shapes& s) {
    Layout L;
    const int count = (int)s.size();
    Arena A;
    L.add("table", -1, A.take(kSim3Pair * count), kSim3Pair * count, UP, 8);
    for (int c = 0; c < count; ++c) {
        L.add("a1", c, A.take(m1(s[c].a)), m1(s[c].a), UP);
        L.add("a2", c, A.take(m1(s[c].b)), m1(s[c].b), UP);
    }
    A.end_upload();
    for (int c = 0; c < count; ++c) {
        L.add("m1", c, A.take(4 * m1(s[c].a)), 4 * m1(s[c].a), SCRATCH, 4);
        L.add("m2", c, A.take(4 * m1(s[c].b)), 4 * m1(s[c].b), SCRATCH, 4);
    }
    A.end_scratch();
    for (int c = 0; c < count; ++c) {
        L.add("out", c, A.take(4 * m1(s[c].a)), 4 * m1(s[c].a), BACK, 4);
        L.add("nf", c, A.take_packed(4), 4, BACK, 4, true);
    }
    A.finish();
    L.up = A.up; L.back = A.back; L.bytes = A.bytes;
    return L;
}

// ---- the three matchers with  table | two flag rows | rec, cand, claim | out | count words:
// rsc_search_by_projection_many (a = kf->n, b = frame->n; second row 4 bytes an element, scratch sized by a,
// out by b), rsc_search_by_projection_kf_many (a = points->n, b = kf->n; second row 1 byte an element) ----
static Layout was_proj(const Shapes& s, size_t table, size_t row2) {
    Layout L;
    const int count = (int)s.size();
    L.add("table", -1, 0, table * count, UP, 8);
    size_t off = al(table * count);
    for (int c = 0; c < count; ++c) {
        L.add("already", c, off, m1(s[c].a), UP); off = al(off + m1(s[c].a));
        L.add("row2", c, off, row2 * m1(s[c].b), UP, row2); off = al(off + row2 * m1(s[c].b));
    }
    L.up = off;
    for (int c = 0; c < count; ++c) {
        L.add("rec", c, off, kProjRec * m1(s[c].a), SCRATCH, 16); off = al(off + kProjRec * m1(s[c].a));
        L.add("cand", c, off, kProjCand * m1(s[c].a), SCRATCH, 16); off = al(off + kProjCand * m1(s[c].a));
        L.add("claim", c, off, 4 * m1(s[c].a), SCRATCH, 4); off = al(off + 4 * m1(s[c].a));
    }
    L.back = off;
    for (int c = 0; c < count; ++c) {
        L.add("out", c, off, 4 * m1(s[c].b), BACK, 4); off = al(off + 4 * m1(s[c].b));
        L.add("cnt", c, off, 8, BACK, 4, true); off += 8;
    }
    L.bytes = al(off);
    return L;
}
static Layout now_proj(const Shapes& s, size_t table, size_t row2) {
    Layout L;
    const int count = (int)s.size();
    Arena A;
    L.add("table", -1, A.take(table * count), table * count, UP, 8);
    for (int c = 0; c < count; ++c) {
        L.add("already", c, A.take(m1(s[c].a)), m1(s[c].a), UP);
        L.add("row2", c, A.take(row2 * m1(s[c].b)), row2 * m1(s[c].b), UP, row2);
    }
    A.end_upload();
    for (int c = 0; c < count; ++c) {
        const size_t n = m1(s[c].a);
        L.add("rec", c, A.take(kProjRec * n), kProjRec * n, SCRATCH, 16);
        L.add("cand", c, A.take(kProjCand * n), kProjCand * n, SCRATCH, 16);
        L.add("claim", c, A.take(4 * n), 4 * n, SCRATCH, 4);
    }
    A.end_scratch();
    for (int c = 0; c < count; ++c) {
        L.add("out", c, A.take(4 * m1(s[c].b)), 4 * m1(s[c].b), BACK, 4);
        L.add("cnt", c, A.take_packed(8), 8, BACK, 4, true);
    }
    A.finish();
    L.up = A.up; L.back = A.back; L.bytes = A.bytes;
    return L;
}

// ---- rsc_fuse_sim3_many: np = s[0].a for every problem, rows of one stride ----
static Layout was_fuse(const Shapes& s) {
    Layout L;
    const size_t count = s.size(), np = m1(s[0].a);
    const size_t row = al(np), row4 = al(4 * np);
    const size_t o_in = al(kFuseProb * count);
    const size_t back = o_in + row * count;
    L.add("table", -1, 0, kFuseProb * count, UP, 8);
    for (size_t c = 0; c < count; ++c) L.add("in_kf", (int)c, o_in + row * c, np, UP);
    for (size_t c = 0; c < count; ++c) L.add("best", (int)c, back + row4 * c, 4 * np, BACK, 4);
    L.up = L.back = back;
    L.bytes = back + row4 * count;
    return L;
}
static Layout now_fuse(const Shapes& s) {
    Layout L;
    const size_t count = s.size(), np = m1(s[0].a);
    const size_t row = rsc::al256(np), row4 = rsc::al256(4 * np);
    Arena A;
    L.add("table", -1, A.take(kFuseProb * count), kFuseProb * count, UP, 8);
    const size_t o_in = A.take(row * count);
    A.end_upload();
    A.end_scratch();
    const size_t o_best = A.take(row4 * count);
    A.finish();
    for (size_t c = 0; c < count; ++c) L.add("in_kf", (int)c, o_in + row * c, np, UP);
    for (size_t c = 0; c < count; ++c) L.add("best", (int)c, o_best + row4 * c, 4 * np, BACK, 4);
    L.up = A.up; L.back = A.back; L.bytes = A.bytes;
    return L;
}

// ---- local_points_impl: a = points->n, b = frame->n; the track records go up (matcher only) or come back (fused) ----
static Layout was_local(const Shapes& s, bool fused) {
    Layout L;
    const int count = (int)s.size();
    L.add("table", -1, 0, kLocalProb * count, UP, 8);
    size_t off = al(kLocalProb * count);
    for (int c = 0; c < count; ++c) {
        const size_t np = m1(s[c].a), nf = m1(s[c].b);
        L.add("skip", c, off, np, UP); off = al(off + np);
        L.add("has_obs", c, off, np, UP); off = al(off + np);
        L.add("occ", c, off, nf, UP); off = al(off + nf);
        if (!fused) { L.add("track", c, off, kLpTrack * np, UP, 8); off = al(off + kLpTrack * np); }
    }
    L.up = off;
    for (int c = 0; c < count; ++c) {
        const size_t np = m1(s[c].a);
        L.add("rec", c, off, kLpRec * np, SCRATCH, 16); off = al(off + kLpRec * np);
        L.add("cand", c, off, kProjCand * np, SCRATCH, 16); off = al(off + kProjCand * np);
        L.add("claim", c, off, 4 * np, SCRATCH, 4); off = al(off + 4 * np);
    }
    L.back = off;
    for (int c = 0; c < count; ++c) {
        const size_t np = m1(s[c].a);
        if (fused) { L.add("track", c, off, kLpTrack * np, BACK, 8); off = al(off + kLpTrack * np); }
        L.add("out", c, off, 4 * m1(s[c].b), BACK, 4); off = al(off + 4 * m1(s[c].b));
        L.add("cnt", c, off, 16, BACK, 4, true); off += 16;
    }
    L.bytes = al(off);
    return L;
}
static Layout now_local(const Shapes& s, bool fused) {
    Layout L;
    const int count = (int)s.size();
    Arena A;
    L.add("table", -1, A.take(kLocalProb * count), kLocalProb * count, UP, 8);
    for (int c = 0; c < count; ++c) {
        const size_t np = m1(s[c].a), nf = m1(s[c].b);
        L.add("skip", c, A.take(np), np, UP);
        L.add("has_obs", c, A.take(np), np, UP);
        L.add("occ", c, A.take(nf), nf, UP);
        if (!fused) L.add("track", c, A.take(kLpTrack * np), kLpTrack * np, UP, 8);
    }
    A.end_upload();
    for (int c = 0; c < count; ++c) {
        const size_t np = m1(s[c].a);
        L.add("rec", c, A.take(kLpRec * np), kLpRec * np, SCRATCH, 16);
        L.add("cand", c, A.take(kProjCand * np), kProjCand * np, SCRATCH, 16);
        L.add("claim", c, A.take(4 * np), 4 * np, SCRATCH, 4);
    }
    A.end_scratch();
    for (int c = 0; c < count; ++c) {
        const size_t np = m1(s[c].a);
        if (fused) L.add("track", c, A.take(kLpTrack * np), kLpTrack * np, BACK, 8);
        L.add("out", c, A.take(4 * m1(s[c].b)), 4 * m1(s[c].b), BACK, 4);
        L.add("cnt", c, A.take_packed(16), 16, BACK, 4, true);
    }
    A.finish();
    L.up = A.up; L.back = A.back; L.bytes = A.bytes;
    return L;
}

// ---- rsc_search_by_projection_last_many: a = frame->n, b = last->n ----
static Layout was_last(const Shapes& s) {
    Layout L;
    const int count = (int)s.size();
    L.add("table", -1, 0, kLastProb * count, UP, 8);
    size_t off = al(kLastProb * count);
    for (int c = 0; c < count; ++c) {
        L.add("occ", c, off, m1(s[c].a), UP); off = al(off + m1(s[c].a));
    }
    L.up = off;
    for (int c = 0; c < count; ++c) {
        const size_t nl = m1(s[c].b);
        L.add("rec", c, off, kLpRec * nl, SCRATCH, 16); off = al(off + kLpRec * nl);
        L.add("cand", c, off, kProjCand * nl, SCRATCH, 16); off = al(off + kProjCand * nl);
        L.add("claim", c, off, 4 * nl, SCRATCH, 4); off = al(off + 4 * nl);
    }
    L.back = off;
    for (int c = 0; c < count; ++c) {
        L.add("out", c, off, 4 * m1(s[c].a), BACK, 4); off = al(off + 4 * m1(s[c].a));
        L.add("cnt", c, off, 16, BACK, 4, true); off += 16;
    }
    L.bytes = al(off);
    return L;
}
static Layout now_last(const Shapes& s) {
    Layout L;
    const int count = (int)s.size();
    Arena A;
    L.add("table", -1, A.take(kLastProb * count), kLastProb * count, UP, 8);
    for (int c = 0; c < count; ++c) L.add("occ", c, A.take(m1(s[c].a)), m1(s[c].a), UP);
    A.end_upload();
    for (int c = 0; c < count; ++c) {
        const size_t nl = m1(s[c].b);
        L.add("rec", c, A.take(kLpRec * nl), kLpRec * nl, SCRATCH, 16);
        L.add("cand", c, A.take(kProjCand * nl), kProjCand * nl, SCRATCH, 16);
        L.add("claim", c, A.take(4 * nl), 4 * nl, SCRATCH, 4);
    }
    A.end_scratch();
    for (int c = 0; c < count; ++c) {
        L.add("out", c, A.take(4 * m1(s[c].a)), 4 * m1(s[c].a), BACK, 4);
        L.add("cnt", c, A.take_packed(16), 16, BACK, 4, true);
    }
    A.finish();
    L.up = A.up; L.back = A.back; L.bytes = A.bytes;
    return L;
}

static long g_bad = 0, g_layouts = 0, g_pieces = 0, g_after_packed = 0, g_literals = 0;

static void fail(const char* what, const char* layout, const Piece* p) {
    ++g_bad;
    if (p) std::fprintf(stderr, "%s: %s: piece %s[%d] at %zu + %zu\n", layout, what, p->name, p->c, p->off, p->size);
    else std::fprintf(stderr, "%s: %s\n", layout, what);
}

static void check(const char* name, const Layout& was, const Layout& now) {
    ++g_layouts;
    if (was.p.size() != now.p.size()) return fail("piece count", name, nullptr);
    if (was.up != now.up || was.back != now.back || was.bytes != now.bytes) fail("up / back / bytes", name, nullptr);
    for (size_t i = 0; i < now.p.size(); ++i)
        if (was.p[i].off != now.p[i].off || was.p[i].size != now.p[i].size) fail("offset differs", name, &now.p[i]);
    const Layout& L = now;
    if (!(L.up <= L.back && L.back <= L.bytes) || L.bytes % 256) fail("up <= back <= bytes", name, nullptr);
    // the order the pieces lie in the buffer (the fuse layout lists them row by row already)
    std::vector<const Piece*> by_off;
    for (const Piece& p : L.p) by_off.push_back(&p);
    std::stable_sort(by_off.begin(), by_off.end(), [](const Piece* x, const Piece* y) { return x->off < y->off; });
    for (size_t i = 0; i < by_off.size(); ++i) {
        const Piece& p = *by_off[i];
        ++g_pieces;
        const size_t lo = p.sec == UP ? 0 : p.sec == SCRATCH ? L.up : L.back;
        const size_t hi = p.sec == UP ? L.up : p.sec == SCRATCH ? L.back : L.bytes;
        if (p.off < lo || p.off + p.size > hi) fail("outside its section", name, &p);
        const size_t next = i + 1 < by_off.size() ? by_off[i + 1]->off : L.bytes;
        if (p.off + p.size > next) fail("runs into the next piece", name, &p);
        if (i && by_off[i - 1]->packed) {
            ++g_after_packed;
            const Piece& q = *by_off[i - 1];
            if (p.off != q.off + q.size || p.off % p.align) fail("after the count words", name, &p);
        } else if (p.off % 256) {
            fail("not on a 256-byte boundary", name, &p);
        }
    }
    // no two pieces overlap: a later memset would show in an earlier piece
    std::vector<unsigned char> block(L.bytes, 0xff);
    for (size_t i = 0; i < L.p.size(); ++i) std::memset(block.data() + L.p[i].off, (int)i, L.p[i].size);
    for (size_t i = 0; i < L.p.size(); ++i)
        for (size_t k = 0; k < L.p[i].size; ++k)
            if (block[L.p[i].off + k] != (unsigned char)i) {
                fail("overwritten by another piece", name, &L.p[i]);
                break;
            }
}

// offsets worked out by hand from the former loops, in piece order, then up, back, bytes
static void literal(const char* name, const Layout& L, const std::vector<size_t>& want) {
    ++g_literals;
    std::vector<size_t> got;
    for (const Piece& p : L.p) got.push_back(p.off);
    got.push_back(L.up);
    got.push_back(L.back);
    got.push_back(L.bytes);
    if (got != want) fail("hand-computed offsets", name, nullptr);
}

int main() {
    // sizes from {0, 1, 255, 256, 257}; every count-3 shape has a problem with n == 0
    const std::vector<Shapes> shapes = {
        {{0, 0}}, {{1, 255}}, {{256, 257}}, {{257, 0}}, {{255, 256}},
        {{0, 257}, {255, 1}, {256, 256}},
        {{257, 255}, {0, 0}, {1, 256}},
        {{256, 0}, {257, 257}, {0, 1}},
    };
    for (const Shapes& s : shapes) {
        check("search_by_sim3", was_sim3(s), now_sim3(s));
        check("search_by_projection", was_proj(s, kFrameProb, 4), now_proj(s, kFrameProb, 4));
        check("search_by_projection_kf", was_proj(s, kKfProb, 1), now_proj(s, kKfProb, 1));
        check("fuse_sim3", was_fuse(s), now_fuse(s));
        check("local_points matcher", was_local(s, false), now_local(s, false));
        check("local_points fused", was_local(s, true), now_local(s, true));
        check("search_by_projection_last", was_last(s), now_last(s));
    }
    // one pair, n1 = 1, n2 = 255: table | a1 a2 | m1 m2 | out nf
    literal("search_by_sim3 {1,255}", now_sim3({{1, 255}}), {0, 256, 512, 768, 1024, 2048, 2304, 768, 2048, 2560});
    // three problems (kf->n, frame->n) = (0, 257), (255, 1), (256, 256): the outputs of problems 1 and 2
    // start 8 bytes past a boundary, behind the count words of the problem before
    literal("search_by_projection {0,257},{255,1},{256,256}",
            now_proj({{0, 257}, {255, 1}, {256, 256}}, kFrameProb, 4),
            {0, 768, 1024, 2304, 2560, 2816, 3072,
             4096, 4352, 4608, 4864, 8960, 13056, 14080, 18176, 22272,
             23296, 24576, 24584, 24832, 24840, 26112,
             4096, 23296, 26368});
    std::printf("{\"layouts\": %ld, \"pieces\": %ld, \"after_packed\": %ld, \"literals\": %ld, \"mismatches\": %ld}\n",
                g_layouts, g_pieces, g_after_packed, g_literals, g_bad);
    return g_bad ? 1 : 0;
}
