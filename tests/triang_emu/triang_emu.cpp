// TEST-ONLY host emulation of triang.hip: the per-candidate and per-pair functions of rsc_triang.h driven (a) by a
// literal sequential loop with the reference's running bestDist (ORBmatcher.cpp:489-669) and (b) by the kernels'
// own order: items per class, a group of G lanes striding the KeyFrame-2 node, the packed-key minimum.
// Built as a ctypes library and, with -DTSE_MAIN, as a stand-alone program that runs a file of dumped cases
// through both forms (tests/triang_emu_lib.py writes the file and reads the results).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "rsc_triang.h"

using namespace rsc;

extern "C" {

struct tse_kf {
    int32_t n;
    const float* kp;
    const float* kp_raw;
    const int32_t* octave;
    const uint8_t* desc;
    const float* angle;
    const float* u_right;
    const float* depth;
    const float* cos_stereo;
    const uint8_t* mp_state;
    int32_t n_nodes;
    const uint32_t* node_id;
    const int32_t* node_begin;
    const uint32_t* feat;
    const float* scale;
    int32_t n_levels;
    float Rcw[9], tcw[3], Rwc[9], Ow[3];
    float fx, fy, cx, cy, invfx, invfy, mb, mbf, scale_factor;
    float Kinv[9];
};

static TriView view_of(const tse_kf& k) {
    TriView v;
    v.kp = k.kp; v.kp_raw = k.kp_raw; v.octave = k.octave; v.scale = k.scale;
    v.u_right = k.u_right; v.depth = k.depth; v.cos_stereo = k.cos_stereo;
    std::memcpy(v.Rcw, k.Rcw, sizeof(v.Rcw)); std::memcpy(v.tcw, k.tcw, sizeof(v.tcw));
    std::memcpy(v.Rwc, k.Rwc, sizeof(v.Rwc)); std::memcpy(v.Ow, k.Ow, sizeof(v.Ow));
    v.fx = k.fx; v.fy = k.fy; v.cx = k.cx; v.cy = k.cy; v.invfx = k.invfx; v.invfy = k.invfy;
    v.mb = k.mb; v.mbf = k.mbf; v.scale_factor = k.scale_factor; v.n = k.n; v.n_levels = k.n_levels;
    return v;
}

static int dist256(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int i = 0; i < 32; ++i) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

static int find_node(const tse_kf& k, uint32_t id) {
    int lo = 0, hi = k.n_nodes;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (k.node_id[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return (lo < k.n_nodes && k.node_id[lo] == id) ? lo : -1;
}

static void finish(const tse_kf& k1, const tse_kf& k2, int check_ori, int den_zero, int32_t* m12, int32_t* counts) {
    counts[1] = den_zero;
    if (den_zero) {
        for (int i = 0; i < k1.n; ++i) m12[i] = -1;
        counts[0] = 0;
        return;
    }
    if (check_ori) {
        int hist[30] = {0};
        for (int i = 0; i < k1.n; ++i)
            if (m12[i] >= 0) {
                const int bin = tri_rot_bin(k1.angle[i], k2.angle[m12[i]]);
                if ((unsigned)bin < 30u) hist[bin]++;  // as the kernel: finite angles give 0..12
            }
        const TriMaxima mx = tri_three_maxima([&](int i) { return hist[i]; });
        for (int i = 0; i < k1.n; ++i)
            if (m12[i] >= 0) {
                const int bin = tri_rot_bin(k1.angle[i], k2.angle[m12[i]]);
                if (bin != mx.ind1 && bin != mx.ind2 && bin != mx.ind3) m12[i] = -1;
            }
    }
    int cnt = 0;
    for (int i = 0; i < k1.n; ++i) cnt += m12[i] >= 0;
    counts[0] = cnt;
}

static bool flag(const uint8_t* given, const tse_kf& k, int i) { return given ? given[i] != 0 : k.mp_state[i] != 0; }

// (a) the literal loop: nodes in ascending id, slots and candidates in vector order, the running bestDist, the
// return at the first den == 0.  counts: nmatches, den_zero.  dzs: the slot that ended the call.
void tse_search_sequential(const tse_kf* k1p, const tse_kf* k2p, const float* F, int only_stereo, int check_ori,
                           const uint8_t* has1, const uint8_t* has2, int32_t* m12, int32_t* counts, uint8_t* dzs) {
    const tse_kf& k1 = *k1p;
    const tse_kf& k2 = *k2p;
    float ex, ey;
    tri_epipole(k2.Rcw, k2.tcw, k1.Ow, k2.fx, k2.fy, k2.cx, k2.cy, ex, ey);
    for (int i = 0; i < k1.n; ++i) { m12[i] = -1; dzs[i] = 0; }
    for (int a = 0; a < k1.n_nodes; ++a) {
        const int b = find_node(k2, k1.node_id[a]);
        if (b < 0) continue;
        for (int e1 = k1.node_begin[a]; e1 < k1.node_begin[a + 1]; ++e1) {
            const int idx1 = (int)k1.feat[e1];
            if (flag(has1, k1, idx1)) continue;
            const bool st1 = k1.u_right[idx1] >= 0;
            if (only_stereo && !st1) continue;
            float la, lb, lc, den;
            tri_epiline(F, k1.kp[2 * idx1], k1.kp[2 * idx1 + 1], la, lb, lc, den);
            if (den == 0) {
                dzs[idx1] = 1;
                finish(k1, k2, check_ori, 1, m12, counts);
                return;
            }
            int bestDist = kTriThLow, best = -1;
            for (int e2 = k2.node_begin[b]; e2 < k2.node_begin[b + 1]; ++e2) {
                const int idx2 = (int)k2.feat[e2];
                if (flag(has2, k2, idx2)) continue;
                const bool st2 = k2.u_right[idx2] >= 0;
                if (only_stereo && !st2) continue;
                const int dist = dist256(k1.desc + 32 * idx1, k2.desc + 32 * idx2);
                if (dist > kTriThLow || dist > bestDist) continue;
                if (tri_candidate_ok(la, lb, lc, den, ex, ey, st1, st2, k2.kp[2 * idx2], k2.kp[2 * idx2 + 1],
                                     k2.scale[k2.octave[idx2]])) {
                    best = idx2;
                    bestDist = dist;
                }
            }
            if (best >= 0) m12[idx1] = best;
        }
    }
    finish(k1, k2, check_ori, 0, m12, counts);
}

// (b) the kernels' order: the join's items by class, G lanes per item, each lane's strided minimum, the butterfly.
// dzs: every eligible slot with den == 0 (what the device reports).
void tse_search_kernel_order(const tse_kf* k1p, const tse_kf* k2p, const float* F, int only_stereo, int check_ori,
                             const uint8_t* has1, const uint8_t* has2, int32_t* m12, int32_t* counts, uint8_t* dzs) {
    const tse_kf& k1 = *k1p;
    const tse_kf& k2 = *k2p;
    float ex, ey;
    tri_epipole(k2.Rcw, k2.tcw, k1.Ow, k2.fx, k2.fy, k2.cx, k2.cy, ex, ey);
    for (int i = 0; i < k1.n; ++i) { m12[i] = -1; dzs[i] = 0; }
    struct Item { int e1, b0, nb; };
    std::vector<Item> items[kTriClasses];
    for (int a = 0; a < k1.n_nodes; ++a) {
        const int b = find_node(k2, k1.node_id[a]);
        if (b < 0) continue;
        const int b0 = k2.node_begin[b], nb = k2.node_begin[b + 1] - b0;
        for (int e1 = k1.node_begin[a]; e1 < k1.node_begin[a + 1]; ++e1) {
            const int idx1 = (int)k1.feat[e1];
            if (flag(has1, k1, idx1) || (only_stereo && !(k1.u_right[idx1] >= 0))) continue;
            items[tri_class_of(nb)].push_back({e1, b0, nb});
        }
    }
    int den_zero = 0;
    for (int cls = 0; cls < kTriClasses; ++cls) {
        const int G = tri_class_width(cls);
        for (const Item& it : items[cls]) {
            const int idx1 = (int)k1.feat[it.e1];
            const bool st1 = k1.u_right[idx1] >= 0;
            float la, lb, lc, den;
            tri_epiline(F, k1.kp[2 * idx1], k1.kp[2 * idx1 + 1], la, lb, lc, den);
            if (den == 0) {
                dzs[idx1] = 1;
                den_zero = 1;
                continue;
            }
            std::vector<uint32_t> key((size_t)G, kTriNoKey);
            for (int gl = 0; gl < G; ++gl)
                for (int q = gl; q < it.nb; q += G) {
                    const int idx2 = (int)k2.feat[it.b0 + q];
                    if (flag(has2, k2, idx2)) continue;
                    const bool st2 = k2.u_right[idx2] >= 0;
                    if (only_stereo && !st2) continue;
                    const uint32_t dist = (uint32_t)dist256(k1.desc + 32 * idx1, k2.desc + 32 * idx2);
                    if (dist > (uint32_t)kTriThLow) continue;
                    if (tri_candidate_ok(la, lb, lc, den, ex, ey, st1, st2, k2.kp[2 * idx2], k2.kp[2 * idx2 + 1],
                                         k2.scale[k2.octave[idx2]])) {
                        const uint32_t k = tri_key(dist, (uint32_t)q);
                        if (k < key[gl]) key[gl] = k;
                    }
                }
            for (int off = G / 2; off >= 1; off >>= 1) {
                std::vector<uint32_t> nk(key);
                for (int gl = 0; gl < G; ++gl) nk[gl] = key[gl] < key[gl ^ off] ? key[gl] : key[gl ^ off];
                key.swap(nk);
            }
            if (key[0] != kTriNoKey) m12[idx1] = (int32_t)k2.feat[it.b0 + (int)tri_key_pos(key[0])];
        }
    }
    finish(k1, k2, check_ori, den_zero, m12, counts);
}

void tse_triangulate(const tse_kf* k1, const tse_kf* k2, int npairs, const int32_t* pairs, int32_t* status, float* x3d) {
    const TriView v1 = view_of(*k1), v2 = view_of(*k2);
    for (int i = 0; i < npairs; ++i) {
        float x[3];
        status[i] = tri_pair(v1, v2, pairs[2 * i], pairs[2 * i + 1], x);
        std::memcpy(x3d + 3 * i, x, sizeof(x));
    }
}

void tse_compute_f12(const tse_kf* k1, const tse_kf* k2, float* F) {
    tri_compute_f12(k1->Rcw, k1->tcw, k2->Rwc, k2->Ow, k1->Kinv, k2->Kinv, F);
}

int tse_baseline_short(const tse_kf* k1, const tse_kf* k2) { return tri_baseline_short(k1->Ow, k2->Ow, k2->mb) ? 1 : 0; }

void tse_svd_last_v(const float* A, float* v) {
    float M[4][4], o[4];
    std::memcpy(M, A, sizeof(M));
    tri_svd_last_v(M, o);
    std::memcpy(v, o, sizeof(o));
}

// The literal neighbour loop of LocalMapping.cpp:224-428 over the sequential matcher: slots filled as it goes.
void tse_create_new_map_points(const tse_kf* cur, const tse_kf* const* neigh, int nn, int32_t* new_neighbour,
                               int32_t* new_idx2, float* new_pos, int32_t* nnew) {
    const int n = cur->n;
    std::vector<uint8_t> filled((size_t)n + 1), dzs((size_t)n + 1);
    std::vector<int32_t> m12((size_t)n + 1);
    for (int i = 0; i < n; ++i) {
        filled[i] = cur->mp_state[i] != 0;
        new_neighbour[i] = new_idx2[i] = -1;
        new_pos[3 * i] = new_pos[3 * i + 1] = new_pos[3 * i + 2] = 0.0f;
    }
    *nnew = 0;
    const TriView v1 = view_of(*cur);
    for (int j = 0; j < nn; ++j) {
        if (tse_baseline_short(cur, neigh[j])) continue;
        float F[9];
        tse_compute_f12(cur, neigh[j], F);
        int32_t counts[2];
        tse_search_sequential(cur, neigh[j], F, 0, 0, filled.data(), nullptr, m12.data(), counts, dzs.data());
        const TriView v2 = view_of(*neigh[j]);
        for (int i = 0; i < n; ++i) {
            if (m12[i] < 0) continue;
            float x[3];
            if (tri_pair(v1, v2, i, m12[i], x) != kTriOk) continue;
            new_neighbour[i] = j;
            new_idx2[i] = m12[i];
            std::memcpy(new_pos + 3 * i, x, sizeof(x));
            filled[i] = 1;
            ++*nnew;
        }
    }
}

}  // extern "C"

#ifdef TSE_MAIN
// Reads the case file of tests/triang_emu_lib.py (dump): int32 words and raw arrays, runs every matcher problem
// through both forms and every pair list through the geometry, and writes the results back for the test to compare.
namespace {
struct Reader {
    std::vector<char> buf;
    size_t off = 0;
    template <class T> const T* take(size_t n) {
        const size_t bytes = (n * sizeof(T) + 7) & ~(size_t)7;
        if (off + bytes > buf.size()) { std::fprintf(stderr, "case file truncated\n"); std::exit(2); }
        const T* p = reinterpret_cast<const T*>(buf.data() + off);
        off += bytes;
        return p;
    }
    int32_t word() { return *take<int32_t>(1); }
};

tse_kf read_kf(Reader& r) {
    tse_kf k;
    k.n = r.word();
    k.n_nodes = r.word();
    k.n_levels = r.word();
    const int nf = r.word();
    const size_t n = (size_t)k.n;
    k.kp = r.take<float>(2 * n); k.kp_raw = r.take<float>(2 * n); k.octave = r.take<int32_t>(n);
    k.desc = r.take<uint8_t>(32 * n); k.angle = r.take<float>(n); k.u_right = r.take<float>(n);
    k.depth = r.take<float>(n); k.cos_stereo = r.take<float>(n); k.mp_state = r.take<uint8_t>(n);
    k.node_id = r.take<uint32_t>((size_t)k.n_nodes); k.node_begin = r.take<int32_t>((size_t)k.n_nodes + 1);
    k.feat = r.take<uint32_t>((size_t)nf); k.scale = r.take<float>((size_t)k.n_levels);
    const float* s = r.take<float>(42);
    std::memcpy(k.Rcw, s, 36); std::memcpy(k.tcw, s + 9, 12); std::memcpy(k.Rwc, s + 12, 36); std::memcpy(k.Ow, s + 21, 12);
    k.fx = s[24]; k.fy = s[25]; k.cx = s[26]; k.cy = s[27]; k.invfx = s[28]; k.invfy = s[29]; k.mb = s[30];
    k.mbf = s[31]; k.scale_factor = s[32];
    std::memcpy(k.Kinv, s + 33, 36);
    return k;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
    Reader r;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    r.buf.resize((size_t)std::ftell(f));
    std::fseek(f, 0, SEEK_SET);
    if (std::fread(r.buf.data(), 1, r.buf.size(), f) != r.buf.size()) return 2;
    std::fclose(f);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const int ncases = r.word();
    for (int c = 0; c < ncases; ++c) {
        const tse_kf k1 = read_kf(r), k2 = read_kf(r);
        const float* F = r.take<float>(9);
        const int only_stereo = r.word(), check_ori = r.word(), npairs = r.word();
        const int32_t* pairs = r.take<int32_t>(2 * (size_t)npairs);
        const size_t n = (size_t)k1.n + 1;
        std::vector<int32_t> ma(n), mb(n), st((size_t)npairs + 1);
        std::vector<uint8_t> da(n), db(n);
        std::vector<float> x(3 * ((size_t)npairs + 1));
        int32_t ca[2], cb[2];
        tse_search_sequential(&k1, &k2, F, only_stereo, check_ori, nullptr, nullptr, ma.data(), ca, da.data());
        tse_search_kernel_order(&k1, &k2, F, only_stereo, check_ori, nullptr, nullptr, mb.data(), cb, db.data());
        tse_triangulate(&k1, &k2, npairs, pairs, st.data(), x.data());
        std::fwrite(ca, 4, 2, o); std::fwrite(ma.data(), 4, (size_t)k1.n, o);
        std::fwrite(cb, 4, 2, o); std::fwrite(mb.data(), 4, (size_t)k1.n, o);
        std::fwrite(st.data(), 4, (size_t)npairs, o); std::fwrite(x.data(), 4, 3 * (size_t)npairs, o);
    }
    std::fclose(o);
    std::printf("%d cases\n", ncases);
    return 0;
}
#endif
