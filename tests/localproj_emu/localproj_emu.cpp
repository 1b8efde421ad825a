// TEST-ONLY host build of the SearchLocalPoints device arithmetic (rsc_localproj.h): the per-point functions
// the kernels run, driven (a) by a literal sequential loop in the reference's order — also the one-core CPU
// baseline of tools/localproj_bench.py — and (b) by the fixed-point rounds exactly as localproj.hip runs
// them.  With -DLPE_MAIN the file is a stand-alone program that draws its own crowded problem and compares
// the two (run under the host sanitizers by tests/test_cpu_localproj.py).  The product library never
// contains this code path.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../orb-slam2-optimized_amd/csrc/rsc_localproj.h"
#include "../proj_emu_common.h"

using namespace rsc;

extern "C" {

struct lpe_problem {
    // Frame
    int32_t nf;
    const float* kp;
    const int32_t* octave;
    const uint8_t* desc;
    const int32_t* cell_begin;
    const int32_t* cell_feat;
    const float* scale;
    int32_t n_levels;
    float min_x, max_x, min_y, max_y, gw_inv, gh_inv, fx, fy, cx, cy, log_sf;
    const float* u_right;
    float mbf;
    // points
    int32_t np;
    const uint8_t* state;
    const float* pos;
    const float* normal;
    const float* dmax;
    const float* dmin;
    const uint8_t* pdesc;
    // call
    const float* Tcw;
    const uint8_t* skip;
    const uint8_t* has_obs;
    const uint8_t* frame_occ;
    const LpTrack* track_in;  // matcher-only mode
    float cos_limit, th, nn_ratio;
    int32_t fused;
};

}  // extern "C"

namespace {

struct Views : EmuFrame {
    DevKfpPoints P;
    std::vector<ProjDesc> pdesc;  // aligned copy
};

void make_views(const lpe_problem& p, Views& v) {
    make_frame_view(p, p.nf, nullptr, v);
    v.pdesc = emu_aligned_descs(p.pdesc, p.np);
    v.P = DevKfpPoints{p.state, p.pos, p.normal, p.dmax, p.dmin, v.pdesc.data(), p.np};
}

// what localproj_setup_kernel does for point i up to the window; *t = the record `track` shows afterwards
LpRec setup_point(const lpe_problem& p, const Views& v, int i, LpTrack* t) {
    LpTrack tr = lp_not_in_view();
    const bool eligible = lp_eligible(v.P, p.skip, i);
    if (p.fused) {
        if (eligible) tr = lp_frustum(v.F, p.mbf, v.P, p.Tcw, i, p.cos_limit);
        *t = tr;
    } else {
        *t = p.track_in[i];
        if (eligible) {
            tr = p.track_in[i];
            if ((unsigned)tr.level >= (unsigned)v.F.n_levels) tr.in_view = 0;
        }
    }
    return lp_window(v.F, tr, p.th);
}

// F.mvpMapPoints[f] = the last claimer; every claim counts
int finish(const lpe_problem& p, const std::vector<int>& claim, int32_t* out) {
    for (int f = 0; f < p.nf; ++f) out[f] = -1;
    int n = 0;
    for (int i = 0; i < p.np; ++i)
        if (claim[i] >= 0) {
            out[claim[i]] = i;
            ++n;
        }
    return n;
}

}  // namespace

extern "C" {

// Tracking.cpp:1003-1016 then the matcher's loop point by point in list order (ORBmatcher.cpp:22-97).
// counts = nmatches, nToMatch, 0.
void lpe_search_sequential(const lpe_problem* p, int32_t* out, LpTrack* track, int32_t* counts) {
    Views v;
    make_views(*p, v);
    std::vector<int> owner((size_t)p->nf + 1), claim((size_t)p->np + 1, -1);
    std::vector<LpRec> rec((size_t)p->np + 1);
    int n_to_match = 0;
    for (int i = 0; i < p->np; ++i) {
        rec[i] = setup_point(*p, v, i, &track[i]);
        n_to_match += rec[i].in_view;
    }
    for (int f = 0; f < p->nf; ++f) owner[f] = p->frame_occ[f] == 2 ? kProjOccupied : kProjFree;
    for (int i = 0; i < p->np; ++i) {
        const int b = lp_best(v.F, p->u_right, rec[i], v.P.desc[i], i, owner.data(), p->nn_ratio);
        claim[i] = b;
        if (b >= 0 && p->has_obs[i]) owner[b] = i;  // from here on the occupant of b has observations (:58-60)
    }
    counts[0] = finish(*p, claim, out);
    counts[1] = n_to_match;
    counts[2] = 0;
}

// The kernels' work (localproj.hip): lp_setup_point for every point, then the rounds.  counts = nmatches,
// nToMatch, rounds; walks[0] = window walks taken, walks[1] = the most of them in one round.
void lpe_search_fixed_point_walks(const lpe_problem* p, int32_t* out, LpTrack* track, int32_t* counts,
                                  int32_t* walks) {
    Views v;
    make_views(*p, v);
    std::vector<int> claim((size_t)p->np + 1);
    std::vector<LpRec> rec((size_t)p->np + 1);
    std::vector<ProjCand> cand((size_t)p->np + 1);
    LocalProjProblem Q{};
    Q.F = &v.F;
    Q.u_right = p->u_right;
    Q.mbf = p->mbf;
    Q.P = v.P;
    if (p->fused) std::memcpy(Q.Tcw, p->Tcw, 12 * sizeof(float));
    Q.skip = p->skip;
    Q.has_obs = p->has_obs;
    Q.frame_occ = p->frame_occ;
    Q.track = track;  // matcher-only mode reads the caller's records from there
    Q.rec = rec.data();
    Q.cand = cand.data();
    Q.claim = claim.data();
    if (!p->fused && p->np) std::memmove(track, p->track_in, sizeof(LpTrack) * (size_t)p->np);
    const int keep_max = lp_keep_max(p->nn_ratio);
    int n_eligible = 0, n_to_match = 0;
    for (int i = 0; i < p->np; ++i) {
        lp_setup_point(Q, i, p->fused, p->cos_limit, p->th, keep_max);
        n_to_match += rec[i].in_view;
        n_eligible += rec[i].cells >= 0;
    }
    counts[2] = emu_rounds(LpRounds{Q, p->nn_ratio}, p->nf, Q.claim, n_eligible, walks, walks + 1);
    counts[0] = finish(*p, claim, out);
    counts[1] = n_to_match;
}

// the same; *fallbacks (may be NULL) = window walks taken
void lpe_search_fixed_point(const lpe_problem* p, int32_t* out, LpTrack* track, int32_t* counts, int32_t* fallbacks) {
    int32_t walks[2];
    lpe_search_fixed_point_walks(p, out, track, counts, walks);
    if (fallbacks) *fallbacks = walks[0];
}

// the streaming update of ORBmatcher.cpp:73-85 over a sequence: res = bestDist, bestLevel, bestDist2,
// bestLevel2, bestIdx
void lpe_top2(int n, const int32_t* dist, const int32_t* level, int32_t* res) {
    LpTop2 t = lp_top2_init();
    for (int k = 0; k < n; ++k) lp_top2_push(t, dist[k], level[k], k);
    res[0] = t.bestDist;
    res[1] = t.bestLevel;
    res[2] = t.bestDist2;
    res[3] = t.bestLevel2;
    res[4] = t.bestIdx;
}

// :89-95 on given values: 1 = the match is written
int lpe_accepts(int best_dist, int best_level, int best_dist2, int best_level2, float nn_ratio) {
    LpTop2 t;
    t.bestDist = best_dist;
    t.bestLevel = best_level;
    t.bestDist2 = best_dist2;
    t.bestLevel2 = best_level2;
    t.bestIdx = 0;
    return lp_decide(t, nn_ratio) >= 0;
}

int lpe_veto_bound(float nn_ratio) { return lp_veto_bound(nn_ratio); }
int lpe_keep_max(float nn_ratio) { return lp_keep_max(nn_ratio); }
float lpe_radius(float view_cos) { return lp_radius(view_cos); }

}  // extern "C"

#ifdef LPE_MAIN
// A crowded problem drawn here: clusters of features a few pixels apart with near-identical descriptors and
// more points than features projecting onto each cluster; identity pose, points at z = 4; a third of the
// points without observations, a third of the features monocular, entry occupants of both kinds.
namespace {
uint32_t g_state = 12345u;
uint32_t rnd() {
    g_state = g_state * 1664525u + 1013904223u;
    return g_state >> 8;
}
float unif(float a, float b) { return a + (b - a) * (float)(rnd() & 0xffff) / 65536.0f; }
}  // namespace

int main() {
    const int clusters = 30, per_kp = 8, per_pt = 12, nf = clusters * per_kp + 200, np = clusters * per_pt + 400;
    const float W = 752.0f, H = 480.0f, fx = 435.0f, fy = 435.0f, cx = 367.0f, cy = 252.0f, mbf = 47.9f;
    std::vector<float> kp(2 * nf), pos(3 * np), normal(3 * np), dmax(np), dmin(np), scale(8), u_right(nf);
    std::vector<int32_t> octave(nf), out_seq(nf), out_fp(nf);
    std::vector<uint8_t> desc(32 * (size_t)nf), pdesc(32 * (size_t)np), state(np, 1), skip(np, 0), has_obs(np, 1),
        occ(nf, 0);
    std::vector<LpTrack> tr_seq(np), tr_fp(np), tr_mo(np);
    scale[0] = 1.0f;
    for (int l = 1; l < 8; ++l) scale[l] = scale[l - 1] * 1.2f;
    auto place = [&](int i, float u, float v, int level) {
        const float z = 4.0f;
        pos[3 * i] = (u - cx) / fx * z;
        pos[3 * i + 1] = (v - cy) / fy * z;
        pos[3 * i + 2] = z;
        const float d = sqrtf(pos[3 * i] * pos[3 * i] + pos[3 * i + 1] * pos[3 * i + 1] + z * z);
        for (int k = 0; k < 3; ++k) normal[3 * i + k] = pos[3 * i + k] / d;
        dmax[i] = d * powf(1.2f, (float)level - 0.5f);
        dmin[i] = dmax[i] / scale[7];
    };
    int k = 0, i = 0;
    for (int c = 0; c < clusters; ++c) {
        const float u = unif(40, W - 40), v = unif(40, H - 40);
        const int o = 1 + (int)(rnd() % 6);
        uint8_t base[32];
        for (int b = 0; b < 32; ++b) base[b] = (uint8_t)rnd();
        for (int m = 0; m < per_kp; ++m, ++k) {
            kp[2 * k] = u + unif(-4, 4);
            kp[2 * k + 1] = v + unif(-4, 4);
            octave[k] = o - (int)(rnd() % 3 == 0);
            std::memcpy(&desc[32 * (size_t)k], base, 32);
            for (int f = 0; f < 5; ++f) desc[32 * (size_t)k + rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
        }
        for (int m = 0; m < per_pt; ++m, ++i) {
            place(i, u, v, o);
            std::memcpy(&pdesc[32 * (size_t)i], base, 32);
            for (int f = 0; f < 3; ++f) pdesc[32 * (size_t)i + rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
        }
    }
    for (; k < nf; ++k) {
        kp[2 * k] = unif(2, W - 2);
        kp[2 * k + 1] = unif(2, H - 2);
        octave[k] = (int)(rnd() % 8);
        for (int b = 0; b < 32; ++b) desc[32 * (size_t)k + b] = (uint8_t)rnd();
    }
    for (; i < np; ++i) {
        const int src = (int)(rnd() % nf);
        place(i, kp[2 * src] + unif(-1, 1), kp[2 * src + 1] + unif(-1, 1), octave[src]);
        std::memcpy(&pdesc[32 * (size_t)i], &desc[32 * (size_t)src], 32);
        for (int f = 0; f < 8; ++f) pdesc[32 * (size_t)i + rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
        if (rnd() % 20 == 0) state[i] = 2;
        if (rnd() % 20 == 0) skip[i] = 1;
        if (rnd() % 20 == 0) pos[3 * i + 2] = rnd() % 2 ? -4.0f : 0.0f;  // behind the camera / z == 0
    }
    for (int j = 0; j < np; ++j) has_obs[j] = rnd() % 3 != 0;
    for (int f = 0; f < nf; ++f) {
        occ[f] = rnd() % 10 == 0 ? 1 + (rnd() % 2) : 0;
        u_right[f] = rnd() % 3 == 0 ? -1.0f : kp[2 * f] - mbf / 4.0f + unif(-6, 6);
    }
    // mGrid as CSR with PosInGrid's rounding
    const float gw = 64.0f / W, gh = 48.0f / H;
    std::vector<int32_t> begin(64 * 48 + 1, 0), feat(nf), cell(nf);
    for (int f = 0; f < nf; ++f) {
        int px = (int)floorf(kp[2 * f] * gw + 0.5f), py = (int)floorf(kp[2 * f + 1] * gh + 0.5f);
        if (px > 63) px = 63;
        if (py > 47) py = 47;
        cell[f] = px * 48 + py;
        ++begin[cell[f] + 1];
    }
    for (int c = 0; c < 64 * 48; ++c) begin[c + 1] += begin[c];
    std::vector<int32_t> fill(begin.begin(), begin.end() - 1);
    for (int f = 0; f < nf; ++f) feat[fill[cell[f]]++] = f;
    const float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    lpe_problem p{nf, kp.data(), octave.data(), desc.data(), begin.data(), feat.data(), scale.data(), 8,
                  0.0f, W, 0.0f, H, gw, gh, fx, fy, cx, cy, logf(1.2f), u_right.data(), mbf,
                  np, state.data(), pos.data(), normal.data(), dmax.data(), dmin.data(), pdesc.data(),
                  T, skip.data(), has_obs.data(), occ.data(), nullptr, 0.5f, 5.0f, 0.8f, 1};
    int mismatches = 0, nmatches = 0, rounds = 0, walks_total = 0;
    for (int pass = 0; pass < 2; ++pass) {  // th = 5, then th = 1
        int32_t c_seq[3], c_fp[3], c_mo[3], walks = 0;
        lpe_search_sequential(&p, out_seq.data(), tr_seq.data(), c_seq);
        lpe_search_fixed_point(&p, out_fp.data(), tr_fp.data(), c_fp, &walks);
        mismatches += c_seq[0] != c_fp[0] || c_seq[1] != c_fp[1];
        for (int f = 0; f < nf; ++f) mismatches += out_seq[f] != out_fp[f];
        mismatches += std::memcmp(tr_seq.data(), tr_fp.data(), sizeof(LpTrack) * (size_t)np) != 0;
        // matcher-only mode on the records of the fused run
        lpe_problem q = p;
        q.fused = 0;
        q.track_in = tr_seq.data();
        lpe_search_fixed_point(&q, out_fp.data(), tr_mo.data(), c_mo, nullptr);
        mismatches += c_mo[0] != c_seq[0] || c_mo[2] != c_fp[2];
        for (int f = 0; f < nf; ++f) mismatches += out_seq[f] != out_fp[f];
        nmatches += c_seq[0];
        rounds += c_fp[2];
        walks_total += walks;
        p.th = 1.0f;
    }
    std::printf("{\"mismatches\": %d, \"nmatches\": %d, \"rounds\": %d, \"fallback_walks\": %d}\n", mismatches,
                nmatches, rounds, walks_total);
    return mismatches ? 1 : 0;
}
#endif
