// TEST-ONLY host build of the last-frame SearchByProjection device arithmetic (rsc_lastproj.h): the per-point
// functions the kernels run, driven (a) by a literal sequential loop in the reference's order on an explicit
// mvpMapPoints with the rotation histogram as lists of entries — also the one-core CPU baseline of
// tools/lastproj_bench.py — and (b) by the fixed-point rounds and the table-based finish exactly as
// lastproj.hip runs them.  With -DLSE_MAIN the file is a stand-alone program that draws its own crowded
// problems, one per level mode, and compares the two (run under the host sanitizers by
// tests/test_cpu_lastproj.py).  The product library never contains this code path.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../orb-slam2-optimized_amd/csrc/rsc_lastproj.h"
#include "../proj_emu_common.h"

using namespace rsc;

extern "C" {

struct lse_problem {
    // current Frame
    int32_t nf;
    const float* kp;
    const int32_t* octave;
    const float* angle;
    const uint8_t* desc;
    const int32_t* cell_begin;
    const int32_t* cell_feat;
    const float* scale;
    int32_t n_levels;
    float min_x, max_x, min_y, max_y, gw_inv, gh_inv, fx, fy, cx, cy, log_sf;
    const float* u_right;
    float mbf;
    // last Frame
    int32_t nl;
    const int32_t* l_octave;
    const float* l_angle;
    const uint8_t* mp_state;
    const float* mp_pos;
    const uint8_t* mp_desc;
    const uint8_t* mp_has_obs;
    // call
    const float* Tcw_cur;
    const float* Tcw_last;
    float mb;
    const uint8_t* frame_occ;
    float th;
    int32_t check_ori;
};

}  // extern "C"

namespace {

struct Views : EmuFrame {
    DevLastFrame L;
    std::vector<ProjDesc> ldesc;  // aligned copy
};

void make_views(const lse_problem& p, Views& v) {
    make_frame_view(p, p.nf, p.angle, v);
    v.ldesc = emu_aligned_descs(p.mp_desc, p.nl);
    v.L = DevLastFrame{p.l_octave, p.l_angle, p.mp_state, p.mp_pos, v.ldesc.data(), p.mp_has_obs, p.nl};
}

}  // namespace

extern "C" {

int lse_mode(const float* Tc, const float* Tl, float mb) { return last_mode(Tc, Tl, mb); }

// ORBmatcher.cpp:1196-1312 slot by slot.  mp[f]: -1 NULL, -2 the entry occupant, >= 0 the LastFrame slot
// held.  counts = nmatches, mode, 0, claims.
void lse_search_sequential(const lse_problem* p, int32_t* out, int32_t* counts) {
    Views v;
    make_views(*p, v);
    const int mode = last_mode(p->Tcw_cur, p->Tcw_last, p->mb);
    std::vector<int> owner((size_t)p->nf + 1), mp((size_t)p->nf + 1, -1);
    std::vector<uint8_t> touched((size_t)p->nf + 1, 0);
    std::vector<std::vector<int>> rotHist(kProjHistoLength);
    for (int f = 0; f < p->nf; ++f) {
        owner[f] = p->frame_occ[f] == 2 ? kProjOccupied : kProjFree;
        mp[f] = p->frame_occ[f] ? -2 : -1;
    }
    int nmatches = 0, claims = 0;
    for (int i = 0; i < p->nl; ++i) {
        const LpRec q = last_eligible(v.L, i) ? last_setup(v.F, p->mbf, v.L, p->Tcw_cur, i, p->th) : lp_no_window();
        const int b = last_best(v.F, p->u_right, q, v.L.mp_desc[i], i, owner.data(), mode);
        if (b < 0) continue;
        mp[b] = i;                                                       // :1273
        touched[b] = 1;
        owner[b] = p->mp_has_obs[i] ? i : kProjFree;                     // the new occupant decides (:1248-1250)
        ++nmatches;                                                      // :1274
        ++claims;
        if (p->check_ori) {
            const int bin = proj_rot_bin(v.L.angle[i], v.F.angle[b]);    // :1278-1283
            if ((unsigned)bin < (unsigned)kProjHistoLength) rotHist[bin].push_back(b);  // :1285
        }
    }
    if (p->check_ori) {
        int hs[kProjHistoLength], keep[3];
        for (int b = 0; b < kProjHistoLength; ++b) hs[b] = (int)rotHist[b].size();
        last_keep_bins(hs, keep);                                        // :1299
        for (int b = 0; b < kProjHistoLength; ++b) {                     // :1301-1311
            if (b == keep[0] || b == keep[1] || b == keep[2]) continue;
            for (int f : rotHist[b]) {
                mp[f] = -1;                                              // :1307
                --nmatches;                                              // :1308
            }
        }
    }
    for (int f = 0; f < p->nf; ++f) out[f] = !touched[f] ? -1 : (mp[f] >= 0 ? mp[f] : kLastNulled);
    counts[0] = nmatches;
    counts[1] = mode;
    counts[2] = 0;
    counts[3] = claims;
}

// The kernels' work (lastproj.hip): last_setup_slot for every slot, then the rounds, then the histogram over
// all claims, the last-writer table and the nulling.  counts = nmatches, mode, rounds, claims; walks[0] =
// window walks taken, walks[1] = the most of them in one round.
void lse_search_fixed_point_walks(const lse_problem* p, int32_t* out, int32_t* counts, int32_t* walks) {
    Views v;
    make_views(*p, v);
    const int mode = last_mode(p->Tcw_cur, p->Tcw_last, p->mb);
    std::vector<int> claim((size_t)p->nl + 1);
    std::vector<LpRec> rec((size_t)p->nl + 1);
    std::vector<ProjCand> cand((size_t)p->nl + 1);
    LastProjProblem Q{};
    Q.F = &v.F;
    Q.u_right = p->u_right;
    Q.mbf = p->mbf;
    Q.mode = mode;
    Q.L = v.L;
    std::memcpy(Q.Tcw, p->Tcw_cur, 12 * sizeof(float));
    Q.frame_occ = p->frame_occ;
    Q.rec = rec.data();
    Q.cand = cand.data();
    Q.claim = claim.data();
    int n_eligible = 0;
    for (int i = 0; i < p->nl; ++i) {
        last_setup_slot(Q, i, p->th);
        n_eligible += rec[i].cells >= 0;
    }
    const int done = emu_rounds(LastRounds{Q, mode}, p->nf, Q.claim, n_eligible, walks, walks + 1);
    int hs[kProjHistoLength] = {}, keep[3] = {-1, -1, -1};
    if (p->check_ori) {
        for (int i = 0; i < p->nl; ++i) {
            if (claim[i] < 0) continue;
            const int bin = proj_rot_bin(v.L.angle[i], v.F.angle[claim[i]]);
            if ((unsigned)bin < (unsigned)kProjHistoLength) ++hs[bin];
        }
        last_keep_bins(hs, keep);
    }
    for (int f = 0; f < p->nf; ++f) out[f] = -1;
    int total = 0, kept = 0;
    for (int i = 0; i < p->nl; ++i)
        if (claim[i] >= 0) {
            if (i > out[claim[i]]) out[claim[i]] = i;  // atomicMax
            ++total;
        }
    for (int i = 0; i < p->nl; ++i) {
        if (claim[i] < 0) continue;
        if (p->check_ori) {
            const int bin = proj_rot_bin(v.L.angle[i], v.F.angle[claim[i]]);
            if (bin != keep[0] && bin != keep[1] && bin != keep[2]) {
                out[claim[i]] = kLastNulled;
                continue;
            }
        }
        ++kept;
    }
    counts[0] = kept;
    counts[1] = mode;
    counts[2] = done;
    counts[3] = total;
}

// the same; *fallbacks (may be NULL) = window walks taken
void lse_search_fixed_point(const lse_problem* p, int32_t* out, int32_t* counts, int32_t* fallbacks) {
    int32_t walks[2];
    lse_search_fixed_point_walks(p, out, counts, walks);
    if (fallbacks) *fallbacks = walks[0];
}

}  // extern "C"

#ifdef LSE_MAIN
// Crowded problems drawn here: clusters of features a few pixels apart with near-identical descriptors and
// more LastFrame slots than features projecting onto each cluster; identity current pose, points at z = 4; a
// third of the slots without observations, some outliers and empty slots, a third of the features monocular,
// entry occupants of both kinds.  One pass per level mode (the last pose's translation against mb).
namespace {
uint32_t g_state = 12345u;
uint32_t rnd() {
    g_state = g_state * 1664525u + 1013904223u;
    return g_state >> 8;
}
float unif(float a, float b) { return a + (b - a) * (float)(rnd() & 0xffff) / 65536.0f; }
}  // namespace

int main() {
    const int clusters = 30, per_kp = 8, per_pt = 12, nf = clusters * per_kp + 200, nl = clusters * per_pt + 400;
    const float W = 752.0f, H = 480.0f, fx = 435.0f, fy = 435.0f, cx = 367.0f, cy = 252.0f, mbf = 47.9f;
    std::vector<float> kp(2 * nf), angle(nf), pos(3 * nl), l_angle(nl), scale(8), u_right(nf);
    std::vector<int32_t> octave(nf), l_octave(nl), out_seq(nf), out_fp(nf);
    std::vector<uint8_t> desc(32 * (size_t)nf), pdesc(32 * (size_t)nl), state(nl, 1), has_obs(nl, 1), occ(nf, 0);
    scale[0] = 1.0f;
    for (int l = 1; l < 8; ++l) scale[l] = scale[l - 1] * 1.2f;
    auto place = [&](int i, float u, float v) {
        const float z = 4.0f;
        pos[3 * i] = (u - cx) / fx * z;
        pos[3 * i + 1] = (v - cy) / fy * z;
        pos[3 * i + 2] = z;
    };
    int k = 0, i = 0;
    for (int c = 0; c < clusters; ++c) {
        const float u = unif(40, W - 40), v = unif(40, H - 40), a = unif(0, 360);
        const int o = 1 + (int)(rnd() % 6);
        uint8_t base[32];
        for (int b = 0; b < 32; ++b) base[b] = (uint8_t)rnd();
        for (int m = 0; m < per_kp; ++m, ++k) {
            kp[2 * k] = u + unif(-4, 4);
            kp[2 * k + 1] = v + unif(-4, 4);
            octave[k] = o - 1 + (int)(rnd() % 3);
            angle[k] = a + unif(-10, 10);
            if (angle[k] < 0) angle[k] += 360.0f;
            if (angle[k] >= 360.0f) angle[k] -= 360.0f;
            std::memcpy(&desc[32 * (size_t)k], base, 32);
            for (int f = 0; f < 5; ++f) desc[32 * (size_t)k + rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
        }
        for (int m = 0; m < per_pt; ++m, ++i) {
            place(i, u, v);
            l_octave[i] = o;
            l_angle[i] = rnd() % 6 == 0 ? unif(0, 360) : a;
            std::memcpy(&pdesc[32 * (size_t)i], base, 32);
            for (int f = 0; f < 3; ++f) pdesc[32 * (size_t)i + rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
        }
    }
    for (; k < nf; ++k) {
        kp[2 * k] = unif(2, W - 2);
        kp[2 * k + 1] = unif(2, H - 2);
        octave[k] = (int)(rnd() % 8);
        angle[k] = unif(0, 360);
        for (int b = 0; b < 32; ++b) desc[32 * (size_t)k + b] = (uint8_t)rnd();
    }
    for (; i < nl; ++i) {
        const int src = (int)(rnd() % nf);
        place(i, kp[2 * src] + unif(-1, 1), kp[2 * src + 1] + unif(-1, 1));
        l_octave[i] = octave[src];
        l_angle[i] = angle[src];
        std::memcpy(&pdesc[32 * (size_t)i], &desc[32 * (size_t)src], 32);
        for (int f = 0; f < 8; ++f) pdesc[32 * (size_t)i + rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
        if (rnd() % 20 == 0) state[i] = 2;
        if (rnd() % 20 == 0) state[i] = 0;
        if (rnd() % 20 == 0) pos[3 * i + 2] = rnd() % 2 ? -4.0f : 0.0f;  // behind the camera / z == 0
    }
    for (int j = 0; j < nl; ++j) has_obs[j] = rnd() % 3 != 0;
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
    float Tl[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    lse_problem p{nf, kp.data(), octave.data(), angle.data(), desc.data(), begin.data(), feat.data(), scale.data(), 8,
                  0.0f, W, 0.0f, H, gw, gh, fx, fy, cx, cy, logf(1.2f), u_right.data(), mbf,
                  nl, l_octave.data(), l_angle.data(), state.data(), pos.data(), pdesc.data(), has_obs.data(),
                  T, Tl, 0.11f, occ.data(), 7.0f, 1};
    const float tz[3] = {0.0f, 0.5f, -0.5f};  // window, forward, backward
    int mismatches = 0, nmatches = 0, rounds = 0, walks_total = 0, nulled = 0;
    for (int pass = 0; pass < 6; ++pass) {  // each mode at th = 7 and th = 15
        Tl[11] = tz[pass % 3];
        p.th = pass < 3 ? 7.0f : 15.0f;
        int32_t c_seq[4], c_fp[4], walks = 0;
        lse_search_sequential(&p, out_seq.data(), c_seq);
        lse_search_fixed_point(&p, out_fp.data(), c_fp, &walks);
        mismatches += c_seq[0] != c_fp[0] || c_seq[1] != c_fp[1] || c_seq[3] != c_fp[3] || c_seq[1] != pass % 3;
        for (int f = 0; f < nf; ++f) {
            mismatches += out_seq[f] != out_fp[f];
            nulled += out_seq[f] == kLastNulled;
        }
        nmatches += c_seq[0];
        rounds += c_fp[2];
        walks_total += walks;
    }
    std::printf("{\"mismatches\": %d, \"nmatches\": %d, \"rounds\": %d, \"fallback_walks\": %d, \"nulled\": %d}\n",
                mismatches, nmatches, rounds, walks_total, nulled);
    return mismatches ? 1 : 0;
}
#endif
