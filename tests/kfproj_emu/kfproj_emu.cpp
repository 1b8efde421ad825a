// TEST-ONLY host build of the loop-closing matchers' device arithmetic (rsc_kfproj.h) and of the Sim3
// composition (rsc_sim3compose.h): the per-point functions the kernels run, driven (a) by a literal
// sequential loop in the reference's order — also the one-core CPU baseline of tools/kfproj_bench.py —
// and (b) by the fixed-point rounds exactly as kfproj.hip runs them.  With -DKFPE_MAIN the file is a
// stand-alone program that draws its own crowded problem and compares the two (run under the host
// sanitizers by tests/test_cpu_kfproj.py).  The product library never contains this code path.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../orb-slam2-optimized_amd/csrc/rsc_kfproj.h"
#include "../../orb-slam2-optimized_amd/csrc/rsc_sim3compose.h"
#include "../proj_emu_common.h"

using namespace rsc;

extern "C" {

struct kfpe_problem {
    // KeyFrame
    int32_t nk;
    const float* kp;
    const int32_t* octave;
    const uint8_t* desc;
    const int32_t* cell_begin;
    const int32_t* cell_feat;
    const float* scale;
    int32_t n_levels;
    float min_x, max_x, min_y, max_y, gw_inv, gh_inv, fx, fy, cx, cy, log_sf;
    // points
    int32_t np;
    const uint8_t* state;
    const float* pos;
    const float* normal;
    const float* dmax;
    const float* dmin;
    const uint8_t* pdesc;
    // call
    const float* Scw;
    const uint8_t* skip;      // already (SearchByProjection) or in_kf (Fuse)
    const uint8_t* occupied;  // [nk], SearchByProjection only
    float th;
};

}  // extern "C"

namespace {

struct Views {
    EmuFrame k;
    DevKfpKF K;
    DevKfpPoints P;
    std::vector<ProjDesc> pdesc;  // aligned copy
};

void make_views(const kfpe_problem& p, Views& v) {
    make_frame_view(p, p.nk, nullptr, v.k);
    static_cast<DevProjFrame&>(v.K) = v.k.F;
    v.pdesc = emu_aligned_descs(p.pdesc, p.np);
    v.P = DevKfpPoints{p.state, p.pos, p.normal, p.dmax, p.dmin, v.pdesc.data(), p.np};
}

int finish(const kfpe_problem& p, const std::vector<int>& claim, int32_t* out) {
    for (int f = 0; f < p.nk; ++f) out[f] = -1;
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

// The reference's loop, point by point in list order (:261-349).  Returns nmatches.
int kfpe_search_sequential(const kfpe_problem* p, int32_t* out) {
    Views v;
    make_views(*p, v);
    float R[9], t[3];
    kfp_decompose(p->Scw, false, R, t);
    std::vector<int> owner((size_t)p->nk + 1), claim((size_t)p->np + 1, -1);
    for (int f = 0; f < p->nk; ++f) owner[f] = p->occupied[f] ? kProjOccupied : kProjFree;
    for (int i = 0; i < p->np; ++i) {
        if (!kfp_eligible(v.P, p->skip, i)) continue;
        const ProjRec q = kfp_setup(v.K, v.P, R, t, i, p->th, false);
        const int b = kfp_best(v.K, q, v.P.desc[i], i, owner.data());
        claim[i] = b;
        if (b >= 0) owner[b] = i;  // vpMatched[bestIdx] = pMP (:345)
    }
    return finish(*p, claim, out);
}

// The kernels' work (kfproj.hip): kfp_setup_point for every point, then the rounds.  Returns nmatches;
// *rounds = rounds run; *fallbacks = window walks taken because the cached four were gone.
int kfpe_search_fixed_point(const kfpe_problem* p, int32_t* out, int32_t* rounds, int32_t* fallbacks) {
    Views v;
    make_views(*p, v);
    std::vector<int> claim((size_t)p->np + 1);
    std::vector<ProjRec> rec((size_t)p->np + 1);
    std::vector<ProjCand> cand((size_t)p->np + 1);
    KfProjProblem Q{};
    Q.K = v.K;
    Q.P = v.P;
    std::memcpy(Q.Scw, p->Scw, 12 * sizeof(float));
    Q.already = p->skip;
    Q.occupied = p->occupied;
    Q.rec = rec.data();
    Q.cand = cand.data();
    Q.claim = claim.data();
    int n_eligible = 0;
    for (int i = 0; i < p->np; ++i) {
        kfp_setup_point(Q, i, p->th);
        n_eligible += rec[i].cells >= 0;
    }
    *rounds = emu_rounds(KfpRounds{Q}, p->nk, Q.claim, n_eligible, fallbacks);
    return finish(*p, claim, out);
}

// Fuse (:846-928), point by point.  Returns the number of best_idx >= 0.
int kfpe_fuse(const kfpe_problem* p, int32_t* best_idx) {
    Views v;
    make_views(*p, v);
    int n = 0;
    for (int i = 0; i < p->np; ++i) {
        best_idx[i] = kfp_fuse_point(v.K, v.P, p->Scw, p->skip, i, p->th);
        n += best_idx[i] >= 0;
    }
    return n;
}

// LoopClosing.cpp:318-320 for `count` pairs: S_cm [count][8], R_mw [count][9], t_mw [count][3] ->
// S_cw [count][8], T [count][16]
void kfpe_compose(int count, const double* S_cm, const float* R_mw, const float* t_mw, double* S_cw, float* T) {
    for (int c = 0; c < count; ++c) {
        const SoSim3 a = sc_sim3_from_array(S_cm + 8 * c);
        const SoSim3 b = sc_sim3_from_pose(R_mw + 9 * c, t_mw + 3 * c);
        const SoSim3 o = sc_compose(a, b);
        sc_sim3_to_array(o, S_cw + 8 * c);
        sc_to_iso(o, T + 16 * c);
    }
}

}  // extern "C"

#ifdef KFPE_MAIN
// A crowded problem drawn here: clusters of keypoints a few pixels apart with near-identical descriptors and
// more points than keypoints projecting onto each cluster; identity pose, points at z = 4.
namespace {
uint32_t g_state = 12345u;
uint32_t rnd() {
    g_state = g_state * 1664525u + 1013904223u;
    return g_state >> 8;
}
float unif(float a, float b) { return a + (b - a) * (float)(rnd() & 0xffff) / 65536.0f; }
}  // namespace

int main() {
    const int clusters = 30, per_kp = 8, per_pt = 12, nk = clusters * per_kp + 200, np = clusters * per_pt + 400;
    const float W = 752.0f, H = 480.0f, fx = 435.0f, fy = 435.0f, cx = 367.0f, cy = 252.0f;
    std::vector<float> kp(2 * nk), pos(3 * np), normal(3 * np), dmax(np), dmin(np), scale(8);
    std::vector<int32_t> octave(nk), out_seq(nk), out_fp(nk), best(np);
    std::vector<uint8_t> desc(32 * (size_t)nk), pdesc(32 * (size_t)np), state(np, 1), skip(np, 0), occupied(nk, 0);
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
    for (; k < nk; ++k) {
        kp[2 * k] = unif(2, W - 2);
        kp[2 * k + 1] = unif(2, H - 2);
        octave[k] = (int)(rnd() % 8);
        for (int b = 0; b < 32; ++b) desc[32 * (size_t)k + b] = (uint8_t)rnd();
    }
    for (; i < np; ++i) {
        const int src = (int)(rnd() % nk);
        place(i, kp[2 * src] + unif(-1, 1), kp[2 * src + 1] + unif(-1, 1), octave[src]);
        std::memcpy(&pdesc[32 * (size_t)i], &desc[32 * (size_t)src], 32);
        for (int f = 0; f < 8; ++f) pdesc[32 * (size_t)i + rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
        if (rnd() % 20 == 0) state[i] = 2;
        if (rnd() % 20 == 0) skip[i] = 1;
        if (rnd() % 20 == 0) pos[3 * i + 2] = rnd() % 2 ? -4.0f : 0.0f;  // behind the camera / z == 0
    }
    for (int f = 0; f < nk; ++f) occupied[f] = rnd() % 10 == 0;
    // mGrid as CSR with PosInGrid's rounding
    const float gw = 64.0f / W, gh = 48.0f / H;
    std::vector<int32_t> begin(64 * 48 + 1, 0), feat(nk), cell(nk);
    for (int f = 0; f < nk; ++f) {
        int px = (int)floorf(kp[2 * f] * gw + 0.5f), py = (int)floorf(kp[2 * f + 1] * gh + 0.5f);
        if (px > 63) px = 63;
        if (py > 47) py = 47;
        cell[f] = px * 48 + py;
        ++begin[cell[f] + 1];
    }
    for (int c = 0; c < 64 * 48; ++c) begin[c + 1] += begin[c];
    std::vector<int32_t> fill(begin.begin(), begin.end() - 1);
    for (int f = 0; f < nk; ++f) feat[fill[cell[f]]++] = f;
    const float S[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    kfpe_problem p{nk, kp.data(), octave.data(), desc.data(), begin.data(), feat.data(), scale.data(), 8,
                   0.0f, W, 0.0f, H, gw, gh, fx, fy, cx, cy, logf(1.2f),
                   np, state.data(), pos.data(), normal.data(), dmax.data(), dmin.data(), pdesc.data(),
                   S, skip.data(), occupied.data(), 10.0f};
    int32_t rounds = 0, walks = 0;
    const int n1 = kfpe_search_sequential(&p, out_seq.data());
    const int n2 = kfpe_search_fixed_point(&p, out_fp.data(), &rounds, &walks);
    int mismatches = n1 != n2;
    for (int f = 0; f < nk; ++f) mismatches += out_seq[f] != out_fp[f];
    float S2[16];
    for (int e = 0; e < 16; ++e) S2[e] = S[e] * (e < 12 ? 1.5f : 1.0f);
    p.Scw = S2;
    p.th = 4.0f;
    const int nf = kfpe_fuse(&p, best.data());
    // one composition per matrix-to-quaternion branch (trace > 0, then each largest diagonal)
    const float Rm[4][9] = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {1, 0, 0, 0, -1, 0, 0, 0, -1}, {-1, 0, 0, 0, 1, 0, 0, 0, -1},
                            {-1, 0, 0, 0, -1, 0, 0, 0, 1}};
    const double Scm[8] = {0.1, -0.2, 0.05, 0.97, 0.3, -0.1, 0.2, 1.1};
    double acc = 0.0;
    for (int b = 0; b < 4; ++b) {
        const float tm[3] = {0.5f, -0.25f, 1.0f};
        double Scw8[8];
        float T[16];
        kfpe_compose(1, Scm, Rm[b], tm, Scw8, T);
        for (int e = 0; e < 16; ++e) acc += T[e];
    }
    std::printf("{\"mismatches\": %d, \"nmatches\": %d, \"rounds\": %d, \"fallback_walks\": %d, \"nfused\": %d, "
                "\"compose_sum\": %.6f}\n", mismatches, n1, rounds, walks, nf, acc);
    return mismatches ? 1 : 0;
}
#endif
