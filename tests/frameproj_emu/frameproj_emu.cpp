// TEST-ONLY host build of ORBmatcher::SearchByProjection's device arithmetic (rsc_frameproj.h): the
// per-MapPoint functions the kernel runs, driven (a) by a literal sequential loop in the reference's
// order — also the one-core CPU baseline of tools/frameproj_bench.py — and (b) by the fixed-point
// rounds exactly as frameproj.hip runs them.  The product library never contains this code path.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../orb-slam2-optimized_amd/csrc/rsc_frameproj.h"
#include "../proj_emu_common.h"

using namespace rsc;

extern "C" {

struct fpe_problem {
    // Frame
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
    // KeyFrame
    int32_t nk;
    const uint8_t* mp_state;
    const float* mp_pos;
    const float* mp_dmax;
    const float* mp_dmin;
    const uint8_t* mp_desc;
    const float* kf_angle;
    // call
    const float* Tcw;
    const uint8_t* already;
    const int32_t* frame_mp;
    float th;
    int32_t orb_dist, check_orientation;
};

}  // extern "C"

namespace {

struct Views : EmuFrame {
    DevProjKF K;
    std::vector<ProjDesc> kdesc;  // aligned copy
};

void make_views(const fpe_problem& p, Views& v) {
    make_frame_view(p, p.nf, p.angle, v);
    v.kdesc = emu_aligned_descs(p.mp_desc, p.nk);
    v.K = DevProjKF{p.mp_state, p.mp_pos, p.mp_dmax, p.mp_dmin, v.kdesc.data(), p.kf_angle, p.nk};
}

// rotation check and output (:1405-1441) over the final claims
int finish(const fpe_problem& p, const Views& v, const std::vector<int>& claim, int32_t* out) {
    for (int f = 0; f < p.nf; ++f) out[f] = -1;
    int hist[kProjHistoLength] = {};
    int keep[3] = {-1, -1, -1};
    if (p.check_orientation) {
        for (int i = 0; i < p.nk; ++i)
            if (claim[i] >= 0) {
                const int b = proj_rot_bin(v.K.angle[i], v.F.angle[claim[i]]);
                if ((unsigned)b < (unsigned)kProjHistoLength) ++hist[b];
            }
        proj_keep_bins(hist, keep);
    }
    int n = 0;
    for (int i = 0; i < p.nk; ++i) {
        const int a = claim[i];
        if (a < 0) continue;
        if (p.check_orientation) {
            const int bin = proj_rot_bin(v.K.angle[i], v.F.angle[a]);
            if (bin != keep[0] && bin != keep[1] && bin != keep[2]) continue;
        }
        out[a] = i;
        ++n;
    }
    return n;
}

}  // namespace

extern "C" {

// The reference's loop, MapPoint by MapPoint in slot order (:1333-1420).  Returns nmatches.
int fpe_search_sequential(const fpe_problem* p, int32_t* out) {
    Views v;
    make_views(*p, v);
    std::vector<int> owner((size_t)p->nf + 1), claim((size_t)p->nk + 1, -1);
    for (int f = 0; f < p->nf; ++f) owner[f] = p->frame_mp[f] >= 0 ? kProjOccupied : kProjFree;
    for (int i = 0; i < p->nk; ++i) {
        if (!proj_eligible(v.K, p->already, i)) continue;
        const ProjRec q = proj_setup(v.F, v.K, p->Tcw, i, p->th);
        const int b = proj_best(v.F, q, v.K.mp_desc[i], i, owner.data(), p->orb_dist);
        claim[i] = b;
        if (b >= 0) owner[b] = i;  // CurrentFrame.mvpMapPoints[bestIdx2] = pMP (:1402)
    }
    return finish(*p, v, claim, out);
}

// The kernels' work (frameproj.hip): proj_setup_point for every MapPoint, then the rounds.  Returns nmatches;
// *rounds = rounds run.
int fpe_search_fixed_point(const fpe_problem* p, int32_t* out, int32_t* rounds) {
    Views v;
    make_views(*p, v);
    std::vector<int> claim((size_t)p->nk + 1);
    std::vector<ProjRec> rec((size_t)p->nk + 1);
    std::vector<ProjCand> cand((size_t)p->nk + 1);
    FrameProjProblem P{};
    P.F = &v.F;
    P.K = v.K;
    std::memcpy(P.Tcw, p->Tcw, 12 * sizeof(float));
    P.already = p->already;
    P.frame_mp = p->frame_mp;
    P.rec = rec.data();
    P.cand = cand.data();
    P.claim = claim.data();
    int n_eligible = 0;  // the MapPoints with a window
    for (int i = 0; i < p->nk; ++i) {
        proj_setup_point(P, i, p->th, p->orb_dist);
        n_eligible += rec[i].cells >= 0;
    }
    const int32_t* frame_mp = p->frame_mp;
    const auto occ = [frame_mp](int f) { return frame_mp[f] >= 0; };
    *rounds = emu_rounds(FrameRounds<decltype(occ)>{P, p->orb_dist, occ}, p->nf, P.claim, n_eligible, nullptr);
    return finish(*p, v, claim, out);
}

}  // extern "C"
