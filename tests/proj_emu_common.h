// TEST-ONLY: what the host emulations of the four projection matchers share (tests/frameproj_emu,
// tests/kfproj_emu, tests/localproj_emu, tests/lastproj_emu): the aligned copy of a Frame / KeyFrame and the
// fixed-point rounds of rsc_projrounds.h restated sequentially, driving the same matcher types as the kernels.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>
#include "../orb-slam2-optimized_amd/csrc/rsc_projcore.h"

namespace rsc {

inline std::vector<ProjDesc> emu_aligned_descs(const uint8_t* desc, int n) {
    std::vector<ProjDesc> d((size_t)n + 1);
    if (n) std::memcpy(d.data(), desc, 32 * (size_t)n);
    return d;
}

// the view over a problem's Frame / KeyFrame arrays (P: the emulation's problem struct), with aligned copies
struct EmuFrame {
    DevProjFrame F;
    std::vector<ProjDesc> fdesc;
    std::vector<ProjPt> kp;
};

template <class P>
void make_frame_view(const P& p, int n, const float* angle, EmuFrame& v) {
    v.fdesc = emu_aligned_descs(p.desc, n);
    v.kp.resize((size_t)n + 1);
    if (n) std::memcpy(v.kp.data(), p.kp, 8 * (size_t)n);
    v.F = DevProjFrame{v.kp.data(), p.octave, angle, v.fdesc.data(), p.cell_begin, p.cell_feat, p.scale,
                       p.min_x, p.max_x, p.min_y, p.max_y, p.gw_inv, p.gh_inv, p.fx, p.fy, p.cx, p.cy, p.log_sf,
                       n, p.n_levels};
}

// The rounds of proj_rounds for matcher m: every round rebuilds the owner table from the blocking claims of the
// round before (a sequential atomicMin) and recomputes every point against it, from its cache or by walking
// its window; stops when no claim changed.  claim: -1 on entry, the fixed point on return.  Returns the rounds
// run; *walks (may be NULL) counts the window walks and *max_round_walks (may be NULL) the most of them in one
// round: the length the kernel's walk list (kProjWalkCap, rsc_projrounds.h) would need.
template <class M>
int emu_rounds(const M& m, int n_features, int32_t* claim, int n_eligible, int32_t* walks,
               int32_t* max_round_walks = nullptr) {
    const int n = m.n_points();
    std::vector<int> owner((size_t)n_features + 1), next((size_t)n + 1);
    int done = 0, walked = 0, most = 0;
    for (int r = 0; r < n_eligible + 1; ++r) {
        for (int f = 0; f < n_features; ++f) owner[f] = m.entry_occupied(f) ? kProjOccupied : kProjFree;
        for (int i = 0; i < n; ++i)
            if (claim[i] >= 0 && m.blocks(i) && i < owner[claim[i]]) owner[claim[i]] = i;
        bool changed = false;
        const int before = walked;
        for (int i = 0; i < n; ++i) {
            int b = m.pick(i, owner.data());
            if (b == kProjSkip) b = -1;
            if (b == -2) {
                b = m.best(i, owner.data());
                ++walked;
            }
            next[i] = b;
            changed |= b != claim[i];
        }
        std::memcpy(claim, next.data(), sizeof(int32_t) * (size_t)n);
        if (walked - before > most) most = walked - before;
        ++done;
        if (!changed) break;
    }
    if (walks) *walks = walked;
    if (max_round_walks) *max_round_walks = most;
    return done;
}

}  // namespace rsc
