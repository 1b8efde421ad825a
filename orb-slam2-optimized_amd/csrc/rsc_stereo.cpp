// rsc_stereo.cpp — the stereo matcher of the C ABI: rsc_compute_stereo_matches_many
// (Frame::ComputeStereoMatches over a batch of resident Frame views, rsc_stereo.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "rsc_host.h"
#include "rsc_stereo.h"

static_assert(sizeof(rsc_stereo_result) == sizeof(StereoOut), "StereoOut is rsc_stereo_result");

extern "C" {

namespace {
int stm_refuse(const char* why) {
    g_last_error = why;
    return RSC_ERR_ARG;
}
}  // namespace

int rsc_compute_stereo_matches_many(rsc_context* C, rsc_frameview* const* frames, const rsc_right_features* right,
                                    int count, const float* mbf, const float* mb, int set_stereo,
                                    float* const* u_right, float* const* depth, int32_t* const* best_right,
                                    int32_t* const* best_dist, rsc_stereo_result* result) {
    if (!C || count < 0) return RSC_ERR_ARG;
    if (count == 0) return RSC_OK;
    if (!frames || !right || !mbf || !mb || !u_right || !depth || !result) return RSC_ERR_ARG;
    if (count > 65535) return stm_refuse("more than 65535 frames in one call");
    int max_left = 0;
    for (int c = 0; c < count; ++c) {
        const rsc_frameview* v = frames[c];
        const rsc_right_features& r = right[c];
        if (!v) return RSC_ERR_ARG;
        if (v->ctx != C) return stm_refuse("a Frame view of another context");
        if (r.n < 0) return RSC_ERR_ARG;
        if (r.n > kStmMaxRight) return stm_refuse("more than RSC_STEREO_MAX_RIGHT (8192) right keypoints");
        if (r.n > 0 && (!r.kp || !r.octave || !r.desc)) return RSC_ERR_ARG;
        if (v->n > 0 && (!u_right[c] || !depth[c])) return RSC_ERR_ARG;
        if (!std::isfinite(mbf[c]) || !(mbf[c] > 0.0f) || !std::isfinite(mb[c]) || !(mb[c] > 0.0f))
            return stm_refuse("mbf and mb must be finite and positive");
        for (int i = 0; i < 2 * r.n; ++i)
            if (!std::isfinite(r.kp[i])) return stm_refuse("a non-finite right keypoint coordinate");
        const int n_levels = (int)v->inv_level_sigma2.size();
        for (int i = 0; i < v->n; ++i)
            if (v->octave[i] < 0 || v->octave[i] >= n_levels) return stm_refuse("a left keypoint octave out of range");
        max_left = std::max(max_left, v->n);
    }
    if (set_stereo) {
        std::vector<const rsc_frameview*> seen(frames, frames + count);
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
            return stm_refuse("the same Frame view twice in one call with set_stereo");
        RSC_HIP(hipSetDevice(C->device));
        for (int c = 0; c < count; ++c)  // the kernel writes the view's own mvuRight
            if (int e = frames[c]->d_uright.ensure((size_t)std::max(frames[c]->n, 1))) return e;
    }
    // layout: problem table | per frame kp, octave, desc of the right image (uploaded)
    //         | per frame u_right, depth, best_right, best_dist, result (comes back); no scratch
    struct Off {
        size_t kp, oct, desc, u, z, br, bd, res;
    };
    std::vector<Off> off((size_t)count);
    Arena A;
    const size_t o_tab = A.take(sizeof(StereoProblem) * (size_t)count);
    for (int c = 0; c < count; ++c) {
        const size_t n = (size_t)std::max(right[c].n, 1);
        off[c].kp = A.take(8 * n);
        off[c].oct = A.take(4 * n);
        off[c].desc = A.take(32 * n);
    }
    A.end_upload();
    A.end_scratch();
    for (int c = 0; c < count; ++c) {
        const size_t n = (size_t)std::max(frames[c]->n, 1);
        off[c].u = A.take(4 * n);
        off[c].z = A.take(4 * n);
        off[c].br = A.take(4 * n);
        off[c].bd = A.take(4 * n);
        off[c].res = A.take(sizeof(StereoOut));
    }
    A.finish();
    auto fill = [&](char* h, char* d) -> int {
        StereoProblem* tab = reinterpret_cast<StereoProblem*>(h + o_tab);
        for (int c = 0; c < count; ++c) {
            const rsc_right_features& r = right[c];
            const size_t n = (size_t)r.n;
            if (n) {
                std::memcpy(h + off[c].kp, r.kp, 8 * n);
                std::memcpy(h + off[c].oct, r.octave, 4 * n);
                std::memcpy(h + off[c].desc, r.desc, 32 * n);
            }
            StereoProblem P{};
            P.left = frames[c]->hdr;
            P.r_kp = reinterpret_cast<const ProjPt*>(d + off[c].kp);
            P.r_octave = reinterpret_cast<const int32_t*>(d + off[c].oct);
            P.r_desc = reinterpret_cast<const ProjDesc*>(d + off[c].desc);
            P.u_right = reinterpret_cast<float*>(d + off[c].u);
            P.depth = reinterpret_cast<float*>(d + off[c].z);
            P.best_right = reinterpret_cast<int32_t*>(d + off[c].br);
            P.best_dist = reinterpret_cast<int32_t*>(d + off[c].bd);
            P.view_uright = set_stereo ? frames[c]->d_uright.p : nullptr;
            P.result = reinterpret_cast<StereoOut*>(d + off[c].res);
            P.n_left = frames[c]->n;
            P.n_right = r.n;
            P.mbf = mbf[c];
            P.mb = mb[c];
            tab[c] = P;
        }
        return 0;
    };
    auto launch = [&](char* d) {
        return launch_stereo(reinterpret_cast<const StereoProblem*>(d + o_tab), count, max_left,
                             C->timing ? C->ev[5] : nullptr, C->stream);
    };
    if (int e = arena_run(C, C->d_fp, C->h_fp, A, fill, launch, true, /*mid=*/true)) return e;
    const char* h = C->h_fp.p;
    for (int c = 0; c < count; ++c) {
        rsc_frameview* v = frames[c];
        const size_t n = (size_t)v->n;
        if (n) {
            std::memcpy(u_right[c], h + off[c].u, 4 * n);
            std::memcpy(depth[c], h + off[c].z, 4 * n);
            if (best_right && best_right[c]) std::memcpy(best_right[c], h + off[c].br, 4 * n);
            if (best_dist && best_dist[c]) std::memcpy(best_dist[c], h + off[c].bd, 4 * n);
        }
        std::memcpy(&result[c], h + off[c].res, sizeof(StereoOut));
        if (set_stereo) {  // as rsc_frameview_set_stereo(v, u_right[c], mbf[c]) leaves the view
            const float* u = reinterpret_cast<const float*>(h + off[c].u);
            v->h_uright.assign(u, u + n);
            v->mbf = mbf[c];
            v->has_stereo = true;
        }
    }
    return RSC_OK;
}

}  // extern "C"
