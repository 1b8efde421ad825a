// Frame.hpp — Frame::ComputeStereoMatches() (src/Frame.cpp:538-673, the keypoint-only matcher) in one device call
// (rsc_compute_stereo_matches_many), header-only and templated on the caller's Frame like the other facades.
//
//     rsc_orb::ComputeStereoMatches(F)          uploads F, writes F.mvuRight and F.mvDepth
//     rsc_orb::ComputeStereoMatches(F, view)    the same on a view the caller keeps (detail::upload_frameview(F)):
//                                               the view is left as after rsc_frameview_set_stereo, so the
//                                               trackers can run on it without another upload
//
// What it reads of the Frame: what detail::upload_frameview reads (N, mvKeysUn, mDescriptors, mGrid, the image
// bounds, the intrinsics, mvScaleFactors, mnScaleLevels, mfLogScaleFactor), mvKeysRight, mDescriptorsRight, mbf and
// mb.  The reference calls the function from the constructor before mb is assigned (:130 against :157) and so
// computes with an indeterminate mb; call this at the end of the constructor, after mb = mbf / fx and
// AssignFeaturesToGrid().  At most RSC_STEREO_MAX_RIGHT right keypoints, mbf and mb finite and
// positive, right keypoint coordinates finite: limits the reference does not have (include/rsc.h).
#pragma once
#include <cstdint>
#include <vector>
#include "ORBmatcher.hpp"

namespace rsc_orb {

namespace detail {

template <class FrameT>
rsc_stereo_result compute_stereo(FrameT& F, rsc_frameview* view, int set_stereo) {
    const size_t n = (size_t)F.N, m = F.mvKeysRight.size();
    std::vector<float> kp(2 * m + 2);
    std::vector<int32_t> oct(m + 1);
    std::vector<uint8_t> desc(32 * m + 32);
    for (size_t j = 0; j < m; ++j) {
        kp[2 * j] = F.mvKeysRight[j].pt.x;
        kp[2 * j + 1] = F.mvKeysRight[j].pt.y;
        oct[j] = F.mvKeysRight[j].octave;
        const uint8_t* row = F.mDescriptorsRight.template ptr<uint8_t>((int)j);
        std::copy(row, row + 32, desc.begin() + 32 * j);
    }
    rsc_right_features right;
    right.n = (int32_t)m;
    right.kp = kp.data();
    right.octave = oct.data();
    right.desc = desc.data();
    std::vector<float> u(n + 1, -1.0f), z(n + 1, -1.0f);
    float* up = u.data();
    float* zp = z.data();
    const float mbf = F.mbf, mb = F.mb;
    rsc_stereo_result res;
    check(rsc_compute_stereo_matches_many(thread_context(), &view, &right, 1, &mbf, &mb, set_stereo, &up, &zp, nullptr,
                                          nullptr, &res),
          "rsc_compute_stereo_matches_many");
    F.mvuRight.assign(u.begin(), u.begin() + (std::ptrdiff_t)n);
    F.mvDepth.assign(z.begin(), z.begin() + (std::ptrdiff_t)n);
    return res;
}

}  // namespace detail

// Returns the call's record: matches accepted before the cut, removed by it, the median distance and thDist.
template <class FrameT>
rsc_stereo_result ComputeStereoMatches(FrameT& F) {
    detail::FrameViewUpload fv = detail::upload_frameview(F);
    return detail::compute_stereo(F, fv.h, 0);
}

template <class FrameT>
rsc_stereo_result ComputeStereoMatches(FrameT& F, detail::FrameViewUpload& view) {
    return detail::compute_stereo(F, view.h, 1);
}

}  // namespace rsc_orb
