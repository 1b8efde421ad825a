// ORBmatcher.hpp — drop-in facade of ORB_SLAM_CUSTOM::ORBmatcher::SearchByBoW (reference
// include/ORBmatcher.hpp:35-60, src/ORBmatcher.cpp:110-240 and :354-488) over the rsc C ABI: the
// Hamming-256 node-restricted matching, ratio test and rotation-histogram filter run on the MI355X
// (librsc.so); results are bit-identical to the reference's sequential walk.
//
// KeyFrameT needs (include/KeyFrame.hpp): N, mDescriptors with template ptr<uint8_t>(row) (cv::Mat,
// 32 CV_8U columns), mvKeysUn[i].angle, mFeatVec (DBoW2::FeatureVector: std::map<NodeId,
// std::vector<unsigned int>>) and GetMapPointMatches() (pointer-likes with isBad()).  FrameT needs
// N, mDescriptors, mvKeys[i].angle and mFeatVec.  In the reference tree:
//     rsc_orb::ORBmatcher matcher(0.75, true);                               // Tracking.cpp:1199
//     int nmatches = matcher.SearchByBoW(pKF, mCurrentFrame, vvpMapPointMatches[i]);  // :1214
//     int nmatches = matcher.SearchByBoW(mpCurrentKF, pKF, vvpMapPointMatches[i]);   // LoopClosing.cpp:251
// and the batched forms run a whole candidate loop (Tracking.cpp:1207-1232,
// LoopClosing.cpp:238-265) in one launch with the shared view uploaded once.
//
// SearchBySim3 (ORBmatcher.cpp:948-1170, LoopClosing.cpp:309) additionally needs, per KeyFrame,
// mvKeysUn[i].pt/.octave, mDescriptors, fx..cy, mnMinX..mnMaxY, mfGridElementWidth/HeightInv,
// mvScaleFactors, mnScaleLevels, mfLogScaleFactor, GetRotation(), GetTranslation(),
// GetMapPointMatches(); per MapPoint isBad(), GetWorldPos(), GetDescriptor() (one cv::Mat row),
// GetIndexInKeyFrame(pKF).  Three members the reference keeps protected are read through the
// customization points below, whose defaults call one-line getters INTEGRATION.md §2 adds to the
// reference: KeyFrame::GetGrid() (mGrid: the grid cannot be rebuilt from the KeyFrame's integer
// image bounds, Frame assigned it with float bounds) and MapPoint::GetMaxDistance()/GetMinDistance()
// (mfMaxDistance/mfMinDistance: GetMaxDistanceInvariance() returns 1.2f*mfMaxDistance, which does
// not round-trip in float).
//
// SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cpp:1317-1444; the
// refinement of Tracking::Relocalization, Tracking.cpp:1296 and :1310) reads the KeyFrame as SearchBySim3
// does plus mvKeysUn[i].angle, and of the Frame only public members (include/Frame.hpp): N, mvKeysUn,
// mDescriptors, mGrid, mnMinX..mnMaxY, mfGridElementWidthInv/HeightInv, fx..cy, mvScaleFactors,
// mnScaleLevels, mfLogScaleFactor, mTcw (rotation() / translation()) and mvpMapPoints, which it writes.
//
// SearchByProjection(F, vpMapPoints, th) (ORBmatcher.cpp:16-100; Tracking.cpp:1027) and the helper
// rsc_orb::SearchLocalPoints (Tracking.cpp:1003-1028) additionally read the Frame's mvuRight, mbf and mnId,
// and per MapPoint Observations(), GetNormal(), mnLastFrameSeen and the track members mbTrackInView,
// mTrackProjX, mTrackProjY, mTrackProjXR, mnTrackScaleLevel, mTrackViewCos; the helper writes those back and
// calls IncreaseVisible().  The points must be distinct and non-null (mvpLocalMapPoints is built through
// mnTrackReferenceForFrame, Tracking.cpp:1041-1062, which guarantees both).
//
// SearchByProjection(CurrentFrame, LastFrame, th) (ORBmatcher.cpp:1173-1315; Tracking.cpp:732,738) and the
// helper rsc_orb::TrackWithMotionModel (Tracking.cpp:724-774) read of the last Frame N, mvKeys[i].octave,
// mvKeysUn[i].angle, mvpMapPoints, mvbOutlier and mTcw, per MapPoint GetWorldPos(), GetDescriptor() and
// Observations(), and of the current Frame additionally mb; the helper also needs mnId, mvbOutlier, mTcw(r, c)
// and SetPose as rsc_orb::PoseOptimization does, and writes mbTrackInView / mnLastFrameSeen on the MapPoints it
// discards as outliers.
//
// SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) (ORBmatcher.cpp:489-669;
// LocalMapping.cpp:242) reads the KeyFrames as SearchBySim3 does plus mFeatVec, mvKeys[i].pt, mvuRight, mvDepth,
// mb, mbf, invfx, invfy, mfScaleFactor, mKinv and the stored inverse pose, the one protected member, through the
// customization point kf_pose_inverse (default: the reference's public KeyFrame::GetPoseInverse()).
#pragma once
#include <algorithm>
#include <cmath>
#include <memory>
#include <set>
#include <stdexcept>
#include <utility>
#include <vector>
#include "rsc_context.hpp"

namespace rsc_orb {

namespace detail {

// A KeyFrame's or Frame's SearchByBoW inputs uploaded to HBM (rsc_bow_create).
struct BowUpload {
    rsc_bow* h = nullptr;
    int n = 0;
    BowUpload() = default;
    BowUpload(const BowUpload&) = delete;
    BowUpload& operator=(const BowUpload&) = delete;
    BowUpload(BowUpload&& o) noexcept : h(o.h), n(o.n) { o.h = nullptr; }
    ~BowUpload() { rsc_bow_destroy(h); }

    // angles(i) gives the keypoint angle the overload reads; valid(i) the map-point test (or true)
    template <class ViewT, class AngleF, class ValidF>
    void build(const ViewT& v, AngleF angles, ValidF valid) {
        n = (int)v.N;
        std::vector<uint8_t> desc(32 * (size_t)n), ok((size_t)n);
        std::vector<float> ang((size_t)n);
        for (int i = 0; i < n; ++i) {
            const uint8_t* row = v.mDescriptors.template ptr<uint8_t>(i);
            std::copy(row, row + 32, desc.begin() + 32 * (size_t)i);
            ang[i] = angles(i);
            ok[i] = valid(i) ? 1 : 0;
        }
        std::vector<uint32_t> ids, feat;
        std::vector<int32_t> begin(1, 0);
        for (const auto& node : v.mFeatVec) {  // std::map order = ascending node ids
            ids.push_back((uint32_t)node.first);
            for (auto f : node.second) feat.push_back((uint32_t)f);
            begin.push_back((int32_t)feat.size());
        }
        rsc_bow_features f;
        f.n = n;
        f.desc = desc.data();
        f.angle = ang.data();
        f.valid = ok.data();
        f.n_nodes = (int32_t)ids.size();
        f.node_id = ids.data();
        f.node_begin = begin.data();
        f.feat = feat.data();
        check(rsc_bow_create(thread_context(), &f, &h), "rsc_bow_create");
    }
};

// pKF side: mvKeysUn angles (ORBmatcher.cpp:185, :435), valid = map point present and not bad
template <class KFPtr>
BowUpload upload_keyframe(const KFPtr& pKF) {
    const auto mps = pKF->GetMapPointMatches();
    BowUpload u;
    u.build(*pKF, [&](int i) { return (float)pKF->mvKeysUn[i].angle; },
            [&](int i) { return (size_t)i < mps.size() && mps[i] && !mps[i]->isBad(); });
    return u;
}

// Frame side of the Frame overload: mvKeys angles (:185), no map-point test
template <class FrameT>
BowUpload upload_frame(const FrameT& F) {
    BowUpload u;
    u.build(F, [&](int i) { return (float)F.mvKeys[i].angle; }, [](int) { return true; });
    return u;
}

// ---- SearchBySim3 ----------------------------------------------------------------------------------
// Customization points (specialise for types with other accessors).
template <class KF>
const auto& kf_grid(const KF& kf) { return kf.GetGrid(); }                   // KeyFrame::mGrid
template <class MP>
float mp_max_distance(MP& mp) { return mp.GetMaxDistance(); }                // MapPoint::mfMaxDistance
template <class MP>
float mp_min_distance(MP& mp) { return mp.GetMinDistance(); }                // MapPoint::mfMinDistance

// A KeyFrame's SearchBySim3 inputs uploaded to HBM (rsc_kfview_create).
struct KFViewUpload {
    rsc_kfview* h = nullptr;
    int n = 0;
    KFViewUpload() = default;
    KFViewUpload(const KFViewUpload&) = delete;
    KFViewUpload& operator=(const KFViewUpload&) = delete;
    KFViewUpload(KFViewUpload&& o) noexcept : h(o.h), n(o.n) { o.h = nullptr; }
    ~KFViewUpload() { rsc_kfview_destroy(h); }
};

template <class KFPtr, class MPPtr>
KFViewUpload upload_kfview(const KFPtr& pKF, const std::vector<MPPtr>& mps) {
    const auto& K = *pKF;
    const int n = (int)K.N;
    std::vector<float> kp(2 * (size_t)n), pos(3 * (size_t)n, 0.f), dmax((size_t)n, 0.f), dmin((size_t)n, 0.f);
    std::vector<int32_t> oct((size_t)n);
    std::vector<uint8_t> desc(32 * (size_t)n), state((size_t)n, 0), mdesc(32 * (size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        kp[2 * i] = K.mvKeysUn[i].pt.x;
        kp[2 * i + 1] = K.mvKeysUn[i].pt.y;
        oct[i] = K.mvKeysUn[i].octave;
        const uint8_t* row = K.mDescriptors.template ptr<uint8_t>(i);
        std::copy(row, row + 32, desc.begin() + 32 * (size_t)i);
        if ((size_t)i >= mps.size() || !mps[i]) continue;  // vpMapPoints[i] NULL
        auto& mp = *mps[i];
        if (mp.isBad()) { state[i] = 2; continue; }
        state[i] = 1;
        const auto X = mp.GetWorldPos();
        for (int c = 0; c < 3; ++c) pos[3 * i + c] = X(c);
        dmax[i] = mp_max_distance(mp);
        dmin[i] = mp_min_distance(mp);
        const auto d = mp.GetDescriptor();
        const uint8_t* dr = d.template ptr<uint8_t>(0);
        std::copy(dr, dr + 32, mdesc.begin() + 32 * (size_t)i);
    }
    const auto& grid = kf_grid(K);  // mGrid[ix][iy] -> CSR over cell = ix * 48 + iy
    if (grid.size() != 64) throw std::runtime_error("rsc: SearchBySim3: FRAME_GRID_COLS must be 64");
    std::vector<int32_t> begin(1, 0), feat;
    for (int ix = 0; ix < 64; ++ix) {
        if (grid[ix].size() != 48) throw std::runtime_error("rsc: SearchBySim3: FRAME_GRID_ROWS must be 48");
        for (int iy = 0; iy < 48; ++iy) {
            for (auto f : grid[ix][iy]) feat.push_back((int32_t)f);
            begin.push_back((int32_t)feat.size());
        }
    }
    if (feat.empty()) feat.push_back(0);
    rsc_sim3_kf k;
    k.n = n;
    k.kp = kp.data();
    k.octave = oct.data();
    k.desc = desc.data();
    k.cell_begin = begin.data();
    k.cell_feat = feat.data();
    k.min_x = (float)K.mnMinX; k.max_x = (float)K.mnMaxX; k.min_y = (float)K.mnMinY; k.max_y = (float)K.mnMaxY;
    k.grid_w_inv = K.mfGridElementWidthInv;
    k.grid_h_inv = K.mfGridElementHeightInv;
    k.fx = K.fx; k.fy = K.fy; k.cx = K.cx; k.cy = K.cy;
    k.scale_factors = K.mvScaleFactors.data();
    k.n_levels = (int32_t)K.mnScaleLevels;
    k.log_scale_factor = K.mfLogScaleFactor;
    const auto R = pKF->GetRotation();
    const auto t = pKF->GetTranslation();
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) k.Rcw[3 * r + c] = R(r, c);
        k.tcw[r] = t(r);
    }
    k.mp_state = state.data();
    k.mp_pos = pos.data();
    k.mp_dmax = dmax.data();
    k.mp_dmin = dmin.data();
    k.mp_desc = mdesc.data();
    KFViewUpload u;
    u.n = n;
    check(rsc_kfview_create(thread_context(), &k, &u.h), "rsc_kfview_create");
    return u;
}

// One upload per distinct KeyFrame object of a list; ki[c] = the view of vpKFs[c] (shared by the matchers and by
// MapPoint.hpp).
template <class KFPtr>
void upload_distinct(const std::vector<KFPtr>& vpKFs, std::vector<KFViewUpload>& views, std::vector<int>& ki) {
    std::vector<const void*> keys;
    ki.assign(vpKFs.size(), 0);
    for (size_t c = 0; c < vpKFs.size(); ++c) {
        size_t j = 0;
        for (; j < keys.size(); ++j)
            if (keys[j] == (const void*)&*vpKFs[c]) break;
        if (j == keys.size()) {
            keys.push_back((const void*)&*vpKFs[c]);
            views.push_back(upload_kfview(vpKFs[c], vpKFs[c]->GetMapPointMatches()));
        }
        ki[c] = (int)j;
    }
}

// Customization point: Twc as KeyFrame::SetPose stored it (KeyFrame.cpp:64-66), an object with rotation() /
// translation() (Eigen::Isometry3f).
template <class KF>
auto kf_pose_inverse(KF& kf) { return kf.GetPoseInverse(); }

// What triangulation reads and the view lacks (rsc_kfview_set_triangulation).  cos_parallax_stereo is the
// expression of LocalMapping.cpp:286,288 on this host's libm.
template <class KFPtr>
void set_triangulation(KFViewUpload& u, const KFPtr& pKF) {
    using std::atan2;
    using std::cos;
    auto& K = *pKF;
    const size_t n = (size_t)u.n;
    std::vector<float> ur(n), depth(n), raw(2 * n), cs(n);
    for (size_t i = 0; i < n; ++i) {
        ur[i] = K.mvuRight[i];
        depth[i] = K.mvDepth[i];
        raw[2 * i] = K.mvKeys[i].pt.x;
        raw[2 * i + 1] = K.mvKeys[i].pt.y;
        cs[i] = cos(2*atan2(K.mb/2,K.mvDepth[i]));
    }
    rsc_kf_triangulation t;
    t.u_right = ur.data();
    t.depth = depth.data();
    t.kp_raw = raw.data();
    t.cos_parallax_stereo = cs.data();
    t.mb = K.mb; t.mbf = K.mbf; t.invfx = K.invfx; t.invfy = K.invfy;
    t.scale_factor = K.mfScaleFactor;
    const auto Twc = kf_pose_inverse(K);
    const auto R = Twc.rotation();
    const auto O = Twc.translation();
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            t.Rwc[3 * r + c] = R(r, c);
            t.Kinv[3 * r + c] = K.mKinv(r, c);
        }
        t.Ow[r] = O(r);
    }
    check(rsc_kfview_set_triangulation(u.h, &t), "rsc_kfview_set_triangulation");
}

// The current Frame's SearchByProjection inputs uploaded to HBM (rsc_frameview_create).
struct FrameViewUpload {
    rsc_frameview* h = nullptr;
    int n = 0;
    FrameViewUpload() = default;
    FrameViewUpload(const FrameViewUpload&) = delete;
    FrameViewUpload& operator=(const FrameViewUpload&) = delete;
    FrameViewUpload(FrameViewUpload&& o) noexcept : h(o.h), n(o.n) { o.h = nullptr; }
    ~FrameViewUpload() { rsc_frameview_destroy(h); }
};

template <class FrameT>
FrameViewUpload upload_frameview(const FrameT& F) {
    const int n = (int)F.N;
    std::vector<float> kp(2 * (size_t)n), ang((size_t)n);
    std::vector<int32_t> oct((size_t)n);
    std::vector<uint8_t> desc(32 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        kp[2 * i] = F.mvKeysUn[i].pt.x;
        kp[2 * i + 1] = F.mvKeysUn[i].pt.y;
        oct[i] = F.mvKeysUn[i].octave;
        ang[i] = F.mvKeysUn[i].angle;
        const uint8_t* row = F.mDescriptors.template ptr<uint8_t>(i);
        std::copy(row, row + 32, desc.begin() + 32 * (size_t)i);
    }
    std::vector<int32_t> begin(1, 0), feat;  // mGrid[ix][iy] -> CSR over cell = ix * 48 + iy
    for (int ix = 0; ix < 64; ++ix)
        for (int iy = 0; iy < 48; ++iy) {
            for (auto f : F.mGrid[ix][iy]) feat.push_back((int32_t)f);
            begin.push_back((int32_t)feat.size());
        }
    if (feat.empty()) feat.push_back(0);
    rsc_frame_features f;
    f.n = n;
    f.kp = kp.data();
    f.octave = oct.data();
    f.angle = ang.data();
    f.desc = desc.data();
    f.cell_begin = begin.data();
    f.cell_feat = feat.data();
    f.min_x = F.mnMinX; f.max_x = F.mnMaxX; f.min_y = F.mnMinY; f.max_y = F.mnMaxY;
    f.grid_w_inv = F.mfGridElementWidthInv;
    f.grid_h_inv = F.mfGridElementHeightInv;
    f.fx = F.fx; f.fy = F.fy; f.cx = F.cx; f.cy = F.cy;
    f.scale_factors = F.mvScaleFactors.data();
    f.n_levels = (int32_t)F.mnScaleLevels;
    f.log_scale_factor = F.mfLogScaleFactor;
    FrameViewUpload u;
    u.n = n;
    check(rsc_frameview_create(thread_context(), &f, &u.h), "rsc_frameview_create");
    return u;
}

// The last Frame's slots as SearchByProjection(CurrentFrame, LastFrame, th) reads them (rsc_lastframe_create).
struct LastFrameUpload {
    rsc_lastframe* h = nullptr;
    int n = 0;
    LastFrameUpload() = default;
    LastFrameUpload(const LastFrameUpload&) = delete;
    LastFrameUpload& operator=(const LastFrameUpload&) = delete;
    LastFrameUpload(LastFrameUpload&& o) noexcept : h(o.h), n(o.n) { o.h = nullptr; }
    ~LastFrameUpload() { rsc_lastframe_destroy(h); }
};

template <class FrameT>
LastFrameUpload upload_lastframe(const FrameT& L) {
    const size_t n = (size_t)L.N;
    std::vector<int32_t> oct(n, 0);
    std::vector<float> ang(n, 0.f), pos(3 * n, 0.f);
    std::vector<uint8_t> state(n, 0), desc(32 * n, 0), has_obs(n, 0);
    for (size_t i = 0; i < n; ++i) {
        oct[i] = L.mvKeys[i].octave;   // ORBmatcher.cpp:1223 reads mvKeys,
        ang[i] = L.mvKeysUn[i].angle;  // :1278 mvKeysUn
        if (i >= L.mvpMapPoints.size() || !L.mvpMapPoints[i]) continue;  // :1200
        auto& mp = *L.mvpMapPoints[i];
        state[i] = i < L.mvbOutlier.size() && L.mvbOutlier[i] ? 2 : 1;  // :1202
        const auto X = mp.GetWorldPos();
        for (int c = 0; c < 3; ++c) pos[3 * i + c] = X(c);
        const auto d = mp.GetDescriptor();
        const uint8_t* dr = d.template ptr<uint8_t>(0);
        std::copy(dr, dr + 32, desc.begin() + 32 * i);
        has_obs[i] = mp.Observations() > 0 ? 1 : 0;
    }
    rsc_last_frame_slots s;
    s.n = (int32_t)n;
    s.octave = oct.data();
    s.angle = ang.data();
    s.mp_state = state.data();
    s.mp_pos = pos.data();
    s.mp_desc = desc.data();
    s.mp_has_obs = has_obs.data();
    LastFrameUpload u;
    u.n = (int)n;
    check(rsc_lastframe_create(thread_context(), &s, &u.h), "rsc_lastframe_create");
    return u;
}

// A MapPoint list on the device (rsc_mpview_create) and its host arrays, for Fuse(pKF, vpMapPoints, th): the
// descriptor bytes are kept because a Replace can change a survivor's descriptor between two KeyFrames.
struct MPViewUpload {
    rsc_mpview* h = nullptr;
    MPViewUpload() = default;
    MPViewUpload(const MPViewUpload&) = delete;
    MPViewUpload& operator=(const MPViewUpload&) = delete;
    MPViewUpload(MPViewUpload&& o) noexcept : h(o.h) { o.h = nullptr; }
    ~MPViewUpload() { rsc_mpview_destroy(h); }
};

struct FusePoints {
    std::vector<uint8_t> state, desc;
    std::vector<float> pos, nrm, dmax, dmin;
    explicit FusePoints(size_t n)
        : state(n > 0 ? n : 1, 2), desc(32 * (n > 0 ? n : 1), 0), pos(3 * (n > 0 ? n : 1), 0.f),
          nrm(3 * (n > 0 ? n : 1), 0.f), dmax(n > 0 ? n : 1, 0.f), dmin(n > 0 ? n : 1, 0.f) {}
    template <class MP>
    void set(size_t i, MP& mp) {
        if (mp.isBad()) return;  // state 2
        state[i] = 1;
        const auto X = mp.GetWorldPos();
        const auto N = mp.GetNormal();
        for (int c = 0; c < 3; ++c) {
            pos[3 * i + c] = X(c);
            nrm[3 * i + c] = N(c);
        }
        dmax[i] = mp_max_distance(mp);
        dmin[i] = mp_min_distance(mp);
        const auto d = mp.GetDescriptor();
        const uint8_t* dr = d.template ptr<uint8_t>(0);
        std::copy(dr, dr + 32, desc.begin() + 32 * i);
    }
    void copy(size_t i, const FusePoints& o, size_t j) {
        state[i] = o.state[j];
        std::copy(o.pos.begin() + 3 * j, o.pos.begin() + 3 * j + 3, pos.begin() + 3 * i);
        std::copy(o.nrm.begin() + 3 * j, o.nrm.begin() + 3 * j + 3, nrm.begin() + 3 * i);
        dmax[i] = o.dmax[j];
        dmin[i] = o.dmin[j];
        std::copy(o.desc.begin() + 32 * j, o.desc.begin() + 32 * j + 32, desc.begin() + 32 * i);
    }
    MPViewUpload upload(size_t n) const {
        rsc_mappoints m;
        m.n = (int32_t)n;
        m.state = state.data();
        m.pos = pos.data();
        m.normal = nrm.data();
        m.dmax = dmax.data();
        m.dmin = dmin.data();
        m.desc = desc.data();
        MPViewUpload u;
        check(rsc_mpview_create(thread_context(), &m, &u.h), "rsc_mpview_create");
        return u;
    }
};

template <class IsoT>
void iso_to_array16(const IsoT& S, float* T) {
    const auto R = S.rotation();
    const auto t = S.translation();
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) T[4 * r + k] = R(r, k);
        T[4 * r + 3] = t(r);
    }
    T[12] = T[13] = T[14] = 0.f;
    T[15] = 1.f;
}

}  // namespace detail

// mvpLoopMapPoints uploaded once (rsc_mpview_create) and shared by the projection call of
// LoopClosing::ComputeSim3 and every Fuse call of LoopClosing::SearchAndFuse.  The points must be distinct
// and non-null (LoopClosing.cpp:350-353 guarantees both).  MapPoint additionally needs GetNormal().
template <class MPPtr>
class LoopMapPoints {
public:
    explicit LoopMapPoints(const std::vector<MPPtr>& vpPoints) : pts(vpPoints) {
        const size_t n = pts.size();
        std::vector<uint8_t> state(n, 2), desc(32 * n, 0);
        std::vector<float> pos(3 * n, 0.f), nrm(3 * n, 0.f), dmax(n, 0.f), dmin(n, 0.f);
        for (size_t i = 0; i < n; ++i) {
            if (!pts[i]) throw std::runtime_error("rsc: LoopMapPoints: null MapPoint");
            auto& mp = *pts[i];
            if (mp.isBad()) continue;
            state[i] = 1;
            const auto X = mp.GetWorldPos();
            const auto N = mp.GetNormal();
            for (int c = 0; c < 3; ++c) {
                pos[3 * i + c] = X(c);
                nrm[3 * i + c] = N(c);
            }
            dmax[i] = detail::mp_max_distance(mp);
            dmin[i] = detail::mp_min_distance(mp);
            const auto d = mp.GetDescriptor();
            const uint8_t* dr = d.template ptr<uint8_t>(0);
            std::copy(dr, dr + 32, desc.begin() + 32 * i);
        }
        rsc_mappoints m;
        m.n = (int32_t)n;
        m.state = state.data();
        m.pos = pos.data();
        m.normal = nrm.data();
        m.dmax = dmax.data();
        m.dmin = dmin.data();
        m.desc = desc.data();
        check(rsc_mpview_create(thread_context(), &m, &h), "rsc_mpview_create");
    }
    LoopMapPoints(const LoopMapPoints&) = delete;
    LoopMapPoints& operator=(const LoopMapPoints&) = delete;
    ~LoopMapPoints() { rsc_mpview_destroy(h); }
    rsc_mpview* handle() const { return h; }
    const std::vector<MPPtr>& points() const { return pts; }

private:
    std::vector<MPPtr> pts;
    rsc_mpview* h = nullptr;
};

class ORBmatcher {
public:
    // ORBmatcher::ORBmatcher (ORBmatcher.cpp:12; defaults include/ORBmatcher.hpp:35)
    explicit ORBmatcher(float nnratio = 0.6f, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

    // SearchByBoW(pKF, F, vpMapPointMatches) (ORBmatcher.cpp:110-240)
    template <class KFPtr, class FrameT, class MPPtr>
    int SearchByBoW(KFPtr pKF, FrameT& F, std::vector<MPPtr>& vpMapPointMatches) {
        std::vector<KFPtr> kfs(1, pKF);
        std::vector<std::vector<MPPtr>> out;
        const int n = SearchByBoWMany(kfs, F, out)[0];
        vpMapPointMatches.swap(out[0]);
        return n;
    }

    // SearchByBoW(pKF1, pKF2, vpMatches12) (ORBmatcher.cpp:354-488)
    template <class KFPtr, class MPPtr>
    int SearchByBoW(KFPtr pKF1, KFPtr pKF2, std::vector<MPPtr>& vpMatches12) {
        std::vector<KFPtr> kf2s(1, pKF2);
        std::vector<std::vector<MPPtr>> out;
        const int n = SearchByBoWMany(pKF1, kf2s, out)[0];
        vpMatches12.swap(out[0]);
        return n;
    }

    // SearchByBoW(vpKFs[c], F, out[c]) for every candidate in one launch (Tracking.cpp:1207-1232).
    template <class KFPtr, class FrameT, class MPPtr>
    std::vector<int> SearchByBoWMany(const std::vector<KFPtr>& vpKFs, FrameT& F,
                                     std::vector<std::vector<MPPtr>>& out) {
        const int C = (int)vpKFs.size();
        detail::BowUpload frame = detail::upload_frame(F);
        std::vector<detail::BowUpload> kfs;
        std::vector<rsc_bow*> hs;
        std::vector<std::vector<MPPtr>> mps;
        kfs.reserve(C);
        for (const auto& k : vpKFs) {
            kfs.push_back(detail::upload_keyframe(k));
            hs.push_back(kfs.back().h);
            mps.push_back(k->GetMapPointMatches());
        }
        std::vector<std::vector<int32_t>> idx(C, std::vector<int32_t>(frame.n > 0 ? frame.n : 1));
        std::vector<int32_t*> ptr(C);
        for (int c = 0; c < C; ++c) ptr[c] = idx[c].data();
        std::vector<int32_t> nm(C > 0 ? C : 1, 0);
        check(rsc_search_by_bow_frame_many(thread_context(), hs.data(), C, frame.h, mfNNratio,
                                           mbCheckOrientation ? 1 : 0, ptr.data(), nm.data()),
              "SearchByBoW(KeyFrame, Frame)");
        out.assign(C, std::vector<MPPtr>(frame.n, nullptr));  // vector<MapPoint*>(F.N, NULL) (:114)
        for (int c = 0; c < C; ++c)
            for (int i = 0; i < frame.n; ++i)
                if (idx[c][i] >= 0) out[c][i] = mps[c][idx[c][i]];
        return std::vector<int>(nm.begin(), nm.begin() + C);
    }

    // SearchByBoW(pKF1, vpKF2[c], out[c]) for every loop candidate in one launch
    // (LoopClosing.cpp:238-265).
    template <class KFPtr, class MPPtr>
    std::vector<int> SearchByBoWMany(KFPtr pKF1, const std::vector<KFPtr>& vpKF2,
                                     std::vector<std::vector<MPPtr>>& out) {
        const int C = (int)vpKF2.size();
        detail::BowUpload kf1 = detail::upload_keyframe(pKF1);
        std::vector<detail::BowUpload> kf2;
        std::vector<rsc_bow*> hs;
        std::vector<std::vector<MPPtr>> mps;
        kf2.reserve(C);
        for (const auto& k : vpKF2) {
            kf2.push_back(detail::upload_keyframe(k));
            hs.push_back(kf2.back().h);
            mps.push_back(k->GetMapPointMatches());
        }
        const int n1 = (int)pKF1->GetMapPointMatches().size();
        std::vector<std::vector<int32_t>> idx(C, std::vector<int32_t>(kf1.n > 0 ? kf1.n : 1));
        std::vector<int32_t*> ptr(C);
        for (int c = 0; c < C; ++c) ptr[c] = idx[c].data();
        std::vector<int32_t> nm(C > 0 ? C : 1, 0);
        check(rsc_search_by_bow_kf_many(thread_context(), kf1.h, hs.data(), C, mfNNratio, mbCheckOrientation ? 1 : 0,
                                        ptr.data(), nm.data()),
              "SearchByBoW(KeyFrame, KeyFrame)");
        out.assign(C, std::vector<MPPtr>(n1, nullptr));  // vpMatches12 sized vpMapPoints1 (:366)
        for (int c = 0; c < C; ++c)
            for (int i = 0; i < kf1.n && i < n1; ++i)
                if (idx[c][i] >= 0) out[c][i] = mps[c][idx[c][i]];
        return std::vector<int>(nm.begin(), nm.begin() + C);
    }

    // SearchBySim3(pKF1, pKF2, vpMatches12, R12, t12, th) (ORBmatcher.cpp:948-1170;
    // LoopClosing.cpp:309 after a Sim3Solver success): new mutual matches are written into
    // vpMatches12 (entries already set are kept), returns their number.
    template <class KFPtr, class MPPtr, class Mat3, class Vec3>
    int SearchBySim3(KFPtr pKF1, KFPtr pKF2, std::vector<MPPtr>& vpMatches12, const Mat3& R12, const Vec3& t12,
                     const float th) {
        std::vector<std::vector<MPPtr>*> m(1, &vpMatches12);
        std::vector<KFPtr> a(1, pKF1), b(1, pKF2);
        float R[9], t[3];
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) R[3 * r + c] = R12(r, c);
            t[r] = t12(r);
        }
        return SearchBySim3Many(a, b, m, R, t, th)[0];
    }

    // SearchBySim3 of several (pKF1[c], pKF2[c]) pairs in one launch; R12 [count][9] row-major,
    // t12 [count][3].  Each KeyFrame object is uploaded once.
    template <class KFPtr, class MPPtr>
    std::vector<int> SearchBySim3Many(const std::vector<KFPtr>& pKF1, const std::vector<KFPtr>& pKF2,
                                      const std::vector<std::vector<MPPtr>*>& vpMatches12, const float* R12,
                                      const float* t12, const float th) {
        const int C = (int)pKF1.size();
        std::vector<const void*> keys;
        std::vector<detail::KFViewUpload> views;
        std::vector<std::vector<MPPtr>> mps;
        auto view_of = [&](const KFPtr& k) {
            for (size_t j = 0; j < keys.size(); ++j)
                if (keys[j] == (const void*)&*k) return (int)j;
            keys.push_back((const void*)&*k);
            mps.push_back(k->GetMapPointMatches());
            views.push_back(detail::upload_kfview(k, mps.back()));
            return (int)keys.size() - 1;
        };
        std::vector<int> v1(C), v2(C);
        for (int c = 0; c < C; ++c) {
            v1[c] = view_of(pKF1[c]);
            v2[c] = view_of(pKF2[c]);
        }
        std::vector<rsc_kfview*> h1(C), h2(C);
        std::vector<std::vector<int32_t>> in(C), out(C);
        std::vector<const int32_t*> pin(C);
        std::vector<int32_t*> pout(C);
        for (int c = 0; c < C; ++c) {
            h1[c] = views[v1[c]].h;
            h2[c] = views[v2[c]].h;
            const int n1 = views[v1[c]].n;
            const std::vector<MPPtr>& m = *vpMatches12[c];
            in[c].assign(n1 > 0 ? n1 : 1, -1);
            out[c].assign(n1 > 0 ? n1 : 1, -1);
            for (int i = 0; i < n1 && (size_t)i < m.size(); ++i) {  // vbAlreadyMatched1/2 (:980-990)
                if (!m[i]) continue;
                const int idx2 = m[i]->GetIndexInKeyFrame(pKF2[c]);
                in[c][i] = (idx2 >= 0 && idx2 < views[v2[c]].n) ? idx2 : -2;
            }
            pin[c] = in[c].data();
            pout[c] = out[c].data();
        }
        std::vector<int32_t> nfound(C > 0 ? C : 1, 0);
        check(rsc_search_by_sim3_many(thread_context(), h1.data(), h2.data(), C, R12, t12, th, pin.data(), pout.data(),
                                      nfound.data()),
              "SearchBySim3");
        for (int c = 0; c < C; ++c) {  // vpMatches12[i1] = vpMapPoints2[idx2] (:1160-1166)
            std::vector<MPPtr>& m = *vpMatches12[c];
            const std::vector<MPPtr>& mp2 = mps[v2[c]];
            for (int i = 0; i < views[v1[c]].n && (size_t)i < m.size(); ++i)
                if (out[c][i] >= 0) m[i] = mp2[out[c][i]];
        }
        return std::vector<int>(nfound.begin(), nfound.begin() + C);
    }

    // SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) (ORBmatcher.cpp:489-669;
    // LocalMapping.cpp:242): the matches of KeyFrame 1's features without a MapPoint against KeyFrame 2's under the
    // epipolar constraint, in ascending idx1.  When an eligible feature's epipolar line has den == 0 the
    // reference returns 0 before it touches vMatchedPairs (:552-553); so does this.
    template <class KFPtr, class Mat3>
    int SearchForTriangulation(KFPtr pKF1, KFPtr pKF2, const Mat3& F12,
                               std::vector<std::pair<size_t, size_t>>& vMatchedPairs, const bool bOnlyStereo) {
        detail::BowUpload b1 = detail::upload_keyframe(pKF1), b2 = detail::upload_keyframe(pKF2);
        detail::KFViewUpload v1 = detail::upload_kfview(pKF1, pKF1->GetMapPointMatches());
        detail::KFViewUpload v2 = detail::upload_kfview(pKF2, pKF2->GetMapPointMatches());
        detail::set_triangulation(v1, pKF1);
        detail::set_triangulation(v2, pKF2);
        float F[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) F[3 * r + c] = F12(r, c);
        std::vector<int32_t> m12((size_t)(v1.n > 0 ? v1.n : 1), -1);
        int32_t* out = m12.data();
        int32_t nmatches = 0, den_zero = 0;
        const rsc_bow* pb1 = b1.h;
        const rsc_bow* pb2 = b2.h;
        const int32_t only_stereo = bOnlyStereo ? 1 : 0;
        // the views' mp_state is GetMapPoint(idx) != nullptr, bad points included: no per-call flags
        check(rsc_search_for_triangulation_many(thread_context(), &pb1, &v1.h, &pb2, &v2.h, 1, F, nullptr, nullptr,
                                                &only_stereo, mbCheckOrientation ? 1 : 0, &out, &nmatches, &den_zero,
                                                nullptr),
              "SearchForTriangulation");
        if (den_zero) return 0;  // `return false`: vMatchedPairs untouched
        vMatchedPairs.clear();
        vMatchedPairs.reserve((size_t)nmatches);
        for (int i = 0; i < v1.n; ++i)
            if (m12[i] >= 0) vMatchedPairs.push_back(std::make_pair((size_t)i, (size_t)m12[i]));
        return nmatches;
    }

    // SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cpp:1317-1444): the
    // MapPoints of pKF that are not in sAlreadyFound are projected with CurrentFrame.mTcw and matched to
    // the free features of the Frame; the new matches are written to CurrentFrame.mvpMapPoints (those the
    // rotation check removes are not), returns their number.
    template <class FrameT, class KFPtr, class MPPtr>
    int SearchByProjection(FrameT& CurrentFrame, KFPtr pKF, const std::set<MPPtr>& sAlreadyFound, const float th,
                           const int ORBdist) {
        std::vector<FrameT*> f(1, &CurrentFrame);
        std::vector<KFPtr> k(1, pKF);
        std::vector<const std::set<MPPtr>*> s(1, &sAlreadyFound);
        return SearchByProjectionMany(f, k, s, th, ORBdist)[0];
    }

    // SearchByProjection(*frames[c], vpKFs[c], *sAlreadyFound[c], th, ORBdist) for several candidates in
    // one launch.  Each Frame and KeyFrame object is uploaded once; problems that share a Frame object all
    // read its mvpMapPoints as they were at the call (give each candidate its own Frame copy, as a
    // relocalization that evaluates candidates side by side does).
    template <class FrameT, class KFPtr, class MPPtr>
    std::vector<int> SearchByProjectionMany(const std::vector<FrameT*>& frames, const std::vector<KFPtr>& vpKFs,
                                            const std::vector<const std::set<MPPtr>*>& sAlreadyFound, const float th,
                                            const int ORBdist) {
        const int C = (int)frames.size();
        std::vector<const void*> fkeys, kkeys;
        std::vector<detail::FrameViewUpload> fviews;
        std::vector<detail::KFViewUpload> kviews;
        std::vector<std::vector<MPPtr>> mps;
        std::vector<int> fi(C), ki(C);
        for (int c = 0; c < C; ++c) {
            size_t j = 0;
            for (; j < fkeys.size(); ++j)
                if (fkeys[j] == (const void*)frames[c]) break;
            if (j == fkeys.size()) {
                fkeys.push_back((const void*)frames[c]);
                fviews.push_back(detail::upload_frameview(*frames[c]));
            }
            fi[c] = (int)j;
            for (j = 0; j < kkeys.size(); ++j)
                if (kkeys[j] == (const void*)&*vpKFs[c]) break;
            if (j == kkeys.size()) {
                kkeys.push_back((const void*)&*vpKFs[c]);
                mps.push_back(vpKFs[c]->GetMapPointMatches());
                kviews.push_back(detail::upload_kfview(vpKFs[c], mps.back()));
                const int n = kviews.back().n;
                std::vector<float> ang((size_t)(n > 0 ? n : 1), 0.f);
                for (int i = 0; i < n; ++i) ang[i] = vpKFs[c]->mvKeysUn[i].angle;
                check(rsc_kfview_set_angles(kviews.back().h, ang.data()), "rsc_kfview_set_angles");
            }
            ki[c] = (int)j;
        }
        std::vector<rsc_frameview*> hf(C);
        std::vector<rsc_kfview*> hk(C);
        std::vector<float> T(16 * (size_t)(C > 0 ? C : 1), 0.f);
        std::vector<std::vector<uint8_t>> already(C);
        std::vector<std::vector<int32_t>> occ(C), out(C);
        std::vector<const uint8_t*> pal(C);
        std::vector<const int32_t*> pocc(C);
        std::vector<int32_t*> pout(C);
        for (int c = 0; c < C; ++c) {
            FrameT& F = *frames[c];
            hf[c] = fviews[fi[c]].h;
            hk[c] = kviews[ki[c]].h;
            const auto R = F.mTcw.rotation();
            const auto t = F.mTcw.translation();
            for (int r = 0; r < 3; ++r) {
                for (int k = 0; k < 3; ++k) T[16 * (size_t)c + 4 * r + k] = R(r, k);
                T[16 * (size_t)c + 4 * r + 3] = t(r);
            }
            T[16 * (size_t)c + 15] = 1.f;
            const std::vector<MPPtr>& m = mps[ki[c]];
            const int nk = kviews[ki[c]].n, nf = fviews[fi[c]].n;
            already[c].assign((size_t)(nk > 0 ? nk : 1), 0);
            for (int i = 0; i < nk && (size_t)i < m.size(); ++i)
                if (m[i] && sAlreadyFound[c]->count(m[i])) already[c][i] = 1;
            occ[c].assign((size_t)(nf > 0 ? nf : 1), -1);
            out[c].assign((size_t)(nf > 0 ? nf : 1), -1);
            for (int i = 0; i < nf && (size_t)i < F.mvpMapPoints.size(); ++i)
                if (F.mvpMapPoints[i]) occ[c][i] = 0;
            pal[c] = already[c].data();
            pocc[c] = occ[c].data();
            pout[c] = out[c].data();
        }
        std::vector<int32_t> nm(C > 0 ? C : 1, 0);
        check(rsc_search_by_projection_many(thread_context(), hf.data(), hk.data(), C, T.data(), pal.data(),
                                            pocc.data(), th, ORBdist, mbCheckOrientation ? 1 : 0, pout.data(),
                                            nm.data(), nullptr),
              "SearchByProjection(Frame, KeyFrame)");
        for (int c = 0; c < C; ++c) {  // CurrentFrame.mvpMapPoints[bestIdx2] = pMP (:1402)
            FrameT& F = *frames[c];
            const std::vector<MPPtr>& m = mps[ki[c]];
            for (int i = 0; i < fviews[fi[c]].n && (size_t)i < F.mvpMapPoints.size(); ++i)
                if (out[c][i] >= 0) F.mvpMapPoints[i] = m[out[c][i]];
        }
        return std::vector<int>(nm.begin(), nm.begin() + C);
    }

    // SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (ORBmatcher.cpp:241-352; LoopClosing.cpp:360):
    // the points that are not bad and not already in vpMatched are projected with Scw (an Isometry3f:
    // rotation() / translation(), used as they are) and matched to the keypoints of pKF whose vpMatched slot
    // is empty; the new matches are written to vpMatched, returns their number.
    template <class KFPtr, class IsoT, class MPPtr>
    int SearchByProjection(KFPtr pKF, const IsoT& Scw, const std::vector<MPPtr>& vpPoints,
                           std::vector<MPPtr>& vpMatched, int th) {
        LoopMapPoints<MPPtr> pts(vpPoints);
        std::vector<KFPtr> k(1, pKF);
        std::vector<IsoT> s(1, Scw);
        std::vector<const LoopMapPoints<MPPtr>*> p(1, &pts);
        std::vector<std::vector<MPPtr>*> m(1, &vpMatched);
        return SearchByProjectionMany(k, s, p, m, th)[0];
    }

    // SearchByProjection(vpKFs[c], Scw[c], *points[c], *vpMatched[c], th) for several problems in one launch
    // over prepared point views.  Each KeyFrame object is uploaded once.
    template <class KFPtr, class IsoT, class MPPtr>
    std::vector<int> SearchByProjectionMany(const std::vector<KFPtr>& vpKFs, const std::vector<IsoT>& Scw,
                                            const std::vector<const LoopMapPoints<MPPtr>*>& points,
                                            const std::vector<std::vector<MPPtr>*>& vpMatched, int th) {
        const int C = (int)vpKFs.size();
        std::vector<detail::KFViewUpload> views;
        std::vector<int> ki;
        upload_distinct(vpKFs, views, ki);
        std::vector<rsc_kfview*> hk(C);
        std::vector<rsc_mpview*> hp(C);
        std::vector<float> T(16 * (size_t)(C > 0 ? C : 1), 0.f);
        std::vector<std::vector<uint8_t>> already(C), occ(C);
        std::vector<std::vector<int32_t>> out(C);
        std::vector<const uint8_t*> pal(C), pocc(C);
        std::vector<int32_t*> pout(C);
        for (int c = 0; c < C; ++c) {
            hk[c] = views[ki[c]].h;
            hp[c] = points[c]->handle();
            iso_to_array(Scw[c], &T[16 * (size_t)c]);
            const std::vector<MPPtr>& pts = points[c]->points();
            const std::vector<MPPtr>& m = *vpMatched[c];
            std::set<MPPtr> found(m.begin(), m.end());  // spAlreadyFound (:255-256)
            found.erase(nullptr);
            const int nk = views[ki[c]].n;
            already[c].assign(pts.size() > 0 ? pts.size() : 1, 0);
            for (size_t i = 0; i < pts.size(); ++i) already[c][i] = found.count(pts[i]) ? 1 : 0;
            occ[c].assign((size_t)(nk > 0 ? nk : 1), 0);
            for (int i = 0; i < nk && (size_t)i < m.size(); ++i) occ[c][i] = m[i] ? 1 : 0;
            out[c].assign((size_t)(nk > 0 ? nk : 1), -1);
            pal[c] = already[c].data();
            pocc[c] = occ[c].data();
            pout[c] = out[c].data();
        }
        std::vector<int32_t> nm(C > 0 ? C : 1, 0);
        check(rsc_search_by_projection_kf_many(thread_context(), hk.data(), hp.data(), C, T.data(), pal.data(),
                                               pocc.data(), th, pout.data(), nm.data(), nullptr),
              "SearchByProjection(KeyFrame, Scw, vpPoints)");
        for (int c = 0; c < C; ++c) {  // vpMatched[bestIdx] = pMP (:345)
            std::vector<MPPtr>& m = *vpMatched[c];
            const std::vector<MPPtr>& pts = points[c]->points();
            for (int i = 0; i < views[ki[c]].n && (size_t)i < m.size(); ++i)
                if (out[c][i] >= 0) m[i] = pts[out[c][i]];
        }
        return std::vector<int>(nm.begin(), nm.begin() + C);
    }

    // Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (ORBmatcher.cpp:823-946; LoopClosing.cpp:593): Scw carries
    // s * R in rotation().  KeyFrame additionally needs GetMapPoints(), GetMapPoint(idx) and
    // AddMapPoint(pMP, idx); MapPoint AddObservation(pKF, idx).
    template <class KFPtr, class IsoT, class MPPtr>
    int Fuse(KFPtr pKF, const IsoT& Scw, const std::vector<MPPtr>& vpPoints, float th,
             std::vector<MPPtr>& vpReplacePoint) {
        LoopMapPoints<MPPtr> pts(vpPoints);
        std::vector<KFPtr> k(1, pKF);
        std::vector<IsoT> s(1, Scw);
        std::vector<std::vector<MPPtr>*> r(1, &vpReplacePoint);
        return FuseMany(k, s, pts, th, r)[0];
    }

    // Fuse(vpKFs[c], Scw[c], points, th, *vpReplacePoints[c]) for every corrected KeyFrame of
    // LoopClosing::SearchAndFuse (:578-600) in one launch against one prepared point view.  Fuse's points
    // are independent of each other, so the device projects every (point, KeyFrame) pair at once and the
    // bookkeeping of :930-940 runs afterwards, KeyFrame by KeyFrame in the reference's order.  What the
    // reference reads from the map between two Fuse calls is read at that moment here too: after_kf(c) is
    // called when KeyFrame c is done (SearchAndFuse runs its pRep->Replace loop there), and the bookkeeping
    // of the next KeyFrame tests spAlreadyFound (:851) against its GetMapPoints() as they are then and reads
    // GetMapPoint(bestIdx) then.  A point that a Replace put into a later KeyFrame is therefore skipped for
    // it, as in the reference; the return values count what the bookkeeping kept.  Not re-read: isBad() of
    // the loop points (Replace never changes it for them).
    template <class KFPtr, class IsoT, class MPPtr>
    std::vector<int> FuseMany(const std::vector<KFPtr>& vpKFs, const std::vector<IsoT>& Scw,
                              const LoopMapPoints<MPPtr>& points, float th,
                              const std::vector<std::vector<MPPtr>*>& vpReplacePoints) {
        return FuseMany(vpKFs, Scw, points, th, vpReplacePoints, [](int) {});
    }

    template <class KFPtr, class IsoT, class MPPtr, class AfterKF>
    std::vector<int> FuseMany(const std::vector<KFPtr>& vpKFs, const std::vector<IsoT>& Scw,
                              const LoopMapPoints<MPPtr>& points, float th,
                              const std::vector<std::vector<MPPtr>*>& vpReplacePoints, AfterKF after_kf) {
        const int C = (int)vpKFs.size();
        std::vector<detail::KFViewUpload> views;
        std::vector<int> ki;
        upload_distinct(vpKFs, views, ki);
        const std::vector<MPPtr>& pts = points.points();
        const size_t np = pts.size();
        std::vector<rsc_kfview*> hk(C);
        std::vector<float> T(16 * (size_t)(C > 0 ? C : 1), 0.f);
        std::vector<std::vector<uint8_t>> in_kf(C);
        std::vector<std::vector<int32_t>> best(C);
        std::vector<const uint8_t*> pin(C);
        std::vector<int32_t*> pbest(C);
        for (int c = 0; c < C; ++c) {
            hk[c] = views[ki[c]].h;
            iso_to_array(Scw[c], &T[16 * (size_t)c]);
            const auto found = vpKFs[c]->GetMapPoints();  // spAlreadyFound (:839)
            in_kf[c].assign(np > 0 ? np : 1, 0);
            for (size_t i = 0; i < np; ++i) in_kf[c][i] = found.count(pts[i]) ? 1 : 0;
            best[c].assign(np > 0 ? np : 1, -1);
            pin[c] = in_kf[c].data();
            pbest[c] = best[c].data();
        }
        std::vector<int32_t> nf(C > 0 ? C : 1, 0);
        check(rsc_fuse_sim3_many(thread_context(), hk.data(), C, points.handle(), T.data(), pin.data(), th,
                                 pbest.data(), nf.data()),
              "Fuse(KeyFrame, Scw, vpPoints)");
        for (int c = 0; c < C; ++c) {
            std::vector<MPPtr>& rep = *vpReplacePoints[c];
            const auto found = vpKFs[c]->GetMapPoints();  // spAlreadyFound as it is now (:839)
            int kept = 0;
            for (size_t i = 0; i < np; ++i) {
                const int idx = best[c][i];
                if (idx < 0) continue;
                if (!in_kf[c][i] && found.count(pts[i])) continue;  // joined the KeyFrame since the launch (:851)
                ++kept;
                MPPtr pMPinKF = vpKFs[c]->GetMapPoint(idx);  // :930
                if (pMPinKF) {
                    if (!pMPinKF->isBad() && i < rep.size()) rep[i] = pMPinKF;  // :933-934
                } else {
                    pts[i]->AddObservation(vpKFs[c], idx);  // :938-939
                    vpKFs[c]->AddMapPoint(pts[i], idx);
                }
            }
            nf[c] = kept;
            after_kf(c);
        }
        return std::vector<int>(nf.begin(), nf.begin() + C);
    }

    // Fuse(pKF, vpMapPoints, th) (ORBmatcher.cpp:671-821; LocalMapping.cpp:465 and :490).  vpMapPoints may hold
    // null and repeated pointers (GetMapPointMatches() has both kinds).  KeyFrame additionally needs
    // mvInvLevelSigma2, GetMapPoint(idx), AddMapPoint(pMP, idx) and what set_triangulation reads; MapPoint
    // IsInKeyFrame(pKF), Observations(), Replace(pMP), AddObservation(pKF, idx) and GetNormal().
    template <class KFPtr, class MPPtr>
    int Fuse(KFPtr pKF, const std::vector<MPPtr>& vpMapPoints, float th = 3.0f) {
        std::vector<KFPtr> k(1, pKF);
        return FuseMany(k, vpMapPoints, th)[0];
    }

    // The loop of LocalMapping::SearchInNeighbors over its target KeyFrames (LocalMapping.cpp:461-466),
    //     for (pKFi : vpTargetKFs) matcher.Fuse(pKFi, vpMapPointMatches);
    // with the matcher of every (point, KeyFrame) pair in one launch (rsc_fuse_kf_many) and the bookkeeping
    // of :690-695 and :797-817 replayed on the caller's objects, KeyFrame by KeyFrame and i ascending: isBad()
    // and IsInKeyFrame(pKF) are read again at that moment, then GetMapPoint(bestIdx), Observations(), Replace in
    // either direction (a tie takes the else branch) or AddObservation / AddMapPoint, and nFused counts as the
    // reference does (a bad occupant counts).  The backward call (:490) is Fuse() after this one returned.
    //
    // Why launching every pair from the state at the call is exact (MapPoint.cpp:76-87, :158-197):
    // (a) During SearchInNeighbors a good point only gains observations (AddObservation here and in Replace;
    //     EraseObservation is not called) and a bad point stays bad (mbBad is only ever set).  So the set of
    //     pairs that pass :695 only shrinks: a pair skipped at launch is skipped by the reference too, and a
    //     pair that became ineligible since is dropped by the replay's own test.
    // (b) Of what the matcher reads from a MapPoint (position, normal, min / max distance, descriptor) only the
    //     descriptor can change between two Fuse calls: Replace ends with ComputeDistinctiveDescriptors() on
    //     the survivor; the others change in UpdateNormalAndDepth, which SearchInNeighbors calls after both
    //     directions (:493-506).  The uploaded descriptor bytes are kept; after every Replace the survivor's
    //     GetDescriptor() is compared with them when the survivor is in the list, and once KeyFrame c is
    //     replayed the changed points are matched again (a second small launch) against KeyFrames c + 1 ..
    //     only, and their bestIdx patched.  Inside one Fuse call nothing is stale: the survivor is either pMP,
    //     whose list position is behind the loop (and a repeated pointer to it is in pKF from now on), or
    //     pMPinKF, which is in pKF and skipped by :695 for the rest of the call.
    // The KeyFrames read nothing that Fuse changes (keypoints, pose, grid), so their views are uploaded once.
    // The step that follows both directions, ComputeDistinctiveDescriptors and UpdateNormalAndDepth on the current
    // KeyFrame's points (:493-506), is rsc_orb::UpdateMapPointsOf(pKF) of MapPoint.hpp.
    template <class KFPtr, class MPPtr>
    std::vector<int> FuseMany(const std::vector<KFPtr>& vpTargetKFs, const std::vector<MPPtr>& vpMapPoints,
                              float th = 3.0f) {
        const int C = (int)vpTargetKFs.size();
        std::vector<int> nFused(C, 0);
        if (C == 0) return nFused;
        // the list without its nulls (:692), in list order, which is the replay's order; repeated pointers stay
        std::vector<MPPtr> pts;
        for (size_t i = 0; i < vpMapPoints.size(); ++i)
            if (vpMapPoints[i]) pts.push_back(vpMapPoints[i]);
        const size_t np = pts.size();
        std::vector<detail::KFViewUpload> views;
        std::vector<int> ki;
        upload_distinct(vpTargetKFs, views, ki);
        {
            std::vector<char> done(views.size(), 0);
            for (int c = 0; c < C; ++c) {
                if (done[ki[c]]) continue;
                done[ki[c]] = 1;
                const auto& K = *vpTargetKFs[c];
                for (size_t l = 0; l < (size_t)K.mnScaleLevels; ++l) {  // ORBextractor.cpp:359,367
                    const float sf = K.mvScaleFactors[l], s2 = sf * sf, inv = 1.0f / s2;
                    if (l >= K.mvInvLevelSigma2.size() || !(K.mvInvLevelSigma2[l] == inv))
                        throw std::runtime_error("rsc: Fuse: mvInvLevelSigma2 is not 1.0f / (mvScaleFactors^2)");
                }
                detail::set_triangulation(views[ki[c]], vpTargetKFs[c]);
            }
        }
        detail::FusePoints up(np);
        for (size_t j = 0; j < np; ++j) up.set(j, *pts[j]);
        detail::MPViewUpload view = up.upload(np);
        std::vector<std::vector<int32_t>> best(C, std::vector<int32_t>(np > 0 ? np : 1, -1));
        fuse_kf_launch(vpTargetKFs, views, ki, 0, view.h, pts, th, best, nullptr);
        std::vector<size_t> changed;  // entries whose descriptor a Replace of this KeyFrame's replay changed
        auto survivor = [&](const MPPtr& s) {
            bool read = false;
            uint8_t now[32];
            for (size_t j = 0; j < np; ++j) {
                if (pts[j] != s) continue;
                if (!read) {
                    const auto d = s->GetDescriptor();
                    const uint8_t* dr = d.template ptr<uint8_t>(0);
                    std::copy(dr, dr + 32, now);
                    read = true;
                }
                if (std::equal(now, now + 32, up.desc.begin() + 32 * j)) continue;
                std::copy(now, now + 32, up.desc.begin() + 32 * j);
                if (std::find(changed.begin(), changed.end(), j) == changed.end()) changed.push_back(j);
            }
        };
        for (int c = 0; c < C; ++c) {
            const KFPtr& pKF = vpTargetKFs[c];
            for (size_t j = 0; j < np; ++j) {
                const MPPtr& pMP = pts[j];
                if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;  // :695, as it is now
                const int bestIdx = best[c][j];
                if (bestIdx < 0) continue;  // :798
                MPPtr pMPinKF = pKF->GetMapPoint(bestIdx);
                if (pMPinKF) {
                    if (!pMPinKF->isBad()) {
                        if (pMPinKF->Observations() > pMP->Observations()) {
                            pMP->Replace(pMPinKF);
                            survivor(pMPinKF);
                        } else {
                            pMPinKF->Replace(pMP);
                            survivor(pMP);
                        }
                    }
                } else {
                    pMP->AddObservation(pKF, bestIdx);
                    pKF->AddMapPoint(pMP, bestIdx);
                }
                ++nFused[c];
            }
            if (!changed.empty() && c + 1 < C) {  // (b): the changed points against the KeyFrames still to come
                std::sort(changed.begin(), changed.end());
                detail::FusePoints sub(changed.size());
                std::vector<MPPtr> spts;
                for (size_t k = 0; k < changed.size(); ++k) {
                    sub.copy(k, up, changed[k]);
                    sub.state[k] = pts[changed[k]]->isBad() ? 2 : 1;
                    spts.push_back(pts[changed[k]]);
                }
                detail::MPViewUpload sview = sub.upload(changed.size());
                fuse_kf_launch(vpTargetKFs, views, ki, c + 1, sview.h, spts, th, best, &changed);
            }
            changed.clear();
        }
        return nFused;
    }

    // SearchByProjection(F, vpMapPoints, th) (ORBmatcher.cpp:16-100; Tracking.cpp:1027): every MapPoint with
    // mbTrackInView that is not bad is matched around (mTrackProjX, mTrackProjY) at levels
    // [mnTrackScaleLevel - 1, mnTrackScaleLevel]; the matches are written to F.mvpMapPoints, returns their
    // number (a feature taken twice, by a point without observations and then by a later one, counts twice).
    template <class FrameT, class MPPtr>
    int SearchByProjection(FrameT& F, const std::vector<MPPtr>& vpMapPoints, const float th) {
        return local_points(F, vpMapPoints, th, mfNNratio, false, 0.f, nullptr);
    }

    // SearchByProjection(CurrentFrame, LastFrame, th) (ORBmatcher.cpp:1173-1315; Tracking.cpp:732,738): every
    // LastFrame slot with a MapPoint that is not an outlier is matched around its projection with
    // CurrentFrame.mTcw, at the levels of the call's mode (forward / backward / neither, from the two poses and
    // CurrentFrame.mb).  Writes CurrentFrame.mvpMapPoints, the nullptr of the rotation check included, and
    // returns the count (claims minus claims in removed rotation bins, as the reference counts).
    template <class FrameT>
    int SearchByProjection(FrameT& CurrentFrame, const FrameT& LastFrame, const float th) {
        detail::FrameViewUpload fv = detail::upload_frameview(CurrentFrame);
        check(rsc_frameview_set_stereo(fv.h, CurrentFrame.mvuRight.data(), CurrentFrame.mbf),
              "rsc_frameview_set_stereo");
        detail::LastFrameUpload lv = detail::upload_lastframe(LastFrame);
        const size_t nf = (size_t)fv.n;
        std::vector<uint8_t> occ(nf > 0 ? nf : 1, 0);
        for (size_t f = 0; f < nf && f < CurrentFrame.mvpMapPoints.size(); ++f)  // :1248-1250
            if (CurrentFrame.mvpMapPoints[f]) occ[f] = CurrentFrame.mvpMapPoints[f]->Observations() > 0 ? 2 : 1;
        std::vector<int32_t> out(nf > 0 ? nf : 1, -1);
        float Tc[16], Tl[16];
        iso_to_array(CurrentFrame.mTcw, Tc);
        iso_to_array(LastFrame.mTcw, Tl);
        const float mb = CurrentFrame.mb;
        rsc_frameview* hf = fv.h;
        rsc_lastframe* hl = lv.h;
        const uint8_t* pocc = occ.data();
        int32_t* pout = out.data();
        int32_t nm = 0;
        check(rsc_search_by_projection_last_many(thread_context(), &hf, &hl, 1, Tc, Tl, &mb, &pocc, th,
                                                 mbCheckOrientation ? 1 : 0, &pout, &nm, nullptr, nullptr),
              "SearchByProjection(CurrentFrame, LastFrame)");
        for (size_t f = 0; f < nf && f < CurrentFrame.mvpMapPoints.size(); ++f) {
            if (out[f] >= 0) CurrentFrame.mvpMapPoints[f] = LastFrame.mvpMapPoints[out[f]];  // :1273
            else if (out[f] == -2) CurrentFrame.mvpMapPoints[f] = nullptr;                   // :1307
        }
        return nm;
    }

    // Tracking::SearchLocalPoints from :1003 on (Tracking.cpp:1003-1028) in one device call: isInFrustum(pMP,
    // 0.5) over the points with mnLastFrameSeen != F.mnId that are not bad, the track members and
    // IncreaseVisible() on the MapPoints as the reference leaves them, then the matcher when nToMatch > 0.
    // The loop over F.mvpMapPoints before it (:982-998) stays with the caller.  Returns the matcher's count.
    template <class FrameT, class MPPtr>
    static int SearchLocalPoints(FrameT& F, const std::vector<MPPtr>& vpLocalMapPoints, float th, float nnratio,
                                 int* nToMatch = nullptr) {
        return local_points(F, vpLocalMapPoints, th, nnratio, true, 0.5f, nToMatch);
    }

private:
    template <class FrameT, class MPPtr>
    static int local_points(FrameT& F, const std::vector<MPPtr>& vpMapPoints, float th, float nnratio, bool fused,
                            float cos_limit, int* nToMatch) {
        LoopMapPoints<MPPtr> view(vpMapPoints);  // state 2 = isBad() (:28 / Tracking.cpp:1008)
        detail::FrameViewUpload fv = detail::upload_frameview(F);
        check(rsc_frameview_set_stereo(fv.h, F.mvuRight.data(), F.mbf), "rsc_frameview_set_stereo");
        const size_t np = vpMapPoints.size(), nf = (size_t)fv.n;
        std::vector<uint8_t> skip(np > 0 ? np : 1, 0), has_obs(np > 0 ? np : 1, 0), occ(nf > 0 ? nf : 1, 0);
        std::vector<rsc_track_record> track(np > 0 ? np : 1);
        for (size_t i = 0; i < np; ++i) {
            auto& mp = *vpMapPoints[i];
            has_obs[i] = mp.Observations() > 0 ? 1 : 0;
            if (fused) {
                skip[i] = mp.mnLastFrameSeen == F.mnId ? 1 : 0;  // Tracking.cpp:1006
                track[i] = rsc_track_record{0, 0.f, 0.f, 0.f, 0, 0.f};
            } else {
                track[i] = rsc_track_record{mp.mbTrackInView ? 1 : 0, mp.mTrackProjX, mp.mTrackProjY, mp.mTrackProjXR,
                                            (int32_t)mp.mnTrackScaleLevel, mp.mTrackViewCos};
            }
        }
        for (size_t f = 0; f < nf && f < F.mvpMapPoints.size(); ++f)  // :58-60
            if (F.mvpMapPoints[f]) occ[f] = F.mvpMapPoints[f]->Observations() > 0 ? 2 : 1;
        std::vector<int32_t> out(nf > 0 ? nf : 1, -1);
        float T[16];
        if (fused) iso_to_array(F.mTcw, T);
        rsc_frameview* hf = fv.h;
        rsc_mpview* hp = view.handle();
        const uint8_t* pskip = skip.data();
        const uint8_t* pobs = has_obs.data();
        const uint8_t* pocc = occ.data();
        int32_t* pout = out.data();
        rsc_track_record* ptr = track.data();
        const rsc_track_record* cptr = track.data();
        int32_t nm = 0, ntm = 0;
        if (fused)
            check(rsc_search_local_points_many(thread_context(), &hf, &hp, 1, T, &pskip, &pobs, &pocc, cos_limit, th,
                                               nnratio, &pout, &ptr, &nm, &ntm, nullptr),
                  "SearchLocalPoints");
        else
            check(rsc_search_by_projection_points_many(thread_context(), &hf, &hp, 1, &pskip, &pobs, &pocc, th, nnratio,
                                                       &pout, &cptr, &nm, &ntm, nullptr),
                  "SearchByProjection(Frame, vpMapPoints)");
        if (fused)
            for (size_t i = 0; i < np; ++i) {
                auto& mp = *vpMapPoints[i];
                if (skip[i] || mp.isBad()) continue;       // Tracking.cpp:1006-1009: isInFrustum did not run
                mp.mbTrackInView = track[i].in_view != 0;  // Frame.cpp:338 / :384
                if (!track[i].in_view) continue;
                mp.mTrackProjX = track[i].proj_x;
                mp.mTrackProjXR = track[i].proj_xr;
                mp.mTrackProjY = track[i].proj_y;
                mp.mnTrackScaleLevel = track[i].level;
                mp.mTrackViewCos = track[i].view_cos;
                mp.IncreaseVisible();                      // Tracking.cpp:1013
            }
        for (size_t f = 0; f < nf && f < F.mvpMapPoints.size(); ++f)  // F.mvpMapPoints[bestIdx] = pMP (:94)
            if (out[f] >= 0) F.mvpMapPoints[f] = vpMapPoints[out[f]];
        if (nToMatch) *nToMatch = ntm;
        return nm;
    }

    // one upload per distinct KeyFrame object; ki[c] = its view
    template <class KFPtr>
    static void upload_distinct(const std::vector<KFPtr>& vpKFs, std::vector<detail::KFViewUpload>& views,
                                std::vector<int>& ki) {
        detail::upload_distinct(vpKFs, views, ki);
    }

    // rsc_fuse_kf_many for KeyFrames c0 .. against the points of `view` (pts: its MapPoints), skip as it is now.
    // The results go to best[c][j] or, with `at`, to best[c][(*at)[j]].
    template <class KFPtr, class MPPtr>
    static void fuse_kf_launch(const std::vector<KFPtr>& kfs, const std::vector<detail::KFViewUpload>& views,
                               const std::vector<int>& ki, int c0, rsc_mpview* view, const std::vector<MPPtr>& pts,
                               float th, std::vector<std::vector<int32_t>>& best, const std::vector<size_t>* at) {
        const int C = (int)kfs.size() - c0;
        const size_t np = pts.size();
        std::vector<rsc_kfview*> hk(C);
        std::vector<rsc_mpview*> hp(C, view);
        std::vector<std::vector<uint8_t>> skip(C, std::vector<uint8_t>(np > 0 ? np : 1, 0));
        std::vector<std::vector<int32_t>> out(C, std::vector<int32_t>(np > 0 ? np : 1, -1));
        std::vector<const uint8_t*> ps(C);
        std::vector<int32_t*> po(C);
        for (int c = 0; c < C; ++c) {
            hk[c] = views[ki[c0 + c]].h;
            for (size_t j = 0; j < np; ++j) skip[c][j] = pts[j]->isBad() || pts[j]->IsInKeyFrame(kfs[c0 + c]) ? 1 : 0;
            ps[c] = skip[c].data();
            po[c] = out[c].data();
        }
        check(rsc_fuse_kf_many(thread_context(), hk.data(), hp.data(), C, ps.data(), th, po.data(), nullptr),
              "Fuse(KeyFrame, vpMapPoints)");
        for (int c = 0; c < C; ++c)
            for (size_t j = 0; j < np; ++j) best[c0 + c][at ? (*at)[j] : j] = out[c][j];
    }

    template <class IsoT>
    static void iso_to_array(const IsoT& S, float* T) {
        detail::iso_to_array16(S, T);
    }

    float mfNNratio;
    bool mbCheckOrientation;
};

// Tracking::SearchLocalPoints from :1003 on (ORBmatcher::SearchLocalPoints above); the reference calls the
// matcher with ORBmatcher(0.8) and th = 1, 3 (RGB-D) or 5 (just relocalised).
template <class FrameT, class MPPtr>
int SearchLocalPoints(FrameT& F, const std::vector<MPPtr>& vpLocalMapPoints, float th, float nnratio = 0.8f,
                      int* nToMatch = nullptr) {
    return ORBmatcher::SearchLocalPoints(F, vpLocalMapPoints, th, nnratio, nToMatch);
}

// Tracking::TrackWithMotionModel from :724 to its return value (Tracking.cpp:724-774) in one device call:
// mvpMapPoints cleared, SearchByProjection(CurrentFrame, LastFrame, th) with ORBmatcher(0.9, true), the retry at
// 2 * th when fewer than 20 matched, Optimizer::PoseOptimization, and the discard loop.  The caller has run
// UpdateLastFrame() (:720) and CurrentFrame.SetPose(mVelocity * LastFrame.mTcw) (:722).  Writes
// CurrentFrame.mvpMapPoints, mvbOutlier and the pose (SetPose), and mbTrackInView = false / mnLastFrameSeen =
// CurrentFrame.mnId on the MapPoints discarded as outliers.  bVO receives mbVO when bOnlyTracking is set and the
// optimisation ran (:770); returns the function's value.  FrameT additionally needs mb, mnId, mvbOutlier,
// mTcw(r, c) and SetPose as rsc_orb::PoseOptimization does.
template <class FrameT>
bool TrackWithMotionModel(FrameT& CurrentFrame, const FrameT& LastFrame, int th, bool bOnlyTracking,
                          bool* bVO = nullptr, rsc_track_motion_result* record = nullptr) {
    detail::FrameViewUpload fv = detail::upload_frameview(CurrentFrame);
    check(rsc_frameview_set_stereo(fv.h, CurrentFrame.mvuRight.data(), CurrentFrame.mbf), "rsc_frameview_set_stereo");
    detail::LastFrameUpload lv = detail::upload_lastframe(LastFrame);
    const size_t nf = (size_t)fv.n;
    std::vector<int32_t> out(nf > 0 ? nf : 1, -1), disc(nf > 0 ? nf : 1, -1);
    float Tc[16], Tl[16];
    detail::iso_to_array16(CurrentFrame.mTcw, Tc);
    detail::iso_to_array16(LastFrame.mTcw, Tl);
    const float mb = CurrentFrame.mb;
    const int32_t only = bOnlyTracking ? 1 : 0;
    rsc_frameview* hf = fv.h;
    rsc_lastframe* hl = lv.h;
    int32_t* pout = out.data();
    int32_t* pdisc = disc.data();
    rsc_track_motion_result r;
    check(rsc_track_motion_model_many(thread_context(), &hf, &hl, 1, Tc, Tl, &mb, (float)th, &only, &r, &pout, &pdisc),
          "TrackWithMotionModel");
    CurrentFrame.mvpMapPoints.assign(CurrentFrame.mvpMapPoints.size(), nullptr);  // :724
    if (CurrentFrame.mvbOutlier.size() < nf) CurrentFrame.mvbOutlier.resize(nf, false);
    for (size_t f = 0; f < nf && f < CurrentFrame.mvpMapPoints.size(); ++f) {
        if (out[f] >= 0) {
            CurrentFrame.mvpMapPoints[f] = LastFrame.mvpMapPoints[out[f]];
            if (r.nmatches_search[r.searches - 1] >= 20) CurrentFrame.mvbOutlier[f] = false;  // Optimizer.cpp:255
        } else if (disc[f] >= 0) {  // :753-761
            auto& mp = *LastFrame.mvpMapPoints[disc[f]];
            CurrentFrame.mvbOutlier[f] = false;
            mp.mbTrackInView = false;
            mp.mnLastFrameSeen = CurrentFrame.mnId;
        }
    }
    if (r.nmatches_search[r.searches - 1] >= 20) {  // PoseOptimization ran: pFrame->SetPose (Optimizer.cpp:420-421)
        auto T = CurrentFrame.mTcw;
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) T(a, b) = r.Tcw[4 * a + b];
        CurrentFrame.SetPose(T);
        if (bOnlyTracking && bVO) *bVO = r.vo != 0;  // :770
    }
    if (record) *record = r;
    return r.ok != 0;
}

}  // namespace rsc_orb
