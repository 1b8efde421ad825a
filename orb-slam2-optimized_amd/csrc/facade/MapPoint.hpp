// MapPoint.hpp — MapPoint::ComputeDistinctiveDescriptors() and MapPoint::UpdateNormalAndDepth()
// (src/MapPoint.cpp:224-289, :312-353) for a batch of the caller's MapPoints in one device call
// (rsc_update_map_points_many), header-only and templated on the caller's types like the other facades.
//
//     rsc_orb::UpdateMapPoints(vpMapPoints, what = 3)   what: 1 descriptor | 2 normal and depth
//     rsc_orb::UpdateMapPointsOf(pKF)                   the loop of LocalMapping.cpp:493-506
//
// What it reads of a MapPoint: isBad(), GetWorldPos(), GetObservations() (the std::map, iterated in map order,
// which is the reference's own iteration order) and GetReferenceKeyFrame(); of a KeyFrame: isBad() and what
// upload_kfview / set_triangulation of ORBmatcher.hpp read.  Null pointers are skipped and a repeated pointer is
// taken once, the first time (the two functions are idempotent on unchanged inputs).  Every distinct KeyFrame is
// uploaded once.  When the reference KeyFrame is not among the observations the reference's observations[pRefKF]
// on its local copy yields index 0, and so does this.
//
// The reference's members are protected, so the results arrive through two members the integrator adds to
// MapPoint, whose bodies are the reference's own lock blocks (:285-288, :347-352):
//     void SetDistinctiveDescriptor(const uint8_t* d);     // mDescriptor = the 32 bytes, under mMutexFeatures
//     void SetNormalAndDepth(const float normal[3], float minDist, float maxDist);  // under mMutexPos
// A list may hold at most RSC_MPUPDATE_MAX_OBS observations (include/rsc.h), a limit the reference does not have.
#pragma once
#include <cstdint>
#include <map>
#include <vector>
#include "ORBmatcher.hpp"

namespace rsc_orb {

// Returns the number of points that were updated (not null, not repeated, not bad, with observations).
template <class MPPtr>
int UpdateMapPoints(const std::vector<MPPtr>& vpMapPoints, int what = 3) {
    std::vector<MPPtr> pts;
    {
        std::map<const void*, int> seen;
        for (const auto& p : vpMapPoints)
            if (p && seen.emplace((const void*)&*p, 0).second) pts.push_back(p);
    }
    const size_t np = pts.size();
    if (np == 0) return 0;
    using KFPtr = decltype(pts[0]->GetReferenceKeyFrame());
    std::vector<KFPtr> kfs;
    std::map<const void*, int> kf_at;
    auto kf_index = [&](const KFPtr& k) {
        const auto r = kf_at.emplace((const void*)&*k, (int)kfs.size());
        if (r.second) kfs.push_back(k);
        return r.first->second;
    };
    std::vector<uint8_t> skip(np, 0);
    std::vector<float> pos(3 * np, 0.f);
    std::vector<int32_t> begin(np + 1, 0), okf, oidx, rkf(np, 0), ridx(np, 0);
    for (size_t p = 0; p < np; ++p) {
        begin[p + 1] = begin[p];
        auto& mp = *pts[p];
        if (mp.isBad()) {  // :233, :320
            skip[p] = 1;
            continue;
        }
        const auto X = mp.GetWorldPos();
        for (int c = 0; c < 3; ++c) pos[3 * p + c] = X(c);
        const auto observations = mp.GetObservations();
        for (const auto& o : observations) {
            okf.push_back(kf_index(o.first));
            oidx.push_back((int32_t)o.second);
        }
        begin[p + 1] = (int32_t)okf.size();
        if (observations.empty() || !(what & 2)) continue;
        const KFPtr ref = mp.GetReferenceKeyFrame();
        if (!ref) throw std::runtime_error("rsc: UpdateMapPoints: a MapPoint without a reference KeyFrame");
        rkf[p] = kf_index(ref);
        const auto it = observations.find(ref);
        ridx[p] = it != observations.end() ? (int32_t)it->second : 0;  // observations[pRefKF] (:343)
    }
    std::vector<detail::KFViewUpload> views;
    std::vector<int> ki;
    detail::upload_distinct(kfs, views, ki);
    std::vector<rsc_kfview*> hk(kfs.size() ? kfs.size() : 1, nullptr);
    std::vector<uint8_t> kf_bad(kfs.size() ? kfs.size() : 1, 0);
    for (size_t k = 0; k < kfs.size(); ++k) {
        if (what & 2) detail::set_triangulation(views[ki[k]], kfs[k]);  // Ow
        hk[k] = views[ki[k]].h;
        kf_bad[k] = kfs[k]->isBad() ? 1 : 0;  // :247
    }
    if (okf.empty()) {
        okf.push_back(0);
        oidx.push_back(0);
    }
    rsc_mappoint_updates in;
    in.n_points = (int32_t)np;
    in.skip = skip.data();
    in.pos = pos.data();
    in.obs_begin = begin.data();
    in.obs_kf = okf.data();
    in.obs_idx = oidx.data();
    in.kf_bad = kf_bad.data();
    in.ref_kf = rkf.data();
    in.ref_idx = ridx.data();
    std::vector<uint8_t> desc(32 * np), updated(np, 0);
    std::vector<int32_t> best(np, -1);
    std::vector<float> normal(3 * np), dmax(np), dmin(np);
    rsc_mappoint_update_out out;
    out.desc = desc.data();
    out.best_obs = best.data();
    out.normal = normal.data();
    out.dmax = dmax.data();
    out.dmin = dmin.data();
    out.updated = updated.data();
    check(rsc_update_map_points_many(thread_context(), hk.data(), (int)kfs.size(), &in, what, &out, nullptr, nullptr),
          "UpdateMapPoints");
    int n = 0;
    for (size_t p = 0; p < np; ++p) {
        if (updated[p] & 1) pts[p]->SetDistinctiveDescriptor(desc.data() + 32 * p);         // :285-288
        if (updated[p] & 2) pts[p]->SetNormalAndDepth(&normal[3 * p], dmin[p], dmax[p]);    // :347-352
        n += updated[p] != 0;
    }
    return n;
}

// The facade's context is the calling thread's (rsc_context.hpp); a context passed in must be that one.
template <class MPPtr>
int UpdateMapPoints(rsc_context* ctx, const std::vector<MPPtr>& vpMapPoints, int what = 3) {
    if (ctx != thread_context()) throw std::runtime_error("rsc: UpdateMapPoints: not the calling thread's context");
    return UpdateMapPoints(vpMapPoints, what);
}

// The update loop of LocalMapping::SearchInNeighbors (LocalMapping.cpp:493-506) over pKF->GetMapPointMatches(),
// the step after ORBmatcher::FuseMany and the backward Fuse.
template <class KFPtr>
int UpdateMapPointsOf(const KFPtr& pKF) {
    return UpdateMapPoints(pKF->GetMapPointMatches(), 3);
}

template <class KFPtr>
int UpdateMapPointsOf(rsc_context* ctx, const KFPtr& pKF) {
    return UpdateMapPoints(ctx, pKF->GetMapPointMatches(), 3);
}

}  // namespace rsc_orb
