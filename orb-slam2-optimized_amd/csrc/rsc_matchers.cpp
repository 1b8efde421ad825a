// rsc_matchers.cpp — the batched matcher entry points of the C ABI: everything that stages through
// arena_run (rsc_host.h, rsc_arena.h), and SearchByBoW.
#include <cmath>
#include <cstring>
#include "rsc_host.h"
#include "rsc_fusekf.h"

extern "C" {

// ---- ORBmatcher::SearchByBoW (src/ORBmatcher.cpp:110-240, :354-488) ----
namespace {
// pairs[c] = (outer[c], inner[c]); out rows of out_n[c] int32 each
int bow_search(rsc_context* C, bool frame_overload, const rsc_bow* const* outer, const rsc_bow* const* inner,
               int count, float nnratio, int check_ori, int32_t* const* out, int32_t* nmatches) {
    std::vector<size_t> ooff(count + 1, 0), roff(count + 1, 0), joff(count + 1, 0), toff(count + 1, 0);
    for (int c = 0; c < count; ++c) {
        if (!outer[c] || !inner[c] || outer[c]->ctx != C || inner[c]->ctx != C) return RSC_ERR_ARG;
        const int on = frame_overload ? inner[c]->n : outer[c]->n;
        if (on && !out[c]) return RSC_ERR_ARG;
        ooff[c + 1] = ooff[c] + al256(4 * (size_t)on);
        roff[c + 1] = roff[c] + (size_t)outer[c]->n_feat * kBowMaxSegs;
        joff[c + 1] = joff[c] + (size_t)outer[c]->n_nodes;
        toff[c + 1] = toff[c] + ((size_t)outer[c]->n_nodes + (size_t)outer[c]->n_feat / 64 + 1) * kBowMaxSegs;
    }
    const size_t o_pairs = 0, o_cnt = al256(sizeof(BowPair) * count), o_out = o_cnt + al256(4 * (size_t)count);
    const size_t o_rec = o_out + ooff[count], o_nodes = o_rec + al256(16 * roff[count]);
    const size_t o_tasks = o_nodes + al256(16 * joff[count]), o_nt = o_tasks + al256(16 * toff[count]);
    const size_t o_mcp = o_nt + al256(8 * (size_t)count);
    const size_t bytes = o_mcp + al256(2 * roff[count] / kBowMaxSegs);
    const size_t back = o_rec;  // counts + outputs come back
    RSC_HIP(hipSetDevice(C->device));
    if (int e = C->d_bow.ensure(bytes)) return e;
    if (int e = C->h_bow.ensure(back)) return e;
    RSC_HIP(hipStreamSynchronize(C->stream));  // the pinned mirror is free again
    char* d = C->d_bow.p;
    BowPair* hp = reinterpret_cast<BowPair*>(C->h_bow.p + o_pairs);
    for (int c = 0; c < count; ++c) {
        hp[c].outer = outer[c]->hdr;
        hp[c].inner = inner[c]->hdr;  // by value
        hp[c].rec = reinterpret_cast<uint4*>(d + o_rec) + roff[c];
        hp[c].nodes = reinterpret_cast<int4*>(d + o_nodes) + joff[c];
        hp[c].tasks = reinterpret_cast<int4*>(d + o_tasks) + toff[c];
        hp[c].ntasks = reinterpret_cast<int32_t*>(d + o_nt) + 2 * c;
        hp[c].mcp = reinterpret_cast<int16_t*>(d + o_mcp) + roff[c] / kBowMaxSegs;
        hp[c].out = reinterpret_cast<int32_t*>(d + o_out + ooff[c]);
        hp[c].nmatches = reinterpret_cast<int32_t*>(d + o_cnt) + c;
    }
    RSC_HIP(hipMemcpyAsync(d, C->h_bow.p, o_cnt, hipMemcpyHostToDevice, C->stream));
    RSC_HIP(timed_launch(C, [&] {
        int max_nodes = 0;
        for (int c = 0; c < count; ++c) max_nodes = std::max(max_nodes, outer[c]->n_nodes);
        return launch_bow_search(frame_overload, count, max_nodes, reinterpret_cast<const BowPair*>(d + o_pairs),
                                 nnratio, check_ori ? 1 : 0, C->stream);
    }));
    RSC_HIP(hipMemcpyAsync(C->h_bow.p + o_cnt, d + o_cnt, back - o_cnt, hipMemcpyDeviceToHost, C->stream));
    RSC_HIP(hipStreamSynchronize(C->stream));
    timing_read(C);
    const int32_t* hc = reinterpret_cast<const int32_t*>(C->h_bow.p + o_cnt);
    for (int c = 0; c < count; ++c) {
        const int on = frame_overload ? inner[c]->n : outer[c]->n;
        if (on) std::memcpy(out[c], C->h_bow.p + o_out + ooff[c], 4 * (size_t)on);
        if (nmatches) nmatches[c] = hc[c];
    }
    return RSC_OK;
}
}  // namespace

int rsc_search_by_bow_frame_many(rsc_context* C, rsc_bow* const* kfs, int count, const rsc_bow* frame, float nnratio,
                                 int check_orientation, int32_t* const* matches, int32_t* nmatches) {
    if (!C || count < 0 || (count && (!kfs || !frame || !matches))) return RSC_ERR_ARG;
    if (count == 0) return RSC_OK;
    std::vector<const rsc_bow*> inner((size_t)count, frame);
    return bow_search(C, true, kfs, inner.data(), count, nnratio, check_orientation, matches, nmatches);
}

int rsc_search_by_bow_kf_many(rsc_context* C, const rsc_bow* kf1, rsc_bow* const* kf2s, int count, float nnratio,
                              int check_orientation, int32_t* const* matches12, int32_t* nmatches) {
    if (!C || count < 0 || (count && (!kf1 || !kf2s || !matches12))) return RSC_ERR_ARG;
    if (count == 0) return RSC_OK;
    std::vector<const rsc_bow*> outer((size_t)count, kf1);
    return bow_search(C, false, outer.data(), kf2s, count, nnratio, check_orientation, matches12, nmatches);
}

int rsc_diag_bow_phase_stamps(rsc_context* C, uint64_t* out, int cap) {
    if (!C || !out || cap < 0) return RSC_ERR_ARG;
    RSC_HIP(hipStreamSynchronize(C->stream));
    RSC_HIP(read_bow_stamps(out, cap));
    return RSC_OK;
}

// ---- ORBmatcher::SearchBySim3 (src/ORBmatcher.cpp:948-1170) ----
int rsc_search_by_sim3_many(rsc_context* C, rsc_kfview* const* kf1, rsc_kfview* const* kf2, int count,
                            const float* R12, const float* t12, float th, const int32_t* const* matched12,
                            int32_t* const* out12, int32_t* nfound) {
    if (!C || count < 0 || (count && (!kf1 || !kf2 || !R12 || !t12 || !matched12 || !out12))) return RSC_ERR_ARG;
    C->s3m_last.clear();
    if (count == 0) return RSC_OK;
    if (!std::isfinite(th)) return RSC_ERR_ARG;
    int max_points = 0;
    for (int c = 0; c < count; ++c) {
        if (!kf1[c] || !kf2[c] || kf1[c]->ctx != C || kf2[c]->ctx != C) return RSC_ERR_ARG;
        for (const rsc_kfview* v : {kf1[c], kf2[c]})
            if (!grid_radius_ok(th, v->top_scale, v->dev.gw_inv, v->dev.gh_inv)) {
                g_last_error = "SearchBySim3 radius out of the grid arithmetic's range";
                return RSC_ERR_ARG;
            }
        if (kf1[c]->n && (!matched12[c] || !out12[c])) return RSC_ERR_ARG;
        max_points = std::max(max_points, std::max(kf1[c]->n, kf2[c]->n));
    }
    // layout: pair table | vbAlreadyMatched1/2 flags (host-derived, :972-984) | vnMatch1/2 scratch |
    // outputs (the only part that comes back)
    std::vector<size_t> o_a1(count), o_a2(count), o_m1(count), o_m2(count), o_out(count), o_nf(count);
    Arena A;
    A.take(sizeof(Sim3MatchPair) * count);
    for (int c = 0; c < count; ++c) {
        o_a1[c] = A.take((size_t)std::max(kf1[c]->n, 1));
        o_a2[c] = A.take((size_t)std::max(kf2[c]->n, 1));
    }
    A.end_upload();
    for (int c = 0; c < count; ++c) {
        o_m1[c] = A.take(4 * (size_t)std::max(kf1[c]->n, 1));
        o_m2[c] = A.take(4 * (size_t)std::max(kf2[c]->n, 1));
    }
    A.end_scratch();
    for (int c = 0; c < count; ++c) {
        o_out[c] = A.take(4 * (size_t)std::max(kf1[c]->n, 1));
        o_nf[c] = A.take_packed(4);
    }
    A.finish();
    auto fill = [&](char* h, char* d) -> int {
        for (int c = 0; c < count; ++c) {
            const int n1 = kf1[c]->n, n2 = kf2[c]->n;
            uint8_t* a1 = reinterpret_cast<uint8_t*>(h + o_a1[c]);
            uint8_t* a2 = reinterpret_cast<uint8_t*>(h + o_a2[c]);
            std::memset(a1, 0, (size_t)std::max(n1, 1));
            std::memset(a2, 0, (size_t)std::max(n2, 1));
            for (int i = 0; i < n1; ++i) {
                const int32_t m = matched12[c][i];
                if (m < -2 || m >= n2) return RSC_ERR_ARG;
                if (m == -1) continue;
                a1[i] = 1;
                if (m >= 0) a2[m] = 1;
            }
            Sim3MatchPair p;
            p.k1 = kf1[c]->hdr;
            p.k2 = kf2[c]->hdr;
            std::memcpy(p.R12, R12 + 9 * c, sizeof(p.R12));
            std::memcpy(p.t12, t12 + 3 * c, sizeof(p.t12));
            p.already1 = reinterpret_cast<const uint8_t*>(d + o_a1[c]);
            p.already2 = reinterpret_cast<const uint8_t*>(d + o_a2[c]);
            p.m1 = reinterpret_cast<int32_t*>(d + o_m1[c]);
            p.m2 = reinterpret_cast<int32_t*>(d + o_m2[c]);
            p.out = reinterpret_cast<int32_t*>(d + o_out[c]);
            p.nfound = reinterpret_cast<int32_t*>(d + o_nf[c]);
            std::memcpy(h + sizeof(Sim3MatchPair) * c, &p, sizeof(p));
        }
        return 0;
    };
    auto launch = [&](char* d) {
        return launch_search_by_sim3(count, max_points, reinterpret_cast<const Sim3MatchPair*>(d), th, C->stream);
    };
    if (int e = arena_run(C, C->d_s3m, C->h_s3m, A, fill, launch)) return e;
    const char* h = C->h_s3m.p;
    for (int c = 0; c < count; ++c) {
        if (kf1[c]->n) std::memcpy(out12[c], h + o_out[c], 4 * (size_t)kf1[c]->n);
        if (nfound) std::memcpy(&nfound[c], h + o_nf[c], 4);
    }
    C->s3m_last.resize((size_t)count);
    for (int c = 0; c < count; ++c) C->s3m_last[c] = {o_m1[c], o_m2[c], kf1[c]->n, kf2[c]->n};
    return RSC_OK;
}

int rsc_diag_sim3match_directions(rsc_context* C, int pair, int32_t* m1, int n1, int32_t* m2, int n2) {
    if (!C || pair < 0 || (size_t)pair >= C->s3m_last.size()) return RSC_ERR_ARG;
    const auto& p = C->s3m_last[(size_t)pair];
    if (n1 != p.n1 || n2 != p.n2 || (n1 && !m1) || (n2 && !m2)) return RSC_ERR_ARG;
    RSC_HIP(hipSetDevice(C->device));
    RSC_HIP(hipStreamSynchronize(C->stream));
    if (n1) RSC_HIP(hipMemcpy(m1, C->d_s3m.p + p.o_m1, 4 * (size_t)n1, hipMemcpyDeviceToHost));
    if (n2) RSC_HIP(hipMemcpy(m2, C->d_s3m.p + p.o_m2, 4 * (size_t)n2, hipMemcpyDeviceToHost));
    return RSC_OK;
}

// ---- ORBmatcher::SearchByProjection(Frame&, KeyFrame, sAlreadyFound, th, ORBdist) (rsc_frameproj.h) ----
int rsc_search_by_projection_many(rsc_context* C, rsc_frameview* const* frames, rsc_kfview* const* kfs, int count,
                                  const float* Tcw, const uint8_t* const* already, const int32_t* const* frame_mp,
                                  float th, int orb_dist, int check_orientation, int32_t* const* out,
                                  int32_t* nmatches, int32_t* rounds) {
    if (!C || count < 0) return RSC_ERR_ARG;
    if (orb_dist < 0 || orb_dist > 255) {  // the reference would write mvpMapPoints[-1] (bestDist starts at 256)
        g_last_error = "ORBdist outside [0, 255]";
        return RSC_ERR_ARG;
    }
    if (count == 0) return RSC_OK;
    if (!frames || !kfs || !Tcw || !already || !frame_mp || !out) return RSC_ERR_ARG;
    for (int c = 0; c < count; ++c) {
        if (!frames[c] || !kfs[c] || frames[c]->ctx != C || kfs[c]->ctx != C) return RSC_ERR_ARG;
        if (kfs[c]->n && !already[c]) return RSC_ERR_ARG;
        if (frames[c]->n && (!frame_mp[c] || !out[c])) return RSC_ERR_ARG;
        if (check_orientation && !kfs[c]->has_angles) {
            g_last_error = "orientation check on a KeyFrame view without angles (rsc_kfview_set_angles)";
            return RSC_ERR_ARG;
        }
    }
    // layout: problem table | already flags | frame_mp  (uploaded)  | windows | candidates | claims  (scratch)  |
    // out | nmatches, rounds  (the part that comes back)
    std::vector<size_t> o_al(count), o_mp(count), o_rec(count), o_cd(count), o_cl(count), o_out(count), o_cnt(count);
    int max_kf_points = 0;
    Arena A;
    A.take(sizeof(FrameProjProblem) * count);
    for (int c = 0; c < count; ++c) {
        o_al[c] = A.take((size_t)std::max(kfs[c]->n, 1));
        o_mp[c] = A.take(4 * (size_t)std::max(frames[c]->n, 1));
    }
    A.end_upload();
    for (int c = 0; c < count; ++c) {
        const size_t nk = (size_t)std::max(kfs[c]->n, 1);
        o_rec[c] = A.take(sizeof(ProjRec) * nk);
        o_cd[c] = A.take(sizeof(ProjCand) * nk);
        o_cl[c] = A.take(4 * nk);
        max_kf_points = std::max(max_kf_points, kfs[c]->n);
    }
    A.end_scratch();
    for (int c = 0; c < count; ++c) {
        o_out[c] = A.take(4 * (size_t)std::max(frames[c]->n, 1));
        o_cnt[c] = A.take_packed(8);
    }
    A.finish();
    auto fill = [&](char* h, char* d) -> int {
        for (int c = 0; c < count; ++c) {
            const rsc_kfview& k = *kfs[c];
            if (k.n) std::memcpy(h + o_al[c], already[c], (size_t)k.n);
            if (frames[c]->n) std::memcpy(h + o_mp[c], frame_mp[c], 4 * (size_t)frames[c]->n);
            FrameProjProblem p;
            p.F = frames[c]->hdr;
            p.K = k.proj;
            std::memcpy(p.Tcw, Tcw + 16 * (size_t)c, sizeof(p.Tcw));
            p.already = reinterpret_cast<const uint8_t*>(d + o_al[c]);
            p.frame_mp = reinterpret_cast<const int32_t*>(d + o_mp[c]);
            p.rec = reinterpret_cast<ProjRec*>(d + o_rec[c]);
            p.cand = reinterpret_cast<ProjCand*>(d + o_cd[c]);
            p.claim = reinterpret_cast<int32_t*>(d + o_cl[c]);
            p.out = reinterpret_cast<int32_t*>(d + o_out[c]);
            p.nmatches = reinterpret_cast<int32_t*>(d + o_cnt[c]);
            p.rounds = p.nmatches + 1;
            std::memcpy(h + sizeof(FrameProjProblem) * c, &p, sizeof(p));
        }
        return 0;
    };
    auto launch = [&](char* d) {
        return launch_search_by_projection(count, max_kf_points, reinterpret_cast<const FrameProjProblem*>(d), th,
                                           orb_dist, check_orientation ? 1 : 0, C->stream);
    };
    if (int e = arena_run(C, C->d_fp, C->h_fp, A, fill, launch)) return e;
    const char* h = C->h_fp.p;
    for (int c = 0; c < count; ++c) {
        if (frames[c]->n) std::memcpy(out[c], h + o_out[c], 4 * (size_t)frames[c]->n);
        if (nmatches) std::memcpy(&nmatches[c], h + o_cnt[c], 4);
        if (rounds) std::memcpy(&rounds[c], h + o_cnt[c] + 4, 4);
    }
    return RSC_OK;
}

// ---- SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) and Fuse(pKF, Scw, vpPoints, th, ...) (rsc_kfproj.h) ----
namespace {
int kfp_check_kf(const rsc_context* C, const rsc_kfview* k) {
    if (!k || k->ctx != C) return RSC_ERR_ARG;
    if (k->n > kKfpMaxKeypoints) {
        g_last_error = "KeyFrame with more than 8192 keypoints";
        return RSC_ERR_ARG;
    }
    if (k->dev.n_levels > 64) return RSC_ERR_ARG;  // the level field of the cached window
    return 0;
}
}  // namespace

int rsc_search_by_projection_kf_many(rsc_context* C, rsc_kfview* const* kfs, rsc_mpview* const* points, int count,
                                     const float* Scw, const uint8_t* const* already,
                                     const uint8_t* const* occupied, int th, int32_t* const* out,
                                     int32_t* nmatches, int32_t* rounds) {
    if (!C || count < 0 || count > 65535) return RSC_ERR_ARG;
    if (count == 0) return RSC_OK;
    if (!kfs || !points || !Scw || !already || !occupied || !out) return RSC_ERR_ARG;
    for (int c = 0; c < count; ++c) {
        if (int e = kfp_check_kf(C, kfs[c])) return e;
        if (!points[c] || points[c]->ctx != C) return RSC_ERR_ARG;
        if (points[c]->n && !already[c]) return RSC_ERR_ARG;
        if (kfs[c]->n && (!occupied[c] || !out[c])) return RSC_ERR_ARG;
    }
    // layout: problem table | already flags | occupied flags  (uploaded)  | windows | candidates | claims
    // (scratch)  | out | nmatches, rounds  (the part that comes back)
    std::vector<size_t> o_al(count), o_oc(count), o_rec(count), o_cd(count), o_cl(count), o_out(count), o_cnt(count);
    int max_points = 0;
    Arena A;
    A.take(sizeof(KfProjProblem) * count);
    for (int c = 0; c < count; ++c) {
        o_al[c] = A.take((size_t)std::max(points[c]->n, 1));
        o_oc[c] = A.take((size_t)std::max(kfs[c]->n, 1));
    }
    A.end_upload();
    for (int c = 0; c < count; ++c) {
        const size_t np = (size_t)std::max(points[c]->n, 1);
        o_rec[c] = A.take(sizeof(ProjRec) * np);
        o_cd[c] = A.take(sizeof(ProjCand) * np);
        o_cl[c] = A.take(4 * np);
        max_points = std::max(max_points, points[c]->n);
    }
    A.end_scratch();
    for (int c = 0; c < count; ++c) {
        o_out[c] = A.take(4 * (size_t)std::max(kfs[c]->n, 1));
        o_cnt[c] = A.take_packed(8);
    }
    A.finish();
    auto fill = [&](char* h, char* d) -> int {
        for (int c = 0; c < count; ++c) {
            const rsc_kfview& k = *kfs[c];
            const rsc_mpview& m = *points[c];
            if (m.n) std::memcpy(h + o_al[c], already[c], (size_t)m.n);
            if (k.n) std::memcpy(h + o_oc[c], occupied[c], (size_t)k.n);
            KfProjProblem p;
            p.K = k.kfp;
            p.P = m.dev;
            std::memcpy(p.Scw, Scw + 16 * (size_t)c, sizeof(p.Scw));
            p.already = reinterpret_cast<const uint8_t*>(d + o_al[c]);
            p.occupied = reinterpret_cast<const uint8_t*>(d + o_oc[c]);
            p.rec = reinterpret_cast<ProjRec*>(d + o_rec[c]);
            p.cand = reinterpret_cast<ProjCand*>(d + o_cd[c]);
            p.claim = reinterpret_cast<int32_t*>(d + o_cl[c]);
            p.out = reinterpret_cast<int32_t*>(d + o_out[c]);
            p.nmatches = reinterpret_cast<int32_t*>(d + o_cnt[c]);
            p.rounds = p.nmatches + 1;
            std::memcpy(h + sizeof(KfProjProblem) * c, &p, sizeof(p));
        }
        return 0;
    };
    auto launch = [&](char* d) {
        return launch_search_by_projection_kf(count, max_points, reinterpret_cast<const KfProjProblem*>(d),
                                              (float)th, C->stream);
    };
    if (int e = arena_run(C, C->d_fp, C->h_fp, A, fill, launch)) return e;
    const char* h = C->h_fp.p;
    for (int c = 0; c < count; ++c) {
        if (kfs[c]->n) std::memcpy(out[c], h + o_out[c], 4 * (size_t)kfs[c]->n);
        if (nmatches) std::memcpy(&nmatches[c], h + o_cnt[c], 4);
        if (rounds) std::memcpy(&rounds[c], h + o_cnt[c] + 4, 4);
    }
    return RSC_OK;
}

int rsc_fuse_sim3_many(rsc_context* C, rsc_kfview* const* kfs, int count, rsc_mpview* points, const float* Scw,
                       const uint8_t* const* in_kf, float th, int32_t* const* best_idx, int32_t* nfused) {
    if (!C || count < 0 || count > 65535) return RSC_ERR_ARG;
    if (count == 0) return RSC_OK;
    if (!kfs || !points || points->ctx != C || !Scw || !in_kf || !best_idx) return RSC_ERR_ARG;
    const int np = points->n;
    for (int c = 0; c < count; ++c) {
        if (int e = kfp_check_kf(C, kfs[c])) return e;
        if (np && (!in_kf[c] || !best_idx[c])) return RSC_ERR_ARG;
    }
    // layout: problem table | in_kf flags  (uploaded)  | best_idx  (comes back)
    // (rows of one stride each: every problem has the same np; no scratch)
    const size_t row = al256((size_t)std::max(np, 1)), row4 = al256(4 * (size_t)std::max(np, 1));
    Arena A;
    A.take(sizeof(KfFuseProblem) * count);
    const size_t o_in = A.take(row * (size_t)count);
    A.end_upload();
    A.end_scratch();
    const size_t o_best = A.take(row4 * (size_t)count);
    A.finish();
    auto fill = [&](char* h, char* d) -> int {
        for (int c = 0; c < count; ++c) {
            if (np) std::memcpy(h + o_in + row * c, in_kf[c], (size_t)np);
            KfFuseProblem p;
            p.K = kfs[c]->kfp;
            std::memcpy(p.Scw, Scw + 16 * (size_t)c, sizeof(p.Scw));
            p.in_kf = reinterpret_cast<const uint8_t*>(d + o_in + row * c);
            p.best_idx = reinterpret_cast<int32_t*>(d + o_best + row4 * c);
            std::memcpy(h + sizeof(KfFuseProblem) * c, &p, sizeof(p));
        }
        return 0;
    };
    auto launch = [&](char* d) {
        return launch_fuse_sim3(count, &points->dev, np, reinterpret_cast<const KfFuseProblem*>(d), th, C->stream);
    };
    if (int e = arena_run(C, C->d_fp, C->h_fp, A, fill, launch, /*download=*/np != 0)) return e;
    const char* h = C->h_fp.p;
    for (int c = 0; c < count; ++c) {
        const int32_t* b = reinterpret_cast<const int32_t*>(h + o_best + row4 * c);
        int nf = 0;
        for (int i = 0; i < np; ++i) {
            best_idx[c][i] = b[i];
            nf += b[i] >= 0;
        }
        if (nfused) nfused[c] = nf;
    }
    return RSC_OK;
}

// ---- LocalMapping::SearchInNeighbors: ORBmatcher::Fuse(pKF, vpMapPoints, th) (rsc_fusekf.h) ----
int rsc_fuse_kf_many(rsc_context* C, rsc_kfview* const* kfs, rsc_mpview* const* points, int count,
                     const uint8_t* const* skip, float th, int32_t* const* best_idx, int32_t* nfused) {
    if (!C || count < 0 || count > 65535) return RSC_ERR_ARG;
    if (count == 0) return RSC_OK;
    if (!kfs || !points || !skip || !best_idx) return RSC_ERR_ARG;
    if (!std::isfinite(th)) {
        g_last_error = "non-finite th";
        return RSC_ERR_ARG;
    }
    int max_points = 0;
    for (int c = 0; c < count; ++c) {
        if (int e = kfp_check_kf(C, kfs[c])) return e;
        const rsc_kfview& k = *kfs[c];
        if (!k.has_triang) {  // u_right, mbf and Ow
            g_last_error = "a KeyFrame view without rsc_kfview_set_triangulation";
            return RSC_ERR_ARG;
        }
        if (!grid_radius_ok(std::fabs(th), k.top_scale, k.dev.gw_inv, k.dev.gh_inv)) {
            g_last_error = "Fuse radius out of the grid arithmetic's range";
            return RSC_ERR_ARG;
        }
        if (!k.octaves_ok) {  // an octave is the index of mvInvLevelSigma2
            g_last_error = "KeyFrame keypoint octave out of range";
            return RSC_ERR_ARG;
        }
        if (!points[c] || points[c]->ctx != C) return RSC_ERR_ARG;
        if (points[c]->n && (!skip[c] || !best_idx[c])) return RSC_ERR_ARG;
        max_points = std::max(max_points, points[c]->n);
    }
    // layout: problem table | skip flags  (uploaded)  | best_idx  (comes back); no scratch
    std::vector<size_t> o_sk(count), o_best(count);
    Arena A;
    A.take(sizeof(FuseKfProblem) * count);
    for (int c = 0; c < count; ++c) o_sk[c] = A.take((size_t)std::max(points[c]->n, 1));
    A.end_upload();
    A.end_scratch();
    for (int c = 0; c < count; ++c) o_best[c] = A.take(4 * (size_t)std::max(points[c]->n, 1));
    A.finish();
    auto fill = [&](char* h, char* d) -> int {
        for (int c = 0; c < count; ++c) {
            const rsc_kfview& k = *kfs[c];
            const rsc_mpview& m = *points[c];
            if (m.n) std::memcpy(h + o_sk[c], skip[c], (size_t)m.n);
            FuseKfProblem p;
            p.K = k.kfp;
            p.P = m.dev;
            std::memcpy(p.Rcw, k.R, sizeof(p.Rcw));
            std::memcpy(p.tcw, k.t, sizeof(p.tcw));
            std::memcpy(p.Ow, k.tri.Ow, sizeof(p.Ow));
            p.mbf = k.tri.mbf;
            p.u_right = k.tri.u_right;
            p.skip = reinterpret_cast<const uint8_t*>(d + o_sk[c]);
            p.best_idx = reinterpret_cast<int32_t*>(d + o_best[c]);
            std::memcpy(h + sizeof(FuseKfProblem) * c, &p, sizeof(p));
        }
        return 0;
    };
    auto launch = [&](char* d) {
        return launch_fuse_kf(count, max_points, reinterpret_cast<const FuseKfProblem*>(d), th, C->stream);
    };
    if (int e = arena_run(C, C->d_fp, C->h_fp, A, fill, launch, /*download=*/max_points != 0)) return e;
    const char* h = C->h_fp.p;
    for (int c = 0; c < count; ++c) {
        const int np = points[c]->n;
        const int32_t* b = reinterpret_cast<const int32_t*>(h + o_best[c]);
        int nf = 0;
        for (int i = 0; i < np; ++i) {
            best_idx[c][i] = b[i];
            nf += b[i] >= 0;
        }
        if (nfused) nfused[c] = nf;
    }
    return RSC_OK;
}

// ---- Tracking::SearchLocalPoints: isInFrustum + SearchByProjection(Frame&, vector<MapPoint>&, th) (rsc_localproj.h) ----
namespace {
static_assert(sizeof(rsc_track_record) == sizeof(LpTrack), "rsc_track_record layout");

int local_points_impl(rsc_context* C, rsc_frameview* const* frames, rsc_mpview* const* points, int count,
                      const float* Tcw, const uint8_t* const* skip, const uint8_t* const* has_obs,
                      const uint8_t* const* frame_occ, float cos_limit, float th, float nn_ratio,
                      int32_t* const* out, rsc_track_record* const* track, int32_t* nmatches, int32_t* n_to_match,
                      int32_t* rounds, bool fused) {
    if (!C || count < 0 || count > 65535) return RSC_ERR_ARG;
    if (!(nn_ratio >= 0.0f) || !(th == th)) {  // the candidate cache's bound needs a monotone veto
        g_last_error = "nn_ratio must be >= 0";
        return RSC_ERR_ARG;
    }
    if (count == 0) return RSC_OK;
    if (!frames || !points || !skip || !has_obs || !frame_occ || !out || !track || (fused && !Tcw))
        return RSC_ERR_ARG;
    for (int c = 0; c < count; ++c) {
        if (!frames[c] || !points[c] || frames[c]->ctx != C || points[c]->ctx != C) return RSC_ERR_ARG;
        if (frames[c]->n > kLpMaxFeatures) {
            g_last_error = "Frame with more than 8192 features";
            return RSC_ERR_ARG;
        }
        if (!frames[c]->has_stereo) {
            g_last_error = "Frame view without mvuRight / mbf (rsc_frameview_set_stereo)";
            return RSC_ERR_ARG;
        }
        if (points[c]->n && (!skip[c] || !has_obs[c] || !track[c])) return RSC_ERR_ARG;
        if (frames[c]->n && (!frame_occ[c] || !out[c])) return RSC_ERR_ARG;
        if (!fused) {
            const int n_levels = (int)frames[c]->inv_level_sigma2.size();
            for (int i = 0; i < points[c]->n; ++i)
                if (track[c][i].in_view && (track[c][i].level < 0 || track[c][i].level >= n_levels)) {
                    g_last_error = "mnTrackScaleLevel out of range";
                    return RSC_ERR_ARG;
                }
        }
    }
    // layout: problem table | skip | has_obs | frame_occ | track (matcher-only)  (uploaded)  | windows |
    // candidates | claims  (scratch)  | track (fused) | out | nmatches, nToMatch, rounds  (what comes back)
    std::vector<size_t> o_sk(count), o_ho(count), o_oc(count), o_tr(count), o_rec(count), o_cd(count), o_cl(count),
        o_out(count), o_cnt(count);
    int max_points = 0;
    Arena A;
    A.take(sizeof(LocalProjProblem) * count);
    for (int c = 0; c < count; ++c) {
        const size_t np = (size_t)std::max(points[c]->n, 1), nf = (size_t)std::max(frames[c]->n, 1);
        o_sk[c] = A.take(np);
        o_ho[c] = A.take(np);
        o_oc[c] = A.take(nf);
        if (!fused) o_tr[c] = A.take(sizeof(LpTrack) * np);
    }
    A.end_upload();
    for (int c = 0; c < count; ++c) {
        const size_t np = (size_t)std::max(points[c]->n, 1);
        o_rec[c] = A.take(sizeof(LpRec) * np);
        o_cd[c] = A.take(sizeof(ProjCand) * np);
        o_cl[c] = A.take(4 * np);
        max_points = std::max(max_points, points[c]->n);
    }
    A.end_scratch();
    for (int c = 0; c < count; ++c) {
        const size_t np = (size_t)std::max(points[c]->n, 1);
        if (fused) o_tr[c] = A.take(sizeof(LpTrack) * np);
        o_out[c] = A.take(4 * (size_t)std::max(frames[c]->n, 1));
        o_cnt[c] = A.take_packed(16);
    }
    A.finish();
    auto fill = [&](char* h, char* d) -> int {
        for (int c = 0; c < count; ++c) {
            const rsc_frameview& f = *frames[c];
            const rsc_mpview& m = *points[c];
            if (m.n) {
                std::memcpy(h + o_sk[c], skip[c], (size_t)m.n);
                std::memcpy(h + o_ho[c], has_obs[c], (size_t)m.n);
                if (!fused) std::memcpy(h + o_tr[c], track[c], sizeof(LpTrack) * (size_t)m.n);
            }
            if (f.n) std::memcpy(h + o_oc[c], frame_occ[c], (size_t)f.n);
            LocalProjProblem p;
            p.F = f.hdr;
            p.u_right = f.d_uright.p;
            p.mbf = f.mbf;
            p.P = m.dev;
            if (fused) std::memcpy(p.Tcw, Tcw + 16 * (size_t)c, sizeof(p.Tcw));
            else std::memset(p.Tcw, 0, sizeof(p.Tcw));
            p.skip = reinterpret_cast<const uint8_t*>(d + o_sk[c]);
            p.has_obs = reinterpret_cast<const uint8_t*>(d + o_ho[c]);
            p.frame_occ = reinterpret_cast<const uint8_t*>(d + o_oc[c]);
            p.track = reinterpret_cast<LpTrack*>(d + o_tr[c]);
            p.rec = reinterpret_cast<LpRec*>(d + o_rec[c]);
            p.cand = reinterpret_cast<ProjCand*>(d + o_cd[c]);
            p.claim = reinterpret_cast<int32_t*>(d + o_cl[c]);
            p.out = reinterpret_cast<int32_t*>(d + o_out[c]);
            p.counts = reinterpret_cast<int32_t*>(d + o_cnt[c]);
            std::memcpy(h + sizeof(LocalProjProblem) * c, &p, sizeof(p));
        }
        return 0;
    };
    auto launch = [&](char* d) {
        return launch_search_local_points(count, max_points, reinterpret_cast<const LocalProjProblem*>(d),
                                          fused ? 1 : 0, cos_limit, th, nn_ratio,
                                          C->timing ? C->ev[5] : nullptr, C->stream);
    };
    if (int e = arena_run(C, C->d_fp, C->h_fp, A, fill, launch, true, /*mid=*/true)) return e;
    const char* h = C->h_fp.p;
    for (int c = 0; c < count; ++c) {
        if (frames[c]->n) std::memcpy(out[c], h + o_out[c], 4 * (size_t)frames[c]->n);
        if (fused && points[c]->n) std::memcpy(track[c], h + o_tr[c], sizeof(LpTrack) * (size_t)points[c]->n);
        if (nmatches) std::memcpy(&nmatches[c], h + o_cnt[c], 4);
        if (n_to_match) std::memcpy(&n_to_match[c], h + o_cnt[c] + 4, 4);
        if (rounds) std::memcpy(&rounds[c], h + o_cnt[c] + 8, 4);
    }
    return RSC_OK;
}
}  // namespace

int rsc_search_local_points_many(rsc_context* C, rsc_frameview* const* frames, rsc_mpview* const* points, int count,
                                 const float* Tcw, const uint8_t* const* skip, const uint8_t* const* has_obs,
                                 const uint8_t* const* frame_occ, float cos_limit, float th, float nn_ratio,
                                 int32_t* const* out, rsc_track_record* const* track, int32_t* nmatches,
                                 int32_t* n_to_match, int32_t* rounds) {
    return local_points_impl(C, frames, points, count, Tcw, skip, has_obs, frame_occ, cos_limit, th, nn_ratio, out,
                             track, nmatches, n_to_match, rounds, true);
}

int rsc_search_by_projection_points_many(rsc_context* C, rsc_frameview* const* frames, rsc_mpview* const* points,
                                         int count, const uint8_t* const* skip, const uint8_t* const* has_obs,
                                         const uint8_t* const* frame_occ, float th, float nn_ratio,
                                         int32_t* const* out, const rsc_track_record* const* track,
                                         int32_t* nmatches, int32_t* n_to_match, int32_t* rounds) {
    return local_points_impl(C, frames, points, count, nullptr, skip, has_obs, frame_occ, 0.0f, th, nn_ratio, out,
                             const_cast<rsc_track_record* const*>(track), nmatches, n_to_match, rounds, false);
}

// ---- ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th) (ORBmatcher.cpp:1173-1315, rsc_lastproj.h) ----
// what rsc_search_by_projection_last_many refuses before any launch
int last_check_args(rsc_context* C, rsc_frameview* const* frames, rsc_lastframe* const* lasts, int count, float th) {
    if (!std::isfinite(th)) {
        g_last_error = "th is not finite";
        return RSC_ERR_ARG;
    }
    for (int c = 0; c < count; ++c) {
        if (!frames[c] || !lasts[c] || frames[c]->ctx != C || lasts[c]->ctx != C) return RSC_ERR_ARG;
        const rsc_frameview& f = *frames[c];
        const rsc_lastframe& l = *lasts[c];
        if (f.n > kLastMaxFeatures || l.n > kLastMaxSlots) {
            g_last_error = "more than 8192 features or LastFrame slots";
            return RSC_ERR_ARG;
        }
        if (!f.has_stereo) {
            g_last_error = "Frame view without mvuRight / mbf (rsc_frameview_set_stereo)";
            return RSC_ERR_ARG;
        }
        if (!grid_radius_ok(std::fabs(th), f.top_scale, f.gw_inv, f.gh_inv)) {
            g_last_error = "last-frame SearchByProjection radius out of the grid arithmetic's range";
            return RSC_ERR_ARG;
        }
        const int n_levels = (int)f.inv_level_sigma2.size();
        for (int i = 0; i < l.n; ++i)
            if (l.mp_state[i] != 0 && (l.octave[i] < 0 || l.octave[i] >= n_levels)) {
                g_last_error = "LastFrame keypoint octave out of range on a slot with a MapPoint";
                return RSC_ERR_ARG;
            }
    }
    return 0;
}

int rsc_search_by_projection_last_many(rsc_context* C, rsc_frameview* const* frames, rsc_lastframe* const* lasts,
                                       int count, const float* Tcw_cur, const float* Tcw_last, const float* mb,
                                       const uint8_t* const* frame_occ, float th, int check_orientation,
                                       int32_t* const* out, int32_t* nmatches, int32_t* mode, int32_t* rounds) {
    if (!C || count < 0 || count > 65535) return RSC_ERR_ARG;
    if (count == 0) return RSC_OK;
    if (!frames || !lasts || !Tcw_cur || !Tcw_last || !mb || !out) return RSC_ERR_ARG;
    if (int e = last_check_args(C, frames, lasts, count, th)) return e;
    for (int c = 0; c < count; ++c)
        if (frames[c]->n && !out[c]) return RSC_ERR_ARG;
    // layout: problem table | frame_occ  (uploaded)  | windows | candidates | claims  (scratch)  |
    // out | nmatches, mode, rounds, claims  (what comes back)
    std::vector<size_t> o_oc(count), o_rec(count), o_cd(count), o_cl(count), o_out(count), o_cnt(count);
    int max_slots = 0;
    Arena A;
    A.take(sizeof(LastProjProblem) * count);
    for (int c = 0; c < count; ++c) o_oc[c] = A.take((size_t)std::max(frames[c]->n, 1));
    A.end_upload();
    for (int c = 0; c < count; ++c) {
        const size_t nl = (size_t)std::max(lasts[c]->n, 1);
        o_rec[c] = A.take(sizeof(LpRec) * nl);
        o_cd[c] = A.take(sizeof(ProjCand) * nl);
        o_cl[c] = A.take(4 * nl);
        max_slots = std::max(max_slots, lasts[c]->n);
    }
    A.end_scratch();
    for (int c = 0; c < count; ++c) {
        o_out[c] = A.take(4 * (size_t)std::max(frames[c]->n, 1));
        o_cnt[c] = A.take_packed(16);
    }
    A.finish();
    auto fill = [&](char* h, char* d) -> int {
        for (int c = 0; c < count; ++c) {
            const rsc_frameview& f = *frames[c];
            const rsc_lastframe& l = *lasts[c];
            if (frame_occ && frame_occ[c]) {
                if (f.n) std::memcpy(h + o_oc[c], frame_occ[c], (size_t)f.n);
            } else {
                std::memset(h + o_oc[c], 0, (size_t)std::max(f.n, 1));
            }
            LastProjProblem p;
            p.F = f.hdr;
            p.u_right = f.d_uright.p;
            p.mbf = f.mbf;
            p.mode = last_mode(Tcw_cur + 16 * (size_t)c, Tcw_last + 16 * (size_t)c, mb[c]);
            p.L = l.dev;
            std::memcpy(p.Tcw, Tcw_cur + 16 * (size_t)c, sizeof(p.Tcw));
            p.frame_occ = reinterpret_cast<const uint8_t*>(d + o_oc[c]);
            p.rec = reinterpret_cast<LpRec*>(d + o_rec[c]);
            p.cand = reinterpret_cast<ProjCand*>(d + o_cd[c]);
            p.claim = reinterpret_cast<int32_t*>(d + o_cl[c]);
            p.out = reinterpret_cast<int32_t*>(d + o_out[c]);
            p.counts = reinterpret_cast<int32_t*>(d + o_cnt[c]);
            std::memcpy(h + sizeof(LastProjProblem) * c, &p, sizeof(p));
        }
        return 0;
    };
    auto launch = [&](char* d) {
        return launch_search_by_projection_last(count, max_slots, reinterpret_cast<const LastProjProblem*>(d), th,
                                                check_orientation ? 1 : 0, C->timing ? C->ev[5] : nullptr,
                                                C->stream);
    };
    if (int e = arena_run(C, C->d_fp, C->h_fp, A, fill, launch, true, /*mid=*/true)) return e;
    const char* h = C->h_fp.p;
    for (int c = 0; c < count; ++c) {
        if (frames[c]->n) std::memcpy(out[c], h + o_out[c], 4 * (size_t)frames[c]->n);
        if (nmatches) std::memcpy(&nmatches[c], h + o_cnt[c], 4);
        if (mode) std::memcpy(&mode[c], h + o_cnt[c] + 4, 4);
        if (rounds) std::memcpy(&rounds[c], h + o_cnt[c] + 8, 4);
    }
    return RSC_OK;
}

// ---- LocalMapping::CreateNewMapPoints: SearchForTriangulation and the triangulation (rsc_triang.h) ----
namespace {
int tri_check_view(const rsc_context* C, const rsc_kfview* k) {
    if (!k || k->ctx != C) return RSC_ERR_ARG;
    if (k->n > kTriMaxFeatures) {
        g_last_error = "more than 8192 keypoints in one view";
        return RSC_ERR_ARG;
    }
    if (!k->has_triang) {
        g_last_error = "a KeyFrame view without rsc_kfview_set_triangulation";
        return RSC_ERR_ARG;
    }
    return 0;
}
}  // namespace

int rsc_search_for_triangulation_many(rsc_context* C, const rsc_bow* const* bow1, rsc_kfview* const* kf1,
                                      const rsc_bow* const* bow2, rsc_kfview* const* kf2, int count,
                                      const float* F12, const uint8_t* const* has_mp1,
                                      const uint8_t* const* has_mp2, const int32_t* only_stereo,
                                      int check_orientation, int32_t* const* matches12, int32_t* nmatches,
                                      int32_t* den_zero, uint8_t* const* den_zero_slot) {
    return tri_search_impl(C, bow1, kf1, bow2, kf2, count, F12, has_mp1, has_mp2, only_stereo, check_orientation,
                           /*speculative=*/0, matches12, nmatches, den_zero, den_zero_slot);
}

// speculative (rsc_create_new_map_points_many, orientation off): a problem with den_zero keeps its matches12
int tri_search_impl(rsc_context* C, const rsc_bow* const* bow1, rsc_kfview* const* kf1, const rsc_bow* const* bow2,
                    rsc_kfview* const* kf2, int count, const float* F12, const uint8_t* const* has_mp1,
                    const uint8_t* const* has_mp2, const int32_t* only_stereo, int check_orientation, int speculative,
                    int32_t* const* matches12, int32_t* nmatches, int32_t* den_zero, uint8_t* const* den_zero_slot) {
    if (!C || count < 0 || (speculative && check_orientation)) return RSC_ERR_ARG;
    if (count == 0) return RSC_OK;
    if (!bow1 || !kf1 || !bow2 || !kf2 || !F12 || !matches12) return RSC_ERR_ARG;
    for (int c = 0; c < count; ++c) {
        if (int e = tri_check_view(C, kf1[c])) return e;
        if (int e = tri_check_view(C, kf2[c])) return e;
        if (!bow1[c] || !bow2[c] || bow1[c]->ctx != C || bow2[c]->ctx != C) return RSC_ERR_ARG;
        if (bow1[c]->n != kf1[c]->n || bow2[c]->n != kf2[c]->n) {
            g_last_error = "the rsc_bow and the rsc_kfview of one KeyFrame differ in size";
            return RSC_ERR_ARG;
        }
        if (kf1[c]->n && !matches12[c]) return RSC_ERR_ARG;
        for (int i = 0; i < 9; ++i)
            if (!std::isfinite(F12[9 * (size_t)c + i])) {
                g_last_error = "non-finite F12";
                return RSC_ERR_ARG;
            }
        if (!kf2[c]->octaves_ok) {
            g_last_error = "KeyFrame-2 keypoint octave out of range";
            return RSC_ERR_ARG;
        }
    }
    // layout: problem table | has1 | has2  (uploaded)  | items | item counts | node table  (scratch)  |
    // matches12 | den_zero_slot | counts  (the part that comes back)
    std::vector<size_t> o_h1(count), o_h2(count), o_it(count), o_ni(count), o_m(count), o_dz(count), o_cnt(count);
    Arena A;
    A.take(sizeof(TriMatchProblem) * count);
    for (int c = 0; c < count; ++c) {
        o_h1[c] = A.take((size_t)std::max(kf1[c]->n, 1));
        o_h2[c] = A.take((size_t)std::max(kf2[c]->n, 1));
    }
    A.end_upload();
    for (int c = 0; c < count; ++c) {
        o_it[c] = A.take(sizeof(int4) * kTriClasses * (size_t)std::max(bow1[c]->n_feat, 1));
        o_ni[c] = A.take(16);
    }
    const size_t o_nodes = A.take(sizeof(int2) * (size_t)kTriMaxFeatures * count);
    A.end_scratch();
    for (int c = 0; c < count; ++c) {
        o_m[c] = A.take(4 * (size_t)std::max(kf1[c]->n, 1));
        o_dz[c] = A.take((size_t)std::max(kf1[c]->n, 1));
        o_cnt[c] = A.take(8);
    }
    A.finish();
    auto fill = [&](char* h, char* d) -> int {
        for (int c = 0; c < count; ++c) {
            const rsc_kfview& k1 = *kf1[c];
            const rsc_kfview& k2 = *kf2[c];
            const uint8_t* g1 = has_mp1 ? has_mp1[c] : nullptr;
            const uint8_t* g2 = has_mp2 ? has_mp2[c] : nullptr;
            uint8_t* a1 = reinterpret_cast<uint8_t*>(h + o_h1[c]);
            uint8_t* a2 = reinterpret_cast<uint8_t*>(h + o_h2[c]);
            const bool stereo_only = only_stereo && only_stereo[c] != 0;
            // a skipped feature: it has a MapPoint (:534, :567), or bOnlyStereo and it is not stereo (:539-541,
            // :572-574; `>= 0`, false for a NaN)
            for (int i = 0; i < k1.n; ++i)
                a1[i] = (g1 ? (g1[i] != 0) : (k1.mp_state[i] != 0)) || (stereo_only && !(k1.h_uright[i] >= 0));
            for (int i = 0; i < k2.n; ++i)
                a2[i] = (g2 ? (g2[i] != 0) : (k2.mp_state[i] != 0)) || (stereo_only && !(k2.h_uright[i] >= 0));
            TriMatchProblem p;
            p.A = bow1[c]->hdr;
            p.B = bow2[c]->hdr;
            p.kp1 = k1.dev.kp;
            p.kp2 = k2.dev.kp;
            p.oct2 = k2.dev.octave;
            p.scale2 = k2.dev.scale;
            p.ur1 = k1.tri.u_right;
            p.ur2 = k2.tri.u_right;
            p.angle1 = bow1[c]->hdr.angle;
            p.angle2 = bow2[c]->hdr.angle;
            p.has1 = reinterpret_cast<const uint8_t*>(d + o_h1[c]);
            p.has2 = reinterpret_cast<const uint8_t*>(d + o_h2[c]);
            std::memcpy(p.F, F12 + 9 * (size_t)c, sizeof(p.F));
            // the epipole (:496-502): Cw = pKF1->GetCameraCenter() = Ow
            tri_epipole(k2.R, k2.t, k1.tri.Ow, k2.K[0], k2.K[1], k2.K[2], k2.K[3], p.ex, p.ey);
            p.items = reinterpret_cast<int4*>(d + o_it[c]);
            p.nitems = reinterpret_cast<int32_t*>(d + o_ni[c]);
            p.matches12 = reinterpret_cast<int32_t*>(d + o_m[c]);
            p.den_zero_slot = reinterpret_cast<uint8_t*>(d + o_dz[c]);
            p.counts = reinterpret_cast<int32_t*>(d + o_cnt[c]);
            std::memcpy(h + sizeof(TriMatchProblem) * c, &p, sizeof(p));
        }
        return 0;
    };
    auto launch = [&](char* d) {
        return launch_search_for_triangulation(count, reinterpret_cast<const TriMatchProblem*>(d),
                                               reinterpret_cast<int2*>(d + o_nodes),
                                               (check_orientation ? 1 : 0) | (speculative ? 2 : 0), C->stream);
    };
    if (int e = arena_run(C, C->d_fp, C->h_fp, A, fill, launch)) return e;
    const char* h = C->h_fp.p;
    for (int c = 0; c < count; ++c) {
        const size_t n1 = (size_t)kf1[c]->n;
        if (n1) std::memcpy(matches12[c], h + o_m[c], 4 * n1);
        if (n1 && den_zero_slot && den_zero_slot[c]) std::memcpy(den_zero_slot[c], h + o_dz[c], n1);
        if (nmatches) std::memcpy(&nmatches[c], h + o_cnt[c], 4);
        if (den_zero) std::memcpy(&den_zero[c], h + o_cnt[c] + 4, 4);
    }
    return RSC_OK;
}

int rsc_triangulate_pairs_many(rsc_context* C, rsc_kfview* const* kf1, rsc_kfview* const* kf2, int count,
                               const int32_t* npairs, const int32_t* const* pairs, int32_t* const* status,
                               float* const* x3d) {
    if (!C || count < 0) return RSC_ERR_ARG;
    if (count == 0) return RSC_OK;
    if (!kf1 || !kf2 || !npairs || !pairs || !status || !x3d) return RSC_ERR_ARG;
    int max_pairs = 0;
    for (int c = 0; c < count; ++c) {
        if (int e = tri_check_view(C, kf1[c])) return e;
        if (int e = tri_check_view(C, kf2[c])) return e;
        if (npairs[c] < 0 || (npairs[c] && (!pairs[c] || !status[c] || !x3d[c]))) return RSC_ERR_ARG;
        const rsc_kfview& k1 = *kf1[c];
        const rsc_kfview& k2 = *kf2[c];
        for (int i = 0; i < npairs[c]; ++i) {
            const int32_t i1 = pairs[c][2 * i], i2 = pairs[c][2 * i + 1];
            if (i1 < 0 || i1 >= k1.n || i2 < 0 || i2 >= k2.n) {
                g_last_error = "pair index out of range";
                return RSC_ERR_ARG;
            }
            if (k1.octave[i1] < 0 || k1.octave[i1] >= k1.dev.n_levels || k2.octave[i2] < 0 ||
                k2.octave[i2] >= k2.dev.n_levels) {
                g_last_error = "keypoint octave out of range";
                return RSC_ERR_ARG;
            }
        }
        max_pairs = std::max(max_pairs, npairs[c]);
    }
    // layout: problem table | pairs  (uploaded)  |  status | x3d  (the part that comes back)
    std::vector<size_t> o_p(count), o_st(count), o_x(count);
    Arena A;
    A.take(sizeof(TriPairsProblem) * count);
    for (int c = 0; c < count; ++c) o_p[c] = A.take(8 * (size_t)std::max(npairs[c], 1));
    A.end_upload();
    A.end_scratch();
    for (int c = 0; c < count; ++c) {
        o_st[c] = A.take(4 * (size_t)std::max(npairs[c], 1));
        o_x[c] = A.take(12 * (size_t)std::max(npairs[c], 1));
    }
    A.finish();
    auto fill = [&](char* h, char* d) -> int {
        for (int c = 0; c < count; ++c) {
            if (npairs[c]) std::memcpy(h + o_p[c], pairs[c], 8 * (size_t)npairs[c]);
            TriPairsProblem p;
            p.K1 = kf1[c]->tri;
            p.K2 = kf2[c]->tri;
            p.pairs = reinterpret_cast<const int32_t*>(d + o_p[c]);
            p.npairs = npairs[c];
            p.status = reinterpret_cast<int32_t*>(d + o_st[c]);
            p.x3d = reinterpret_cast<float*>(d + o_x[c]);
            std::memcpy(h + sizeof(TriPairsProblem) * c, &p, sizeof(p));
        }
        return 0;
    };
    auto launch = [&](char* d) {
        return launch_triangulate_pairs(count, max_pairs, reinterpret_cast<const TriPairsProblem*>(d), C->stream);
    };
    if (int e = arena_run(C, C->d_fp, C->h_fp, A, fill, launch)) return e;
    const char* h = C->h_fp.p;
    for (int c = 0; c < count; ++c) {
        if (!npairs[c]) continue;
        std::memcpy(status[c], h + o_st[c], 4 * (size_t)npairs[c]);
        std::memcpy(x3d[c], h + o_x[c], 12 * (size_t)npairs[c]);
    }
    return RSC_OK;
}

}  // extern "C"
