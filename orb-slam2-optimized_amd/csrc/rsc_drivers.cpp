// rsc_drivers.cpp — the driver entry points of the C ABI: they launch nothing themselves and only
// compose other ABI calls in the reference's control-flow order, on the bookkeeping of rsc_rounds.h.
#include "rsc_host.h"
#include "rsc_rounds.h"
#include "rsc_poseopt.h"
#include "rsc_sim3opt.h"
#include "rsc_sim3compose.h"

namespace {
// hypotheses the next iterate(5) call runs unless it succeeds: PnP's '||' loop (Q1)
// max(5, maxIts - mnIterations), Sim3's '&&' loop min(5, maxIts - mnIterations); none when N is
// below minInliers (the call returns at once)
int pnp_pred_its(const rsc_pnp* s) {
    const PnPState& t = s->st;
    return (t.N < t.mRansacMinInliers) ? 0 : std::max(0, std::max(5, t.mRansacMaxIts - t.mnIterations));
}
int sim3_pred_its(const rsc_sim3* s) {
    const Sim3State& t = s->st;
    return (t.N < t.mRansacMinInliers) ? 0 : std::max(0, std::min(5, t.mRansacMaxIts - t.mnIterations));
}
}  // namespace

extern "C" {
// Tracking::Relocalization's refinement chain (Tracking.cpp:1294-1323); each stage one launch over the
// candidates still in the chain.
int rsc_reloc_refine_many(rsc_context* C, rsc_frameview* const* frames, rsc_kfview* const* kfs, int count,
                          const rsc_reloc_frame* fr, int32_t* const* frame_mp, const uint8_t* const* found,
                          const int32_t* n_good_in, const float* Tcw_in, rsc_reloc_refine_result* out) {
    if (!C || count < 0) return RSC_ERR_ARG;
    if (count == 0) return RSC_OK;
    if (!frames || !kfs || !fr || !frame_mp || !found || !n_good_in || !Tcw_in || !out) return RSC_ERR_ARG;
    for (int c = 0; c < count; ++c) {
        if (!frames[c] || !kfs[c] || frames[c]->ctx != C || kfs[c]->ctx != C) return RSC_ERR_ARG;
        if ((frames[c]->n && !frame_mp[c]) || (kfs[c]->n && !found[c])) return RSC_ERR_ARG;
        for (int f = 0; f < frames[c]->n; ++f)
            if (frame_mp[c][f] < -1 || frame_mp[c][f] >= kfs[c]->n) return RSC_ERR_ARG;
        rsc_reloc_refine_result& r = out[c];
        r.n_good = n_good_in[c];
        r.n_additional[0] = r.n_additional[1] = -1;
        r.pose_opts = 0;
        std::memcpy(r.Tcw, Tcw_in + 16 * (size_t)c, sizeof(r.Tcw));
    }
    // SearchByProjection over the candidates in `sel` with sAlreadyFound = fnd[c]; the new matches are
    // written to frame_mp (CurrentFrame.mvpMapPoints[bestIdx2] = pMP), nadd[c] = the return value
    std::vector<int32_t> nadd(count, 0);
    auto search = [&](const std::vector<int>& sel, const std::vector<const uint8_t*>& fnd, float th, int orb_dist) -> int {
        const int m = (int)sel.size();
        std::vector<rsc_frameview*> F = gather(frames, sel);
        std::vector<rsc_kfview*> K = gather(kfs, sel);
        std::vector<int32_t*> mp = gather(frame_mp, sel);
        std::vector<float> T(16 * (size_t)m);
        std::vector<std::vector<int32_t>> res(m);
        std::vector<int32_t*> rp(m);
        std::vector<int32_t> nm(m);
        for (int q = 0; q < m; ++q) {
            const int c = sel[q];
            std::memcpy(&T[16 * (size_t)q], out[c].Tcw, 16 * sizeof(float));
            res[q].assign((size_t)std::max(frames[c]->n, 1), -1);
            rp[q] = res[q].data();
        }
        if (int st = rsc_search_by_projection_many(C, F.data(), K.data(), m, T.data(), fnd.data(), mp.data(), th,
                                                   orb_dist, 1, rp.data(), nm.data(), nullptr))
            return st;
        for (int q = 0; q < m; ++q) {
            const int c = sel[q];
            for (int f = 0; f < frames[c]->n; ++f)
                if (res[q][f] >= 0) frame_mp[c][f] = res[q][f];
            nadd[c] = nm[q];
        }
        return RSC_OK;
    };
    // PoseOptimization(&mCurrentFrame) over the candidates in `sel`, on every occupied slot
    auto optimise = [&](const std::vector<int>& sel, bool null_outliers) -> int {
        const int m = (int)sel.size();
        PoseOptBatch B;
        for (int c : sel) {
            const rsc_frameview& F = *frames[c];
            B.add_slots(F.n, frame_mp[c], kfs[c]->mp_pos.data(), F.kp.data(), F.octave.data(),
                        F.inv_level_sigma2.data(), F.K, fr[c].u_right, fr[c].bf, out[c].Tcw);
        }
        std::vector<rsc_poseopt_result> res(m);
        if (int st = rsc_pose_optimization_many(C, B.problems.data(), m, res.data(), B.outlier.data())) return st;
        for (int q = 0; q < m; ++q) {
            const int c = sel[q];
            out[c].n_good = res[q].n_good;
            std::memcpy(out[c].Tcw, res[q].Tcw, sizeof(out[c].Tcw));
            out[c].pose_opts++;
            if (null_outliers)  // :1317-1319
                for (int f = 0; f < frames[c]->n; ++f)
                    if (B.arrays[q].has_mp[f] && B.outlier[q][f]) frame_mp[c][f] = -1;
        }
        return RSC_OK;
    };
    std::vector<int> s1, s2, s3, s4;
    std::vector<const uint8_t*> f1;
    for (int c = 0; c < count; ++c)
        if (out[c].n_good < 50) {  // :1294
            s1.push_back(c);
            f1.push_back(found[c]);
        }
    if (s1.empty()) return RSC_OK;
    if (int st = search(s1, f1, 10.0f, 100)) return st;  // :1296
    for (int c : s1) {
        out[c].n_additional[0] = nadd[c];
        if (nadd[c] + out[c].n_good >= 50) s2.push_back(c);  // :1298
    }
    if (s2.empty()) return RSC_OK;
    if (int st = optimise(s2, false)) return st;  // :1300
    std::vector<std::vector<uint8_t>> found2;
    for (int c : s2)
        if (out[c].n_good > 30 && out[c].n_good < 50) {  // :1304
            s3.push_back(c);
            std::vector<uint8_t> fnd((size_t)std::max(kfs[c]->n, 1), 0);  // :1306-1309
            for (int f = 0; f < frames[c]->n; ++f)
                if (frame_mp[c][f] >= 0) fnd[frame_mp[c][f]] = 1;
            found2.push_back(std::move(fnd));
        }
    if (s3.empty()) return RSC_OK;
    std::vector<const uint8_t*> f3;
    for (const auto& v : found2) f3.push_back(v.data());
    if (int st = search(s3, f3, 3.0f, 64)) return st;  // :1310
    for (int c : s3) {
        out[c].n_additional[1] = nadd[c];
        if (out[c].n_good + nadd[c] >= 50) s4.push_back(c);  // :1313
    }
    if (s4.empty()) return RSC_OK;
    return optimise(s4, true);  // :1315-1319
}

// ---- Event drivers (config 5) ----
int rsc_reloc_events(rsc_pnp* const* solvers, const int32_t* event_begin, int n_events, rsc_pnp_result* per_candidate,
                     rsc_event_result* per_event) {
    if (n_events <= 0) return RSC_OK;
    if (!solvers || !event_begin || !per_candidate || !per_event) return RSC_ERR_ARG;
    const int total = event_begin[n_events];
    for (int e = 0; e < n_events; ++e) {
        if (event_begin[e + 1] < event_begin[e]) return RSC_ERR_ARG;
        per_event[e] = rsc_event_result{-1, -1, -1, 0};
    }
    for (int i = 0; i < total; ++i)
        if (!solvers[i]) return RSC_ERR_ARG;
    EventRounds R(solvers, event_begin, n_events);
    while (R.collect()) {
        std::vector<rsc_pnp*> act = gather(solvers, R.idx);
        std::vector<int32_t> its(act.size(), 5);
        std::vector<rsc_pnp_result> r(act.size());
        std::vector<uint8_t*> nomask(act.size(), nullptr);
        if (int st = rsc_pnp_iterate_many(act.data(), (int)act.size(), its.data(), r.data(), nomask.data())) return st;
        for (size_t q = 0; q < act.size(); ++q) R.take((int)q, r[q], per_candidate);
        for (int e = 0; e < n_events; ++e) {  // the first success of the round in candidate order wins
            if (R.resolved[e]) continue;
            const int i = R.next_success(e, event_begin[e], per_candidate);
            if (i < event_begin[e + 1]) R.win(e, i, per_candidate[i], per_event[e]);
        }
        R.close();
    }
    return RSC_OK;
}

int rsc_loop_events(rsc_sim3* const* solvers, const int32_t* event_begin, int n_events,
                    rsc_sim3_result* per_candidate, rsc_event_result* per_event) {
    if (n_events <= 0) return RSC_OK;
    if (!solvers || !event_begin || !per_candidate || !per_event) return RSC_ERR_ARG;
    const int total = event_begin[n_events];
    std::vector<int32_t> its(total), start_it(total);
    for (int i = 0; i < total; ++i) {
        if (!solvers[i]) return RSC_ERR_ARG;
        start_it[i] = solvers[i]->st.mnIterations;
        its[i] = std::max(1, solvers[i]->st.mRansacMaxIts - solvers[i]->st.mnIterations);
    }
    std::vector<uint8_t*> nomask(total, nullptr);
    if (total > 0)
        if (int st = rsc_sim3_iterate_many(solvers, total, its.data(), per_candidate, nomask.data())) return st;
    for (int e = 0; e < n_events; ++e) {
        per_event[e] = rsc_event_result{-1, -1, -1, 0};
        int best_round = 0;
        for (int i = event_begin[e]; i < event_begin[e + 1]; ++i) {
            if (!per_candidate[i].ok) continue;
            const int h = per_candidate[i].iterations - 1 - start_it[i];
            const int round = h / 5;
            if (per_event[e].winner < 0 || round < best_round) {
                best_round = round;
                per_event[e] = rsc_event_result{i - event_begin[e], round, h, per_candidate[i].n_inliers};
            }
        }
    }
    return RSC_OK;
}

// ---- Events on the reference's shared rand() stream (Q3): shared_events of rsc_rounds.h ----
int rsc_reloc_events_shared(rsc_pnp* const* solvers, const int32_t* event_begin, int n_events,
                            rsc_stream* const* streams, rsc_pnp_result* per_candidate, rsc_event_result* per_event) {
    for (int i = 0; n_events > 0 && solvers && event_begin && i < event_begin[n_events]; ++i)
        if (solvers[i] && solvers[i]->stream) return RSC_ERR_ARG;  // events position their own calls
    return shared_events(solvers, event_begin, n_events, streams, per_candidate, per_event, pnp_iterate_many_impl,
                         pnp_pred_its);
}

int rsc_loop_events_shared(rsc_sim3* const* solvers, const int32_t* event_begin, int n_events,
                           rsc_stream* const* streams, rsc_sim3_result* per_candidate, rsc_event_result* per_event) {
    for (int i = 0; n_events > 0 && solvers && event_begin && i < event_begin[n_events]; ++i)
        if (solvers[i] && solvers[i]->stream) return RSC_ERR_ARG;
    return shared_events(solvers, event_begin, n_events, streams, per_candidate, per_event, sim3_iterate_many_impl,
                         sim3_pred_its);
}

// ---- Gated events (round 6) ----
// Tracking::Relocalization (Tracking.cpp:1239-1335): each round runs iterate(5) on every live
// candidate of every unresolved event in one set of launches (own streams: the results are the
// reference's calls whatever happens before them in the round), then walks each event's successes in
// candidate order: PoseOptimization on the success (mCurrentFrame.mvpMapPoints = the inlier matches,
// mTcw = the RANSAC pose, :1268-1284), nGood < 10 -> the next success of the round (:1286-1287),
// nGood >= 50 -> match (:1327-1331), otherwise SearchByProjection's turn (handed off).  The gate
// passes of all events run as one rsc_pose_optimization_many each.
//
// rsc_reloc_events_refined is the same loop with `refine` set: a success with 10 <= nGood < 50 goes
// through the SearchByProjection chain (rsc_reloc_refine_many over the events of the pass) and is a match
// when that leaves nGood >= 50; otherwise the walk continues with the event's next success (:1327-1333).
namespace {
struct RelocRefine {
    const rsc_reloc_candidate* cands;
    rsc_frameview* const* views;
    rsc_reloc_refined_result* per_event;
    int32_t* const* frame_mp_out;
};

int reloc_events_gated_impl(rsc_pnp* const* solvers, const int32_t* event_begin, int n_events,
                            const rsc_reloc_frame* frames, rsc_pnp_result* per_candidate,
                            rsc_reloc_gate_result* per_event, uint8_t* const* outlier, uint8_t* const* inliers,
                            const RelocRefine* refine) {
    if (n_events <= 0) return RSC_OK;
    if (!solvers || !event_begin || !frames || !per_candidate || !per_event) return RSC_ERR_ARG;
    const int total = event_begin[n_events];
    rsc_context* C = nullptr;
    for (int e = 0; e < n_events; ++e) {
        if (event_begin[e + 1] < event_begin[e] || event_begin[e] < 0) return RSC_ERR_ARG;
        rsc_reloc_gate_result& r = per_event[e];
        std::memset(&r, 0, sizeof(r));
        r.status = RSC_GATE_NONE;
        r.winner = r.round = r.hypothesis = -1;
        for (int i = event_begin[e]; i < event_begin[e + 1]; ++i) {
            if (!solvers[i]) return RSC_ERR_ARG;
            if (solvers[i]->stream) return RSC_ERR_UNSUPPORTED;  // gating moves later calls' stream positions
            if (!C) C = solvers[i]->ctx;
            // one Frame per event: every candidate's vbInliers indexes the same mCurrentFrame slots
            if (solvers[i]->ctx != C || solvers[i]->st.N_points != solvers[event_begin[e]]->st.N_points)
                return RSC_ERR_ARG;
        }
    }
    if (!C) return RSC_OK;
    std::vector<std::vector<uint8_t>> mask(total);
    for (int i = 0; i < total; ++i) mask[i].assign((size_t)std::max(solvers[i]->st.N_points, 1), 0);
    struct Job { int e, i; };  // a gate job: event and candidate (its PoseOptimization problem is B's q-th)
    EventRounds R(solvers, event_begin, n_events);
    // an accepted (or handed-off) success resolves its event; mp: its mvpMapPoints as KeyFrame slots (refined form)
    auto accept = [&](const Job& j, int status, int n_good, const float* Tcw, const int32_t* mp) {
        rsc_reloc_gate_result& g = per_event[j.e];
        g.status = status;
        R.win(j.e, j.i, per_candidate[j.i], g);
        g.n_good = n_good;
        std::memcpy(g.Tcw, Tcw, sizeof(g.Tcw));
        const size_t nf = (size_t)solvers[j.i]->st.N_points;
        if (refine && refine->frame_mp_out && refine->frame_mp_out[j.e]) std::memcpy(refine->frame_mp_out[j.e], mp, 4 * nf);
        if (inliers && inliers[j.e]) std::memcpy(inliers[j.e], mask[j.i].data(), nf);
    };
    while (R.collect()) {
        std::vector<rsc_pnp*> act = gather(solvers, R.idx);
        std::vector<int32_t> its(act.size(), 5);
        std::vector<rsc_pnp_result> r(act.size());
        std::vector<uint8_t*> mp(act.size());
        for (size_t q = 0; q < act.size(); ++q) mp[q] = mask[R.idx[q]].data();
        if (int st = rsc_pnp_iterate_many(act.data(), (int)act.size(), its.data(), r.data(), mp.data())) return st;
        for (size_t q = 0; q < act.size(); ++q) R.take((int)q, r[q], per_candidate);
        // gate passes: each unresolved event's next success of this round, in candidate order
        std::vector<int> cursor(event_begin, event_begin + n_events);
        for (;;) {
            std::vector<Job> jobs;
            PoseOptBatch B;
            for (int e = 0; e < n_events; ++e) {
                if (R.resolved[e]) continue;
                const int i = R.next_success(e, cursor[e], per_candidate);
                cursor[e] = i + 1;
                if (i >= event_begin[e + 1]) continue;
                const rsc_pnp* s = solvers[i];
                const PnPState& st = s->st;
                B.add_compacted(st.N_points, st.N, st.kp_index.data(), mask[i].data(), s->h_p2d.data(), s->h_p3d.data(),
                                st.sigma2.data(), st.fx, st.fy, st.cx, st.cy, frames[e].u_right, frames[e].bf,
                                per_candidate[i].T);
                jobs.push_back(Job{e, i});
            }
            if (jobs.empty()) break;
            std::vector<rsc_poseopt_result> res(jobs.size());
            if (int st = rsc_pose_optimization_many(C, B.problems.data(), (int)jobs.size(), res.data(), B.outlier.data()))
                return st;
            struct Chain {
                size_t q;  // its job
                std::vector<int32_t> mp;
                std::vector<uint8_t> found;
            };
            std::vector<Chain> chains;
            for (size_t q = 0; q < jobs.size(); ++q) {
                const Job& j = jobs[q];
                rsc_reloc_gate_result& g = per_event[j.e];
                g.gates++;
                const int nGood = res[q].n_good;
                if (nGood < 10) {  // Tracking.cpp:1286-1287: continue with the next candidate
                    g.rejected++;
                    continue;
                }
                Chain ch;
                if (refine) {
                    // mvpMapPoints after :1289-1291 as KeyFrame slots, and sFound (:1278, every inlier)
                    const rsc_pnp* s = solvers[j.i];
                    const rsc_reloc_candidate& cd = refine->cands[j.i];
                    ch.q = q;
                    ch.mp.assign((size_t)std::max(s->st.N_points, 1), -1);
                    ch.found.assign((size_t)std::max(cd.kf->n, 1), 0);
                    for (int c = 0; c < s->st.N; ++c) {
                        const int slot = s->st.kp_index[c];
                        if (!mask[j.i][slot]) continue;
                        const int32_t ks = cd.matches[slot];
                        if (ks < 0 || ks >= cd.kf->n) {
                            g_last_error = "a RANSAC inlier's Frame slot has no KeyFrame slot in the candidate's matches";
                            return RSC_ERR_ARG;
                        }
                        ch.found[ks] = 1;
                        if (!B.outlier[q][slot]) ch.mp[slot] = ks;
                    }
                    rsc_reloc_refined_result& x = refine->per_event[j.e];
                    if (nGood < 50) {  // :1294: the chain decides
                        chains.push_back(std::move(ch));
                        continue;
                    }
                    x.n_good_first = nGood;
                    x.n_additional[0] = x.n_additional[1] = -1;
                }
                accept(j, nGood >= 50 ? RSC_GATE_MATCH : RSC_GATE_HANDOFF, nGood, res[q].Tcw, ch.mp.data());
                if (outlier && outlier[j.e]) std::memcpy(outlier[j.e], B.outlier[q], (size_t)solvers[j.i]->st.N_points);
            }
            if (!chains.empty()) {  // Tracking.cpp:1294-1323 on this pass's successes with 10 <= nGood < 50
                const size_t m = chains.size();
                std::vector<rsc_frameview*> F(m);
                std::vector<rsc_kfview*> K(m);
                std::vector<rsc_reloc_frame> fr(m);
                std::vector<int32_t*> mp(m);
                std::vector<const uint8_t*> fnd(m);
                std::vector<int32_t> ng(m);
                std::vector<float> T(16 * m);
                std::vector<rsc_reloc_refine_result> rr(m);
                for (size_t k = 0; k < m; ++k) {
                    const Job& j = jobs[chains[k].q];
                    F[k] = refine->views[j.e];
                    K[k] = refine->cands[j.i].kf;
                    fr[k] = frames[j.e];
                    mp[k] = chains[k].mp.data();
                    fnd[k] = chains[k].found.data();
                    ng[k] = res[chains[k].q].n_good;
                    std::memcpy(&T[16 * k], res[chains[k].q].Tcw, 16 * sizeof(float));
                }
                if (int st = rsc_reloc_refine_many(C, F.data(), K.data(), (int)m, fr.data(), mp.data(), fnd.data(),
                                                   ng.data(), T.data(), rr.data()))
                    return st;
                for (size_t k = 0; k < m; ++k) {
                    const Job& j = jobs[chains[k].q];
                    rsc_reloc_gate_result& g = per_event[j.e];
                    rsc_reloc_refined_result& x = refine->per_event[j.e];
                    x.chains++;
                    if (rr[k].n_good < 50) {  // :1327 fails: the next success of the round
                        g.rejected++;
                        continue;
                    }
                    x.n_good_first = ng[k];
                    x.n_additional[0] = rr[k].n_additional[0];
                    x.n_additional[1] = rr[k].n_additional[1];
                    accept(j, RSC_GATE_MATCH, rr[k].n_good, rr[k].Tcw, chains[k].mp.data());
                }
            }
        }
        R.close();
    }
    return RSC_OK;
}
}  // namespace

int rsc_reloc_events_gated(rsc_pnp* const* solvers, const int32_t* event_begin, int n_events,
                           const rsc_reloc_frame* frames, rsc_pnp_result* per_candidate,
                           rsc_reloc_gate_result* per_event, uint8_t* const* outlier, uint8_t* const* inliers) {
    return reloc_events_gated_impl(solvers, event_begin, n_events, frames, per_candidate, per_event, outlier,
                                   inliers, nullptr);
}

int rsc_reloc_events_refined(rsc_pnp* const* solvers, const rsc_reloc_candidate* candidates,
                             const int32_t* event_begin, int n_events, rsc_frameview* const* views,
                             const rsc_reloc_frame* frames, rsc_pnp_result* per_candidate,
                             rsc_reloc_refined_result* per_event, int32_t* const* frame_mp_out) {
    if (n_events <= 0) return RSC_OK;
    if (!solvers || !candidates || !event_begin || !views || !frames || !per_candidate || !per_event)
        return RSC_ERR_ARG;
    for (int e = 0; e < n_events; ++e) {
        if (event_begin[e + 1] < event_begin[e] || event_begin[e] < 0) return RSC_ERR_ARG;
        if (event_begin[e + 1] > event_begin[e] && !views[e]) return RSC_ERR_ARG;
        for (int i = event_begin[e]; i < event_begin[e + 1]; ++i) {
            if (!solvers[i] || !candidates[i].kf || !candidates[i].matches) return RSC_ERR_ARG;
            if (solvers[i]->st.N_points != views[e]->n || candidates[i].kf->ctx != solvers[i]->ctx ||
                views[e]->ctx != solvers[i]->ctx)
                return RSC_ERR_ARG;
            if (!candidates[i].kf->has_angles) return RSC_ERR_ARG;  // matcher2(0.9, true) checks orientation
        }
        std::memset(&per_event[e], 0, sizeof(per_event[e]));
        per_event[e].n_additional[0] = per_event[e].n_additional[1] = -1;
    }
    std::vector<rsc_reloc_gate_result> g((size_t)n_events);
    const RelocRefine rf{candidates, views, per_event, frame_mp_out};
    const int st = reloc_events_gated_impl(solvers, event_begin, n_events, frames, per_candidate, g.data(), nullptr,
                                           nullptr, &rf);
    if (st) return st;
    // status .. gates: the records begin alike
    static_assert(offsetof(rsc_reloc_refined_result, n_good_first) == offsetof(rsc_reloc_gate_result, Tcw), "gate record");
    for (int e = 0; e < n_events; ++e) {
        std::memcpy(&per_event[e], &g[e], offsetof(rsc_reloc_gate_result, Tcw));
        std::memcpy(per_event[e].Tcw, g[e].Tcw, sizeof(g[e].Tcw));
    }
    return RSC_OK;
}

// LoopClosing::ComputeSim3 (LoopClosing.cpp:268-329): a candidate's k-th success comes back from the
// call that reaches it (Sim3Solver::iterate returns at the first hypothesis with more than
// mRansacMinInliers inliers, Sim3Solver.cpp:155-163), so with its own stream each candidate's
// successes are computed one at a time, each with the whole remaining budget in one call, and placed
// in the round-robin: a call starting at hypothesis p in round c covers p..p+4, so the success at
// hypothesis s is returned in round c + (s - p) / 5 and the next call starts at s + 1 in the round
// after.  The event takes its successes in (round, candidate) order: SearchBySim3(7.5) on the inliers
// (:296-309), OptimizeSim3(gScm = Sim3(R, t, 1), 10) (:310-311), accepted when nInliers >= 20
// (:314-325); a rejected candidate's next success is computed and the walk goes on.  Each pass gates
// one success per unresolved event (one launch of each stage over all of them).
int rsc_loop_events_gated(rsc_sim3* const* solvers, const rsc_loop_candidate* cands, const int32_t* event_begin,
                          int n_events, rsc_sim3_result* per_candidate, rsc_loop_gate_result* per_event,
                          int32_t* const* matches_out) {
    if (n_events <= 0) return RSC_OK;
    if (!solvers || !cands || !event_begin || !per_candidate || !per_event) return RSC_ERR_ARG;
    const int total = event_begin[n_events];
    rsc_context* C = nullptr;
    for (int e = 0; e < n_events; ++e) {
        if (event_begin[e + 1] < event_begin[e] || event_begin[e] < 0) return RSC_ERR_ARG;
        rsc_loop_gate_result& r = per_event[e];
        std::memset(&r, 0, sizeof(r));
        r.status = RSC_GATE_NONE;
        r.winner = r.round = r.hypothesis = -1;
        for (int i = event_begin[e]; i < event_begin[e + 1]; ++i) {
            const rsc_loop_candidate& k = cands[i];
            if (!solvers[i] || !k.kf1 || !k.kf2) return RSC_ERR_ARG;
            if (solvers[i]->stream) return RSC_ERR_UNSUPPORTED;
            if (!C) C = solvers[i]->ctx;
            if (solvers[i]->ctx != C || k.kf1->ctx != C || k.kf2->ctx != C) return RSC_ERR_ARG;
            if (solvers[i]->st.mN1 != k.kf1->n || (k.kf1->n > 0 && !k.matches12)) return RSC_ERR_ARG;
            if (k.kf1 != cands[event_begin[e]].kf1) return RSC_ERR_ARG;  // one mpCurrentKF per event
            for (int a = 0; a < k.kf1->n; ++a)
                if (k.matches12[a] < -2 || k.matches12[a] >= k.kf2->n) return RSC_ERR_ARG;
        }
    }
    if (!C) return RSC_OK;
    std::vector<int32_t> start_it(total), pos(total), calls(total, 0), s_round(total, -1);
    std::vector<std::vector<uint8_t>> mask(total);
    for (int i = 0; i < total; ++i) {
        start_it[i] = pos[i] = solvers[i]->st.mnIterations;
        mask[i].assign((size_t)std::max(solvers[i]->st.mN1, 1), 0);
    }
    // the next success of each listed candidate (s_round = its round, -1: none left)
    auto refill = [&](const std::vector<int>& list) -> int {
        if (list.empty()) return RSC_OK;
        std::vector<rsc_sim3*> act;
        std::vector<int32_t> its;
        std::vector<uint8_t*> mp;
        for (int i : list) {
            act.push_back(solvers[i]);
            its.push_back(std::max(1, solvers[i]->st.mRansacMaxIts - solvers[i]->st.mnIterations));
            mp.push_back(mask[i].data());
        }
        std::vector<rsc_sim3_result> r(act.size());
        if (int st = rsc_sim3_iterate_many(act.data(), (int)act.size(), its.data(), r.data(), mp.data())) return st;
        for (size_t q = 0; q < list.size(); ++q) {
            const int i = list[q];
            per_candidate[i] = r[q];
            if (!r[q].ok) {
                s_round[i] = -1;
                continue;
            }
            const int s = r[q].iterations - 1;
            s_round[i] = calls[i] + (s - pos[i]) / 5;
            pos[i] = s + 1;
            calls[i] = s_round[i] + 1;
        }
        return RSC_OK;
    };
    {
        std::vector<int> all(total);
        for (int i = 0; i < total; ++i) all[i] = i;
        if (int st = refill(all)) return st;
    }
    std::vector<char> resolved(n_events, 0);
    for (;;) {
        std::vector<int> ev, ci;  // one gate job per unresolved event: its smallest (round, candidate)
        for (int e = 0; e < n_events; ++e) {
            if (resolved[e]) continue;
            int best = -1;
            for (int i = event_begin[e]; i < event_begin[e + 1]; ++i)
                if (s_round[i] >= 0 && (best < 0 || s_round[i] < s_round[best])) best = i;
            if (best < 0) {
                resolved[e] = 1;  // every candidate discarded: bMatch stays false
                continue;
            }
            ev.push_back(e);
            ci.push_back(best);
        }
        const int J = (int)ev.size();
        if (J == 0) break;
        // SearchBySim3 over the RANSAC inliers (vpMapPointMatches[j] = inlier ? match : NULL)
        std::vector<rsc_kfview*> k1(J), k2(J);
        std::vector<float> R12(9 * (size_t)J), t12(3 * (size_t)J);
        std::vector<std::vector<int32_t>> m12(J), o12(J);
        std::vector<const int32_t*> m12p(J);
        std::vector<int32_t*> o12p(J);
        std::vector<int32_t> nfound(J, 0);
        for (int q = 0; q < J; ++q) {
            const int i = ci[q];
            const rsc_loop_candidate& k = cands[i];
            k1[q] = k.kf1;
            k2[q] = k.kf2;
            std::memcpy(&R12[9 * (size_t)q], per_candidate[i].R, 9 * sizeof(float));
            std::memcpy(&t12[3 * (size_t)q], per_candidate[i].t, 3 * sizeof(float));
            const int n1 = k.kf1->n;
            m12[q].assign((size_t)std::max(n1, 1), -1);
            o12[q].assign((size_t)std::max(n1, 1), -1);
            for (int a = 0; a < n1; ++a) m12[q][a] = mask[i][a] ? k.matches12[a] : -1;
            m12p[q] = m12[q].data();
            o12p[q] = o12[q].data();
        }
        if (int st = rsc_search_by_sim3_many(C, k1.data(), k2.data(), J, R12.data(), t12.data(), 7.5f, m12p.data(),
                                             o12p.data(), nfound.data()))
            return st;
        // OptimizeSim3 on vpMapPointMatches after the search (Optimizer.cpp:1108-1171 slot rules)
        std::vector<rsc_sim3opt_problem> pr(J);
        std::vector<rsc_sim3opt_result> res(J);
        std::vector<std::vector<uint8_t>> valid(J), keep(J);
        std::vector<std::vector<float>> X1(J), X2(J), u1(J), u2(J), i1(J), i2(J);
        std::vector<uint8_t*> keepp(J);
        for (int q = 0; q < J; ++q) {
            const int i = ci[q];
            const rsc_kfview& a = *cands[i].kf1;
            const rsc_kfview& b = *cands[i].kf2;
            const int n1 = a.n;
            for (int x = 0; x < n1; ++x)
                if (o12[q][x] >= 0) m12[q][x] = o12[q][x];  // vpMatches12[i1] = vpMapPoints2[idx2]
            valid[q].assign((size_t)std::max(n1, 1), 0);
            keep[q].assign((size_t)std::max(n1, 1), 1);
            X1[q].assign(3 * (size_t)std::max(n1, 1), 0.f);
            X2[q].assign(3 * (size_t)std::max(n1, 1), 0.f);
            u1[q].assign(2 * (size_t)std::max(n1, 1), 0.f);
            u2[q].assign(2 * (size_t)std::max(n1, 1), 0.f);
            i1[q].assign((size_t)std::max(n1, 1), 0.f);
            i2[q].assign((size_t)std::max(n1, 1), 0.f);
            for (int x = 0; x < n1; ++x) {
                const int y = m12[q][x];
                // vpMatches1[i] set, pMP1 set, neither bad, i2 = GetIndexInKeyFrame(pKF2) >= 0
                if (y < 0 || a.mp_state[x] != 1 || b.mp_state[y] != 1) continue;
                valid[q][x] = 1;
                for (int c = 0; c < 3; ++c) {
                    X1[q][3 * x + c] = a.mp_pos[3 * x + c];
                    X2[q][3 * x + c] = b.mp_pos[3 * (size_t)y + c];
                }
                u1[q][2 * x] = a.kp[2 * x];
                u1[q][2 * x + 1] = a.kp[2 * x + 1];
                u2[q][2 * x] = b.kp[2 * (size_t)y];
                u2[q][2 * x + 1] = b.kp[2 * (size_t)y + 1];
                const int o1 = a.octave[x], o2 = b.octave[y];
                if (o1 < 0 || o1 >= (int)a.inv_level_sigma2.size() || o2 < 0 || o2 >= (int)b.inv_level_sigma2.size())
                    return RSC_ERR_ARG;
                i1[q][x] = a.inv_level_sigma2[o1];
                i2[q][x] = b.inv_level_sigma2[o2];
            }
            rsc_sim3opt_problem& P = pr[q];
            P.n = n1;
            P.valid = valid[q].data();
            P.X1w = X1[q].data();
            P.X2w = X2[q].data();
            P.uv1 = u1[q].data();
            P.uv2 = u2[q].data();
            P.inv1 = i1[q].data();
            P.inv2 = i2[q].data();
            std::memcpy(P.R1w, a.R, sizeof(P.R1w));
            std::memcpy(P.t1w, a.t, sizeof(P.t1w));
            std::memcpy(P.R2w, b.R, sizeof(P.R2w));
            std::memcpy(P.t2w, b.t, sizeof(P.t2w));
            std::memcpy(P.K1, a.K, sizeof(P.K1));
            std::memcpy(P.K2, b.K, sizeof(P.K2));
            // g2o::Sim3 gScm(R.cast<double>(), t.cast<double>(), 1.0): Quaterniond(R), no normalisation
            double Rd[3][3];
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) Rd[r][c] = (double)per_candidate[i].R[3 * r + c];
            const PoQuat qq = po_quat_from_R(Rd);
            P.S[0] = qq.x; P.S[1] = qq.y; P.S[2] = qq.z; P.S[3] = qq.w;
            for (int c = 0; c < 3; ++c) P.S[4 + c] = (double)per_candidate[i].t[c];
            P.S[7] = 1.0;
            P.th2 = 10.0f;
            keepp[q] = keep[q].data();
        }
        if (int st = rsc_optimize_sim3_many(C, pr.data(), J, res.data(), keepp.data())) return st;
        std::vector<int> again;
        for (int q = 0; q < J; ++q) {
            const int e = ev[q], i = ci[q];
            rsc_loop_gate_result& g = per_event[e];
            if (res[q].n_inliers < 20) {  // LoopClosing.cpp:314: not accepted, the round-robin goes on
                g.rejected++;
                again.push_back(i);
                continue;
            }
            g.status = RSC_GATE_MATCH;
            fill_winner(g, i - event_begin[e], s_round[i], per_candidate[i], start_it[i]);
            g.n_found = nfound[q];
            g.n_opt_inliers = res[q].n_inliers;
            std::memcpy(g.S, res[q].S, sizeof(g.S));
            if (matches_out && matches_out[e]) {
                const int n1 = cands[i].kf1->n;
                for (int x = 0; x < n1; ++x) matches_out[e][x] = keep[q][x] ? m12[q][x] : -1;  // outliers NULLed
            }
            resolved[e] = 1;
        }
        if (int st = refill(again)) return st;
    }
    return RSC_OK;
}

// LoopClosing.cpp:318-320 and :360-370 (rsc_sim3compose.h)
int rsc_loop_verify_many(rsc_context* C, rsc_kfview* const* kf_cur, rsc_kfview* const* kf_matched,
                         rsc_mpview* const* loop_points, int count, const double* S,
                         const int32_t* const* matches, const uint8_t* const* already,
                         rsc_loop_verify_result* res, int32_t* const* projected) {
    if (!C || count < 0) return RSC_ERR_ARG;
    if (count == 0) return RSC_OK;
    if (!kf_cur || !kf_matched || !loop_points || !S || !matches || !already || !res) return RSC_ERR_ARG;
    std::vector<float> Scw(16 * (size_t)count);
    std::vector<std::vector<uint8_t>> occ(count);
    std::vector<std::vector<int32_t>> outs(count);
    std::vector<const uint8_t*> occp(count);
    std::vector<int32_t*> outp(count);
    std::vector<int32_t> nm(count);
    for (int c = 0; c < count; ++c) {
        if (!kf_cur[c] || !kf_matched[c] || kf_matched[c]->ctx != C) return RSC_ERR_ARG;
        const int n = kf_cur[c]->n;
        if (n && !matches[c]) return RSC_ERR_ARG;
        const SoSim3 gScm = sc_sim3_from_array(S + 8 * (size_t)c);
        const SoSim3 gSmw = sc_sim3_from_pose(kf_matched[c]->R, kf_matched[c]->t);  // :318
        const SoSim3 gScw = sc_compose(gScm, gSmw);                                  // :319
        sc_sim3_to_array(gScw, res[c].Scw_sim3);
        sc_to_iso(gScw, res[c].Scw);                                                 // :320
        std::memcpy(&Scw[16 * (size_t)c], res[c].Scw, sizeof(res[c].Scw));
        occ[c].assign((size_t)std::max(n, 1), 0);
        for (int i = 0; i < n; ++i) occ[c][i] = matches[c][i] != -1;  // -2 is a non-null pointer
        outs[c].assign((size_t)std::max(n, 1), -1);
        occp[c] = occ[c].data();
        outp[c] = outs[c].data();
    }
    if (int st = rsc_search_by_projection_kf_many(C, kf_cur, loop_points, count, Scw.data(), already, occp.data(),
                                                  10, outp.data(), nm.data(), nullptr))  // :360
        return st;
    for (int c = 0; c < count; ++c) {
        const int n = kf_cur[c]->n;
        int total = nm[c];
        for (int i = 0; i < n; ++i) total += occ[c][i];  // :363-368
        res[c].n_projected = nm[c];
        res[c].n_total = total;
        res[c].accepted = total >= 40;  // :370
        if (projected && projected[c] && n) std::memcpy(projected[c], outs[c].data(), 4 * (size_t)n);
    }
    return RSC_OK;
}

// Tracking::TrackWithMotionModel (Tracking.cpp:724-774); each stage one launch over the frames still in it.
int rsc_track_motion_model_many(rsc_context* C, rsc_frameview* const* frames, rsc_lastframe* const* lasts, int count,
                                const float* Tcw_cur, const float* Tcw_last, const float* mb, float th,
                                const int32_t* only_tracking, rsc_track_motion_result* result, int32_t* const* out,
                                int32_t* const* discarded) {
    if (!C || count < 0 || count > 65535) return RSC_ERR_ARG;
    if (count == 0) return RSC_OK;
    if (!frames || !lasts || !Tcw_cur || !Tcw_last || !mb || !only_tracking || !result || !out || !discarded)
        return RSC_ERR_ARG;
    if (int e = last_check_args(C, frames, lasts, count, th)) return e;
    if (int e = last_check_args(C, frames, lasts, count, 2.0f * th)) return e;
    for (int c = 0; c < count; ++c)
        if (frames[c]->n && (!out[c] || !discarded[c])) return RSC_ERR_ARG;
    std::vector<int32_t> nm(count), md(count);
    // :724-732: from an empty mvpMapPoints (frame_occ NULL)
    if (int st = rsc_search_by_projection_last_many(C, frames, lasts, count, Tcw_cur, Tcw_last, mb, nullptr, th, 1,
                                                    out, nm.data(), md.data(), nullptr))
        return st;
    std::vector<int> again, opt;
    for (int c = 0; c < count; ++c) {
        rsc_track_motion_result& r = result[c];
        std::memset(&r, 0, sizeof(r));
        r.searches = 1;
        r.nmatches_search[0] = nm[c];
        r.nmatches_search[1] = -1;
        r.mode = md[c];
        r.nmatches = nm[c];
        std::memcpy(r.Tcw, Tcw_cur + 16 * (size_t)c, sizeof(r.Tcw));
        for (int f = 0; f < frames[c]->n; ++f) discarded[c][f] = -1;
        if (nm[c] < 20) again.push_back(c);  // :735
    }
    if (!again.empty()) {  // :737-738: again from empty, at 2 * th
        const int m = (int)again.size();
        std::vector<rsc_frameview*> F = gather(frames, again);
        std::vector<rsc_lastframe*> L = gather(lasts, again);
        std::vector<float> Tc = gather(Tcw_cur, again, 16), Tl = gather(Tcw_last, again, 16), b = gather(mb, again);
        std::vector<int32_t*> op = gather(out, again);
        std::vector<int32_t> nm2(m);
        if (int st = rsc_search_by_projection_last_many(C, F.data(), L.data(), m, Tc.data(), Tl.data(), b.data(),
                                                        nullptr, 2.0f * th, 1, op.data(), nm2.data(), nullptr, nullptr))
            return st;
        for (int q = 0; q < m; ++q) {
            rsc_track_motion_result& r = result[again[q]];
            r.searches = 2;
            r.nmatches_search[1] = nm2[q];
            r.nmatches = nm2[q];
        }
    }
    for (int c = 0; c < count; ++c) {
        for (int f = 0; f < frames[c]->n; ++f)
            if (out[c][f] < 0) out[c][f] = -1;  // a slot the rotation check nulled is empty
        if (result[c].nmatches >= 20) opt.push_back(c);  // :741
    }
    if (opt.empty()) return RSC_OK;
    // :745 Optimizer::PoseOptimization(&mCurrentFrame) on every occupied slot
    const int m = (int)opt.size();
    PoseOptBatch B;
    for (int c : opt) {
        const rsc_frameview& F = *frames[c];
        B.add_slots(F.n, out[c], lasts[c]->mp_pos.data(), F.kp.data(), F.octave.data(), F.inv_level_sigma2.data(), F.K,
                    F.h_uright.data(), F.mbf, result[c].Tcw);
    }
    std::vector<rsc_poseopt_result> res(m);
    if (int st = rsc_pose_optimization_many(C, B.problems.data(), m, res.data(), B.outlier.data())) return st;
    for (int q = 0; q < m; ++q) {
        const int c = opt[q];
        const rsc_lastframe& L = *lasts[c];
        rsc_track_motion_result& r = result[c];
        r.n_good = res[q].n_good;
        std::memcpy(r.Tcw, res[q].Tcw, sizeof(r.Tcw));
        int map = 0;
        for (int f = 0; f < frames[c]->n; ++f) {  // :749-766
            const int32_t s = out[c][f];
            if (s < 0) continue;
            if (B.outlier[q][f]) {
                discarded[c][f] = s;
                out[c][f] = -1;
                r.nmatches--;
            } else if (L.mp_has_obs[s]) {
                ++map;
            }
        }
        r.nmatches_map = map;
        if (only_tracking[c]) {  // :768-772
            r.vo = map < 10;
            r.ok = r.nmatches > 20;
        } else {
            r.ok = map >= 10;  // :774
        }
    }
    return RSC_OK;
}

// LocalMapping::CreateNewMapPoints' neighbour loop (LocalMapping.cpp:224-428), speculated on the device and
// replayed on the host (the shape of the RANSAC engine).
//
// Why the replay is exact.  The loop over neighbours is sequential only through the current KeyFrame's slots: a
// successful triangulation fills slot idx1 (:415) and the next neighbour's matcher skips a filled slot before
// anything else (ORBmatcher.cpp:531-535).  Inside one SearchForTriangulation call a slot is decided alone:
// vbMatched2 is never set (read at :567, written nowhere), and with the orientation check off (ORBmatcher
// matcher(0.6, false), :202) no histogram couples the slots.  So the match, the den == 0 flag and the
// triangulation of (neighbour i, slot s) computed from the INITIAL slot state are the ones the reference
// computes whenever it reaches s with the slot still empty, and are never looked at otherwise.  The neighbour's
// own slots change only after its matcher returned (:416), and a covisibility list names a KeyFrame once.  The
// replay walks the neighbours in order: a neighbour is void when one of its den == 0 slots is still empty
// (`return false` leaves vMatchedIndices empty); otherwise every match on a still-empty slot whose
// triangulation succeeded is emitted in ascending idx1 and fills the slot.  The problems of one call are each
// evaluated from the views' state at the call.
int rsc_create_new_map_points_many(rsc_context* C, const rsc_bow* const* bow_cur, rsc_kfview* const* kf_cur, int count,
                                   const int32_t* neigh_begin, const rsc_bow* const* bow_neigh,
                                   rsc_kfview* const* kf_neigh, int32_t* const* new_neighbour,
                                   int32_t* const* new_idx2, float* const* new_pos, int32_t* nnew) {
    if (!C || count < 0) return RSC_ERR_ARG;
    if (count == 0) return RSC_OK;
    if (!bow_cur || !kf_cur || !neigh_begin || !new_neighbour || !new_idx2 || !new_pos || !nnew) return RSC_ERR_ARG;
    if (neigh_begin[0] != 0) return RSC_ERR_ARG;
    for (int c = 0; c < count; ++c)
        if (neigh_begin[c + 1] < neigh_begin[c]) return RSC_ERR_ARG;
    const int total = neigh_begin[count];
    if (total && (!bow_neigh || !kf_neigh)) return RSC_ERR_ARG;
    auto usable = [&](const rsc_kfview* k) {
        if (!k || k->ctx != C) return false;
        if (!k->has_triang) g_last_error = "a KeyFrame view without rsc_kfview_set_triangulation";
        return k->has_triang;
    };
    for (int c = 0; c < count; ++c) {
        if (!usable(kf_cur[c]) || !bow_cur[c]) return RSC_ERR_ARG;
        if (kf_cur[c]->n && (!new_neighbour[c] || !new_idx2[c] || !new_pos[c])) return RSC_ERR_ARG;
    }
    for (int g = 0; g < total; ++g)
        if (!usable(kf_neigh[g]) || !bow_neigh[g]) return RSC_ERR_ARG;
    // the baseline gate (:232-236) and ComputeF12 (:512-531) on the host
    std::vector<int> sel_c, sel_g;
    std::vector<float> F;
    for (int c = 0; c < count; ++c)
        for (int g = neigh_begin[c]; g < neigh_begin[c + 1]; ++g) {
            const rsc_kfview& k1 = *kf_cur[c];
            const rsc_kfview& k2 = *kf_neigh[g];
            if (tri_baseline_short(k1.tri.Ow, k2.tri.Ow, k2.tri.mb)) continue;
            float f[9];
            tri_compute_f12(k1.R, k1.t, k2.tri.Rwc, k2.tri.Ow, k1.Kinv, k2.Kinv, f);
            F.insert(F.end(), f, f + 9);
            sel_c.push_back(c);
            sel_g.push_back(g);
        }
    const int J = (int)sel_c.size();
    std::vector<std::vector<int32_t>> m((size_t)J), pairs((size_t)J), status((size_t)J);
    std::vector<std::vector<uint8_t>> dzs((size_t)J);
    std::vector<std::vector<float>> x3d((size_t)J);
    if (J) {
        // one matcher launch over every (problem, neighbour) that passed the gate, from the initial slots
        std::vector<const rsc_bow*> b1(J), b2(J);
        std::vector<rsc_kfview*> k1(J), k2(J);
        std::vector<int32_t*> mp(J);
        std::vector<uint8_t*> dp(J);
        for (int j = 0; j < J; ++j) {
            b1[j] = bow_cur[sel_c[j]];
            k1[j] = kf_cur[sel_c[j]];
            b2[j] = bow_neigh[sel_g[j]];
            k2[j] = kf_neigh[sel_g[j]];
            const size_t n1 = (size_t)std::max(k1[j]->n, 1);
            m[j].assign(n1, -1);
            dzs[j].assign(n1, 0);
            mp[j] = m[j].data();
            dp[j] = dzs[j].data();
        }
        if (int st = tri_search_impl(C, b1.data(), k1.data(), b2.data(), k2.data(), J, F.data(), nullptr, nullptr,
                                     /*only_stereo=*/nullptr, /*check_orientation=*/0, /*speculative=*/1, mp.data(), nullptr,
                                     nullptr, dp.data()))
            return st;
        // one triangulation launch over all matches
        std::vector<int32_t> np(J);
        std::vector<const int32_t*> pp(J);
        std::vector<int32_t*> sp(J);
        std::vector<float*> xp(J);
        for (int j = 0; j < J; ++j) {
            for (int i = 0; i < k1[j]->n; ++i)
                if (m[j][i] >= 0) {
                    pairs[j].push_back(i);
                    pairs[j].push_back(m[j][i]);
                }
            np[j] = (int32_t)(pairs[j].size() / 2);
            status[j].assign((size_t)std::max(np[j], 1), -1);
            x3d[j].assign(3 * (size_t)std::max(np[j], 1), 0.0f);
            pp[j] = pairs[j].data();
            sp[j] = status[j].data();
            xp[j] = x3d[j].data();
        }
        if (int st = rsc_triangulate_pairs_many(C, k1.data(), k2.data(), J, np.data(), pp.data(), sp.data(), xp.data()))
            return st;
    }
    // the replay: neighbours in order, slots filled as the reference fills them
    int j = 0;
    for (int c = 0; c < count; ++c) {
        const rsc_kfview& k1 = *kf_cur[c];
        std::vector<uint8_t> filled(k1.mp_state.size());
        for (size_t i = 0; i < filled.size(); ++i) filled[i] = k1.mp_state[i] != 0;
        for (int i = 0; i < k1.n; ++i) {
            new_neighbour[c][i] = -1;
            new_idx2[c][i] = -1;
            new_pos[c][3 * i] = new_pos[c][3 * i + 1] = new_pos[c][3 * i + 2] = 0.0f;
        }
        nnew[c] = 0;
        for (; j < J && sel_c[j] == c; ++j) {
            bool voided = false;
            for (int i = 0; i < k1.n && !voided; ++i) voided = dzs[j][i] && !filled[i];
            if (voided) continue;
            const int np = (int)(pairs[j].size() / 2);
            for (int k = 0; k < np; ++k) {
                const int i1 = pairs[j][2 * k];
                if (filled[i1] || status[j][k] != 0) continue;
                new_neighbour[c][i1] = sel_g[j] - neigh_begin[c];
                new_idx2[c][i1] = pairs[j][2 * k + 1];
                std::memcpy(new_pos[c] + 3 * i1, x3d[j].data() + 3 * k, 12);
                filled[i1] = 1;
                ++nnew[c];
            }
        }
    }
    return RSC_OK;
}
}  // extern "C"
