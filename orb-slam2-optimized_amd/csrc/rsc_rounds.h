// rsc_rounds.h — the drivers' bookkeeping (rsc_drivers.cpp): the event round-robin, the shared-stream
// events on it, the PoseOptimization batch and the row gather.  Host only, no HIP include: it builds
// with a plain C++ compiler (tests/cpp/rounds_test.cpp).
#pragma once
#include <deque>
#include "../../include/rsc.h"
#include "rsc_engine.h"  // and <algorithm>, <cstdint>, <cstring>, <vector>

namespace rsc {
#pragma GCC visibility push(hidden)  // private to librsc
// rand() draws per hypothesis: mRansacMinSet RandomInt calls (PnPsolver.cpp:125-131,
// MLPnPsolver.cpp:84-92), 3 for Sim3 (Sim3Solver.cpp:140-147).
inline int draws_per_hypothesis(const PnPState& s) { return s.mRansacMinSet; }
inline int draws_per_hypothesis(const Sim3State&) { return 3; }
inline int draws_per_hypothesis(const MLState& s) { return s.mRansacMinSet; }

// rows[sel[0]], rows[sel[1]], ...: the per-problem arguments of a sub-call over a subset of a batch
// (`width` elements per row, concatenated)
template <class T>
std::vector<T> gather(const T* rows, const std::vector<int>& sel, size_t width = 1) {
    std::vector<T> out(sel.size() * width);
    for (size_t q = 0; q < sel.size(); ++q)
        for (size_t k = 0; k < width; ++k) out[width * q + k] = rows[width * (size_t)sel[q] + k];
    return out;
}

// The winner record of an event (rsc_event_result and the gate results that begin like it); start_it
// is the candidate's mnIterations when the event began.
template <class Rec, class Res>
void fill_winner(Rec& rec, int candidate, int round, const Res& r, int start_it) {
    rec.winner = candidate;
    rec.round = round;
    rec.hypothesis = r.iterations - 1 - start_it;
    rec.n_inliers = r.n_inliers;
}

// The round-robin of iterate(5) calls over the candidates of Tracking::Relocalization /
// LoopClosing::ComputeSim3 events (Tracking.cpp:1239-1262, LoopClosing.cpp:271-296): event e owns the
// candidates [begin[e], begin[e + 1]).  Per round: collect() lists the live candidates of the
// unresolved events; the caller runs them in one call and hands each record to take(); win() resolves
// an event on a success; close() resolves the events that have no live candidate left.
struct EventRounds {
    const int32_t* begin;
    int n_events, total;
    int round = -1;                     // the round collect() opened last
    std::vector<char> discarded, resolved;
    std::vector<int32_t> start_it;      // mnIterations of each candidate when the events began
    std::vector<int> idx;               // this round's candidates, in event and candidate order
    std::vector<int> slot;              // [total] a candidate's place in idx, -1: not iterated this round

    template <class Solver>
    EventRounds(Solver* const* solvers, const int32_t* event_begin, int n)
        : begin(event_begin), n_events(n), total(event_begin[n]), discarded(total, 0), resolved(n, 0),
          start_it(total), slot(total, -1) {
        for (int i = 0; i < total; ++i) start_it[i] = solvers[i]->st.mnIterations;
    }
    // Opens the next round; false when no candidate is left to iterate.
    bool collect() {
        ++round;
        idx.clear();
        std::fill(slot.begin(), slot.end(), -1);
        for (int e = 0; e < n_events; ++e) {
            if (resolved[e]) continue;
            for (int i = begin[e]; i < begin[e + 1]; ++i)
                if (!discarded[i]) {
                    slot[i] = (int)idx.size();
                    idx.push_back(i);
                }
        }
        return !idx.empty();
    }
    // The record of candidate idx[q]'s call: kept as the candidate's last result; bNoMore discards it
    // (Tracking.cpp:1257-1261, LoopClosing.cpp:292-296).
    template <class Res>
    void take(int q, const Res& r, Res* per_candidate) {
        per_candidate[idx[q]] = r;
        if (r.no_more) discarded[idx[q]] = 1;
    }
    // The first candidate of event e at or after `from` that this round iterated with success;
    // begin[e + 1] when there is none.
    template <class Res>
    int next_success(int e, int from, const Res* per_candidate) const {
        int i = from;
        while (i < begin[e + 1] && !(slot[i] >= 0 && per_candidate[i].ok)) ++i;
        return i;
    }
    // Candidate i's success of this round resolves event e.
    template <class Rec, class Res>
    void win(int e, int i, const Res& r, Rec& rec) {
        fill_winner(rec, i - begin[e], round, r, start_it[i]);
        resolved[e] = 1;
    }
    // End of a round: nCandidates == 0 ends the event's while loop (Tracking.cpp:1239).
    void close() {
        for (int e = 0; e < n_events; ++e)
            if (std::all_of(discarded.begin() + begin[e], discarded.begin() + begin[e + 1], [](char d) { return d != 0; }))
                resolved[e] = 1;
    }
};

// Events on the reference's shared rand() stream (Q3).  One round of the round-robin: every live
// candidate of every unresolved event runs iterate(5) in one set of launches.  A candidate's call
// starts where the previous candidate's call of its event ended, assuming every call runs its whole
// loop; the only call that ends early is a success, which resolves the event (Tracking.cpp:1284-1331 /
// LoopClosing.cpp:311-327 with the gate passed), so the candidates after it in that round are calls
// the reference never makes: their records are discarded (left as they were before the round) and the
// stream advances by the calls made.
// Solver: { ctx (with the RngTable `table`), st }; Stream: { ctx, st, position }; iter: iterate_many;
// pred_its(solver): the hypotheses its next iterate(5) runs unless it succeeds.
template <class Solver, class Stream, class Res, class IterFn, class PredFn>
int shared_events(Solver* const* solvers, const int32_t* event_begin, int n_events, Stream* const* streams,
                  Res* per_candidate, rsc_event_result* per_event, IterFn iter, PredFn pred_its) {
    if (n_events <= 0) return RSC_OK;
    if (!solvers || !event_begin || !streams || !per_candidate || !per_event) return RSC_ERR_ARG;
    const int total = event_begin[n_events];
    for (int e = 0; e < n_events; ++e) {
        if (event_begin[e + 1] < event_begin[e] || !streams[e] || streams[e]->ctx != streams[0]->ctx)
            return RSC_ERR_ARG;
        for (int f = 0; f < e; ++f)
            if (streams[f] == streams[e]) return RSC_ERR_ARG;  // one stream per event (calls of two events would interleave)
        per_event[e] = rsc_event_result{-1, -1, -1, 0};
    }
    for (int i = 0; i < total; ++i)
        if (!solvers[i] || solvers[i]->ctx != streams[0]->ctx) return RSC_ERR_ARG;
    // the calls draw from the event's stream; a solver's own stream (st.rng of an unbound one) is
    // parked here and resumes on every way out, a failed round included
    struct Parked {
        Solver* const* solvers;
        std::vector<RngStream> own;
        ~Parked() { for (size_t i = 0; i < own.size(); ++i) solvers[i]->st.rng = own[i]; }
    } parked{solvers, std::vector<RngStream>((size_t)total)};
    for (int i = 0; i < total; ++i) parked.own[i] = solvers[i]->st.rng;
    EventRounds R(solvers, event_begin, n_events);
    while (R.collect()) {
        for (int e = 0; e < n_events; ++e) {
            RngStream cur = streams[e]->st;  // call positions, assuming every call runs its whole loop
            for (int i = event_begin[e]; i < event_begin[e + 1]; ++i) {
                if (R.slot[i] < 0) continue;
                Solver* s = solvers[i];
                s->st.rng = cur;
                cur.advance(s->ctx->table, (int64_t)pred_its(s) * draws_per_hypothesis(s->st));
            }
        }
        std::vector<Solver*> act = gather(solvers, R.idx);
        std::vector<int32_t> its(act.size(), 5), it0(act.size());
        for (size_t q = 0; q < act.size(); ++q) it0[q] = act[q]->st.mnIterations;
        std::vector<Res> r(act.size());
        std::vector<uint8_t*> nomask(act.size(), nullptr);
        if (int st = iter(act.data(), (int)act.size(), its.data(), r.data(), nomask.data())) return st;
        for (int e = 0; e < n_events; ++e) {
            if (R.resolved[e]) continue;
            int64_t used = 0;
            for (int i = event_begin[e]; i < event_begin[e + 1]; ++i) {
                const int q = R.slot[i];
                if (q < 0) continue;  // discarded in an earlier round
                used += (int64_t)(act[q]->st.mnIterations - it0[q]) * draws_per_hypothesis(act[q]->st);
                R.take(q, r[q], per_candidate);
                if (r[q].ok) {
                    R.win(e, i, r[q], per_event[e]);
                    break;
                }
            }
            streams[e]->st.advance(streams[e]->ctx->table, used);
            streams[e]->position += used;
        }
        R.close();
    }
    return RSC_OK;
}

// A batch of Optimizer::PoseOptimization problems for one rsc_pose_optimization_many call.  It owns
// every per-problem array (each at least one element long, so never NULL); a deque holds them, so
// adding a problem moves no earlier problem's arrays and the pointers in `problems` stay valid.
struct PoseOptBatch {
    struct Arrays {
        std::vector<uint8_t> has_mp, outl;
        std::vector<float> uv, Xw, inv;
        Arrays(size_t m, bool own_uv) : has_mp(m, 0), outl(m, 0), uv(own_uv ? 2 * m : 0, 0.f), Xw(3 * m, 0.f), inv(m, 0.f) {}
    };
    std::deque<Arrays> arrays;
    std::vector<rsc_poseopt_problem> problems;
    std::vector<uint8_t*> outlier;  // rsc_pose_optimization_many's mvbOutlier outputs: arrays[q].outl

    // PoseOptimization(&mCurrentFrame) from a Frame view's slots: slot f holds the point
    // slot_point[f] of `pos` ([..][3]) or nothing (< 0); kp (the problem's uv), octave,
    // inv_level_sigma2 and K are the view's host copies.
    void add_slots(int n, const int32_t* slot_point, const float* pos, const float* kp, const int32_t* octave,
                   const float* inv_level_sigma2, const float* K, const float* u_right, float bf, const float* Tcw) {
        Arrays& a = open(n, false, kp, K[0], K[1], K[2], K[3], u_right, bf, Tcw);
        for (size_t f = 0; f < (size_t)n; ++f) {
            const int32_t s = slot_point[f];
            if (s < 0) continue;
            a.has_mp[f] = 1;
            for (int k = 0; k < 3; ++k) a.Xw[3 * f + k] = pos[3 * (size_t)s + k];
            a.inv[f] = inv_level_sigma2[octave[f]];
        }
    }
    // The relocalization gate's problem from a PnP solver's compacted arrays (Tracking.cpp:1268-1284):
    // mvpMapPoints[kp_index[c]] = inlier ? match c : NULL over the Frame's n_slots slots.
    void add_compacted(int n_slots, int n, const int32_t* kp_index, const uint8_t* inlier, const float* p2d,
                       const float* p3d, const float* sigma2, float fx, float fy, float cx, float cy,
                       const float* u_right, float bf, const float* Tcw) {
        Arrays& a = open(n_slots, true, nullptr, fx, fy, cx, cy, u_right, bf, Tcw);
        for (int c = 0; c < n; ++c) {
            const int slot = kp_index[c];
            if (!inlier[slot]) continue;  // mvpMapPoints[j] = inlier ? match : NULL (:1276-1282)
            a.has_mp[slot] = 1;
            a.uv[2 * slot] = p2d[2 * c];
            a.uv[2 * slot + 1] = p2d[2 * c + 1];
            for (int k = 0; k < 3; ++k) a.Xw[3 * slot + k] = p3d[3 * c + k];
            a.inv[slot] = 1.0f / sigma2[c];  // mvInvLevelSigma2 = 1.0f / mvLevelSigma2
        }
    }

private:
    // The next problem, every slot empty; own_uv: the batch holds its uv too.
    Arrays& open(int n, bool own_uv, const float* uv, float fx, float fy, float cx, float cy, const float* u_right,
                 float bf, const float* Tcw) {
        arrays.emplace_back((size_t)std::max(n, 1), own_uv);
        Arrays& a = arrays.back();
        rsc_poseopt_problem P;
        P.n = n;
        P.has_mp = a.has_mp.data();
        P.uv = own_uv ? a.uv.data() : uv;
        P.Xw = a.Xw.data();
        P.inv_sigma2 = a.inv.data();
        P.u_right = u_right;
        P.fx = fx; P.fy = fy; P.cx = cx; P.cy = cy;
        std::memcpy(P.Tcw, Tcw, sizeof(P.Tcw));
        P.bf = bf;
        problems.push_back(P);
        outlier.push_back(a.outl.data());
        return a;
    }
};

#pragma GCC visibility pop
}  // namespace rsc
