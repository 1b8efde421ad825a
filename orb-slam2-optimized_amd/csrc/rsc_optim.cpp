// rsc_optim.cpp — the LM optimisers of the C ABI: PoseOptimization, OptimizeSim3 and LocalBundleAdjustment.
#include <cstring>
#include "rsc_host.h"
#include "rsc_poseopt.h"
#include "rsc_sim3opt.h"
#include "rsc_localba.h"

constexpr int kSoCoopCUs = 256;  // OptimizeSim3's cooperative form: workgroups per launch at most (MI355X CUs)

namespace {

// The device backend of lba_drive (rsc_localba.h): one staging arena per problem —
//     edges | cameras | bad | the phase's plan                         uploaded (the plan again for the second phase)
//     backups, errors, terms, sums, reduced system, vectors           scratch, never copied
//     LbaCtl | estimates | flags                                      read back (LbaCtl once per trial)
// and every stage one launch on the context stream.  The pinned mirror holds the uploaded span and, right behind it,
// the read-back span; the scratch has no host copy.
struct LbaDeviceBackend {
    rsc_context* C;
    const LbaProblem& P;
    const std::vector<LbaEdge>& E;
    Arena A;
    LbaDev D{};
    char* h = nullptr;
    // the mirror of a read-back piece at arena offset o (>= A.back)
    char* HT(size_t o) const { return h + (o - A.back + A.up); }
    char* d = nullptr;
    size_t o_edge, o_cam, o_bad, o_plan, o_ctl, o_est_kf, o_est_pt, o_flags;
    // plan pieces, sized for the first phase (the second has no more of anything)
    size_t p_ae, p_rob, p_hidx, p_lidx, p_hk, p_lp, p_peb, p_pee, p_keb, p_kel, p_kll, p_pfb, p_pfl, p_slot;
    // with timing on: an event pair around every stage launch, harvested after the trial's synchronise
    std::vector<hipEvent_t> ev;
    std::vector<int> ev_stage;
    size_t ev_used = 0;
    ~LbaDeviceBackend() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    template <class Launch>
    int stage(int which, const char* what, Launch&& launch) {
        if (!C->timing) return hip(launch(), what);
        if (ev_used + 2 > ev.size()) {
            hipEvent_t a, b;
            if (int e = hip(hipEventCreate(&a), "hipEventCreate")) return e;
            ev.push_back(a);
            if (int e = hip(hipEventCreate(&b), "hipEventCreate")) return e;
            ev.push_back(b);
        }
        (void)hipEventRecord(ev[ev_used], C->stream);
        const int r = hip(launch(), what);
        (void)hipEventRecord(ev[ev_used + 1], C->stream);
        ev_stage.push_back(which);
        ev_used += 2;
        return r;
    }
    void harvest() {  // after a synchronise
        for (size_t i = 0; i < ev_used; i += 2) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) C->lba_stage_ms[ev_stage[i / 2]] += ms;
        }
        ev_used = 0;
        ev_stage.clear();
    }
    int hip(hipError_t e, const char* what) {
        if (e == hipSuccess) return 0;
        g_last_error = std::string(what) + ": " + hipGetErrorString(e);
        return RSC_ERR_HIP;
    }
    LbaDeviceBackend(rsc_context* c, const LbaProblem& p, const std::vector<LbaEdge>& e) : C(c), P(p), E(e) {}

    int setup() {
        const size_t ne = std::max(E.size(), (size_t)1), nk = (size_t)std::max(P.n_kfs, 1), np = (size_t)std::max(P.n_points, 1);
        size_t nfree = 0;
        for (int k = 0; k < P.n_kfs; ++k) nfree += P.kf_fixed[k] ? 0 : 1;
        const size_t F = std::max(nfree, (size_t)1), n = 6 * F;
        o_edge = A.take(sizeof(LbaEdge) * ne);
        o_cam = A.take(sizeof(PoCam) * nk);
        o_bad = A.take(np);
        o_plan = A.off;
        p_ae = A.take(4 * ne); p_rob = A.take(ne); p_hidx = A.take(4 * nk); p_lidx = A.take(4 * np);
        p_hk = A.take(4 * F); p_lp = A.take(4 * np); p_peb = A.take(4 * np); p_pee = A.take(4 * np);
        p_keb = A.take(4 * (F + 1)); p_kel = A.take(4 * ne); p_kll = A.take(4 * ne); p_pfb = A.take(4 * (np + 1));
        p_pfl = A.take(4 * ne); p_slot = A.take(4 * F * np);
        A.end_upload();
        const size_t s_bak_kf = A.take(sizeof(PoSE3) * nk), s_bak_pt = A.take(24 * np), s_err = A.take(24 * ne);
        const size_t s_terms = A.take(8 * (size_t)kLbaTerms * ne), s_chi = A.take(8 * ne), s_Hll = A.take(72 * np);
        const size_t s_bl = A.take(24 * np), s_Hpp = A.take(288 * F), s_bp = A.take(48 * F), s_Dinv = A.take(72 * np);
        const size_t s_db = A.take(24 * np), s_S = A.take(8 * n * n), s_bs = A.take(8 * n), s_x = A.take(8 * (n + 3 * np));
        const size_t s_sc = A.take(8 * (n + 3 * np));
        A.end_scratch();
        o_ctl = A.take(sizeof(LbaCtl));
        o_est_kf = A.take(sizeof(PoSE3) * nk);
        o_est_pt = A.take(24 * np);
        o_flags = A.take(ne);
        A.finish();
        if (int e = hip(hipSetDevice(C->device), "hipSetDevice")) return e;
        if (int e = C->d_lba.ensure(A.bytes)) return e;
        if (int e = C->h_lba.ensure(A.up + (A.bytes - A.back))) return e;
        if (int e = hip(hipStreamSynchronize(C->stream), "hipStreamSynchronize")) return e;
        h = C->h_lba.p;
        d = C->d_lba.p;
        if (!E.empty()) std::memcpy(h + o_edge, E.data(), sizeof(LbaEdge) * E.size());
        std::vector<PoSE3> kf;
        std::vector<PoCam> cam;
        std::vector<double> pt;
        lba_initial(P, kf, cam, pt);
        if (P.n_kfs) std::memcpy(h + o_cam, cam.data(), sizeof(PoCam) * cam.size());
        if (P.n_points) std::memcpy(h + o_bad, P.bad, (size_t)P.n_points);
        if (P.n_kfs) std::memcpy(HT(o_est_kf), kf.data(), sizeof(PoSE3) * kf.size());
        if (P.n_points) std::memcpy(HT(o_est_pt), pt.data(), 8 * pt.size());
        std::memset(HT(o_flags), 0, ne);
        std::memset(HT(o_ctl), 0, sizeof(LbaCtl));
        auto dp = [&](size_t o) { return d + o; };
        D.edge = reinterpret_cast<const LbaEdge*>(dp(o_edge));
        D.cam = reinterpret_cast<const PoCam*>(dp(o_cam));
        D.pt_bad = reinterpret_cast<const uint8_t*>(dp(o_bad));
        D.est_kf = reinterpret_cast<PoSE3*>(dp(o_est_kf));
        D.est_pt = reinterpret_cast<double*>(dp(o_est_pt));
        D.bak_kf = reinterpret_cast<PoSE3*>(dp(s_bak_kf));
        D.bak_pt = reinterpret_cast<double*>(dp(s_bak_pt));
        D.err = reinterpret_cast<double*>(dp(s_err));
        D.flags = reinterpret_cast<uint8_t*>(dp(o_flags));
        auto i32 = [&](size_t o) { return reinterpret_cast<const int32_t*>(dp(o)); };
        D.ae = i32(p_ae); D.robust = reinterpret_cast<const uint8_t*>(dp(p_rob)); D.kf_hidx = i32(p_hidx);
        D.pt_lidx = i32(p_lidx); D.hk = i32(p_hk); D.lp = i32(p_lp); D.pe_begin = i32(p_peb); D.pe_end = i32(p_pee);
        D.ke_begin = i32(p_keb); D.ke_list = i32(p_kel); D.kl_list = i32(p_kll); D.pf_begin = i32(p_pfb);
        D.pf_list = i32(p_pfl); D.slot = i32(p_slot);
        auto f64 = [&](size_t o) { return reinterpret_cast<double*>(dp(o)); };
        D.terms = f64(s_terms); D.chi = f64(s_chi); D.Hll = f64(s_Hll); D.bl = f64(s_bl); D.Hpp = f64(s_Hpp);
        D.bp = f64(s_bp); D.Dinv = f64(s_Dinv); D.db = f64(s_db); D.S = f64(s_S); D.bs = f64(s_bs); D.x = f64(s_x);
        D.sc = f64(s_sc);
        D.ctl = reinterpret_cast<LbaCtl*>(dp(o_ctl));
        D.n_kfs = P.n_kfs; D.n_points = P.n_points; D.n_edges = (int)E.size();
        D.na = D.F = D.L = D.n = 0;
        // the problem, and the estimates / flags / LbaCtl at the tail
        if (int e = hip(hipMemcpyAsync(d, h, o_plan, hipMemcpyHostToDevice, C->stream), "hipMemcpyAsync")) return e;
        if (int e = hip(hipMemcpyAsync(d + A.back, HT(A.back), A.bytes - A.back, hipMemcpyHostToDevice, C->stream),
                        "hipMemcpyAsync"))
            return e;
        // errors of edges that are never evaluated are read by nothing; x starts at zero in begin_phase
        return 0;
    }
    template <class T>
    void put(size_t o, const std::vector<T>& v) {
        if (!v.empty()) std::memcpy(h + o, v.data(), sizeof(T) * v.size());
    }
    int begin_phase(const LbaPlan& Q, int) {
        // the pinned plan is rewritten: the first phase's upload is long complete (its trials were read back)
        put(p_ae, Q.ae); put(p_rob, Q.robust); put(p_hidx, Q.kf_hidx); put(p_lidx, Q.pt_lidx); put(p_hk, Q.hk);
        put(p_lp, Q.lp); put(p_peb, Q.pe_begin); put(p_pee, Q.pe_end); put(p_keb, Q.ke_begin); put(p_kel, Q.ke_list);
        put(p_kll, Q.kl_list); put(p_pfb, Q.pf_begin); put(p_pfl, Q.pf_list); put(p_slot, Q.slot);
        D.na = (int)Q.ae.size(); D.F = Q.F; D.L = Q.L; D.n = 6 * Q.F;
        // everything before the slot table in one copy, the table at the size this phase uses
        if (int e = hip(hipMemcpyAsync(d + o_plan, h + o_plan, p_slot - o_plan, hipMemcpyHostToDevice, C->stream), "hipMemcpyAsync"))
            return e;
        if (!Q.slot.empty())
            if (int e = hip(hipMemcpyAsync(d + p_slot, h + p_slot, 4 * Q.slot.size(), hipMemcpyHostToDevice, C->stream),
                            "hipMemcpyAsync"))
                return e;
        if (int e = hip(hipMemsetAsync(D.ctl, 0, sizeof(LbaCtl), C->stream), "hipMemsetAsync")) return e;
        const size_t xb = 8 * ((size_t)D.n + 3 * (size_t)D.L);  // > 0: a phase with an edge has a point
        return hip(hipMemsetAsync(D.x, 0, xb, C->stream), "hipMemsetAsync");
    }
    int edges(bool build) { return stage(build ? 0 : 6, "launch_lba_edges", [&] { return launch_lba_edges(D, build, C->stream); }); }
    int fold() { return stage(1, "launch_lba_fold", [&] { return launch_lba_fold(D, C->stream); }); }
    int ctl_begin(int it) { return stage(2, "launch_lba_ctl_begin", [&] { return launch_lba_ctl_begin(D, it, C->stream); }); }
    int point_prep() { return stage(3, "launch_lba_point_prep", [&] { return launch_lba_point_prep(D, C->stream); }); }
    int schur() { return stage(4, "launch_lba_schur", [&] { return launch_lba_schur(D, C->stream); }); }
    int solve() { return stage(5, "launch_lba_solve", [&] { return launch_lba_solve(D, C->stream); }); }
    int update() { return stage(7, "launch_lba_update", [&] { return launch_lba_update(D, C->stream); }); }
    int ctl_trial() { return stage(8, "launch_lba_ctl_trial", [&] { return launch_lba_ctl_trial(D, C->stream); }); }
    int restore() { return stage(9, "launch_lba_restore", [&] { return launch_lba_restore(D, C->stream); }); }
    int classify(int phase) { return stage(10, "launch_lba_classify", [&] { return launch_lba_classify(D, phase, C->stream); }); }
    int read_ctl() {
        if (int e = hip(hipMemcpyAsync(HT(o_ctl), d + o_ctl, sizeof(LbaCtl), hipMemcpyDeviceToHost, C->stream), "hipMemcpyAsync"))
            return e;
        if (int e = hip(hipStreamSynchronize(C->stream), "hipStreamSynchronize")) return e;
        harvest();
        return 0;
    }
    int read_flags(int32_t* f) {  // the one record read of a trial
        if (int e = read_ctl()) return e;
        const LbaCtl* c = reinterpret_cast<const LbaCtl*>(HT(o_ctl));
        f[0] = c->accepted; f[1] = c->again; f[2] = c->stop;
        return 0;
    }
    int end_phase(LbaCtl& c) {
        if (int e = read_ctl()) return e;
        std::memcpy(&c, HT(o_ctl), sizeof(c));
        return 0;
    }
    int get_edge_flags(uint8_t* f) {
        if (E.empty()) return 0;
        if (int e = hip(hipMemcpyAsync(HT(o_flags), d + o_flags, E.size(), hipMemcpyDeviceToHost, C->stream), "hipMemcpyAsync"))
            return e;
        if (int e = hip(hipStreamSynchronize(C->stream), "hipStreamSynchronize")) return e;
        std::memcpy(f, HT(o_flags), E.size());
        return 0;
    }
    int get_state(PoSE3* kf, double* pt, uint8_t* f) {
        timing_begin(C, 4);
        if (int e = hip(hipMemcpyAsync(HT(A.back), d + A.back, A.bytes - A.back, hipMemcpyDeviceToHost, C->stream), "hipMemcpyAsync"))
            return e;
        if (int e = hip(hipStreamSynchronize(C->stream), "hipStreamSynchronize")) return e;
        harvest();
        if (P.n_kfs) std::memcpy(kf, HT(o_est_kf), sizeof(PoSE3) * (size_t)P.n_kfs);
        if (P.n_points) std::memcpy(pt, HT(o_est_pt), 24 * (size_t)P.n_points);
        if (!E.empty()) std::memcpy(f, HT(o_flags), E.size());
        return 0;
    }
};

}  // namespace

extern "C" {

// ---- Optimizer::LocalBundleAdjustment (src/Optimizer.cpp:426-787) ----
int rsc_local_bundle_adjustment_many(rsc_context* C, const rsc_localba_problem* problems, int count,
                                     const rsc_localba_out* out, rsc_localba_result* result) {
    if (!C || count < 0 || (count && !problems)) return RSC_ERR_ARG;
    if (count == 0) return RSC_OK;
    // every problem is checked before anything runs
    for (int c = 0; c < count; ++c) {
        int status = 0;
        if (const char* why = lba_check(lba_problem(problems[c]), status)) {
            g_last_error = why;
            return status;
        }
    }
    double total_ms = 0.0;
    for (double& v : C->lba_stage_ms) v = 0.0;
    for (int c = 0; c < count; ++c) {
        const LbaProblem P = lba_problem(problems[c]);
        const std::vector<LbaEdge> E = lba_edges(P);
        LbaDeviceBackend be(C, P, E);
        if (int e = be.setup()) return e;
        timing_begin(C, 3);
        if (int e = lba_run(be, P, E, out ? out + c : nullptr, result ? result + c : nullptr)) return e;
        timing_read(C);
        total_ms += C->last_ms[2];
    }
    if (C->timing) C->last_ms[2] = total_ms;
    return RSC_OK;
}

int rsc_diag_localba_stages(rsc_context* C, double* out, int cap) {
    if (!C || !out || cap < 11) return RSC_ERR_ARG;
    for (int i = 0; i < 11; ++i) out[i] = C->lba_stage_ms[i];
    return RSC_OK;
}

// ---- Optimizer::PoseOptimization (src/Optimizer.cpp:205-424) ----
int rsc_pose_optimization_many(rsc_context* C, const rsc_poseopt_problem* P, int count, rsc_poseopt_result* out,
                               uint8_t* const* outlier) {
    if (!C || count < 0 || (count && (!P || !out))) return RSC_ERR_ARG;
    if (count == 0) return RSC_OK;
    // compaction of the slots with a map point (the edges, Optimizer.cpp:247-325), in slot order
    std::vector<int> run;             // problems with >= 3 edges (the others return 0, :329-330)
    std::vector<size_t> eoff(1, 0);   // edge offsets of the run problems
    for (int c = 0; c < count; ++c) {
        const rsc_poseopt_problem& q = P[c];
        if (q.n < 0 || (q.n > 0 && (!q.uv || !q.Xw || !q.inv_sigma2))) return RSC_ERR_ARG;
        int ne = 0;
        for (int i = 0; i < q.n; ++i) {
            if (q.has_mp && !q.has_mp[i]) continue;
            ++ne;
        }
        if (ne > kPoseMaxEdges) {
            g_last_error = "more than 8192 map-point matches in one Frame";
            return RSC_ERR_UNSUPPORTED;
        }
        rsc_poseopt_result& r = out[c];
        std::memset(&r, 0, sizeof(r));
        r.n_initial = ne;
        std::memcpy(r.Tcw, q.Tcw, sizeof(r.Tcw));
        if (outlier && outlier[c])
            for (int i = 0; i < q.n; ++i)
                if (!q.has_mp || q.has_mp[i]) outlier[c][i] = 0;
        if (ne >= 3) {
            run.push_back(c);
            eoff.push_back(eoff.back() + (size_t)ne);
        }
    }
    const int R = (int)run.size();
    if (R == 0) return RSC_OK;
    const size_t E = eoff.back();
    RSC_HIP(hipSetDevice(C->device));
    const size_t o_probs = 0, o_xw = al256(sizeof(DevPoseProb) * R), o_uv = o_xw + al256(sizeof(float4) * E);
    const size_t o_ur = o_uv + al256(sizeof(float2) * E);  // mvuRight of the edges (stereo: >= 0)
    const size_t in_bytes = o_ur + al256(sizeof(float) * E);
    const size_t r_out = 0, r_flags = al256(sizeof(float) * 16 * R);
    const size_t res_bytes = r_flags + al256(E);
    if (int e = C->h_po_in.ensure(in_bytes)) return e;
    if (int e = C->d_po_in.ensure(in_bytes)) return e;
    if (int e = C->h_po_res.ensure(res_bytes)) return e;
    if (int e = C->d_po_res.ensure(res_bytes)) return e;
    // the previous call's copies out of the pinned staging must be complete
    RSC_HIP(hipStreamSynchronize(C->stream));
    char* h = C->h_po_in.p;
    char* d = C->d_po_in.p;
    DevPoseProb* hp = reinterpret_cast<DevPoseProb*>(h + o_probs);
    float4* hxw = reinterpret_cast<float4*>(h + o_xw);
    float2* huv = reinterpret_cast<float2*>(h + o_uv);
    float* hur = reinterpret_cast<float*>(h + o_ur);
    for (int k = 0; k < R; ++k) {
        const rsc_poseopt_problem& q = P[run[k]];
        size_t e = eoff[k];
        bool stereo = false;
        for (int i = 0; i < q.n; ++i) {
            if (q.has_mp && !q.has_mp[i]) continue;
            hxw[e] = make_float4(q.Xw[3 * i], q.Xw[3 * i + 1], q.Xw[3 * i + 2], q.inv_sigma2[i]);
            huv[e] = make_float2(q.uv[2 * i], q.uv[2 * i + 1]);
            hur[e] = q.u_right ? q.u_right[i] : -1.0f;
            stereo |= hur[e] >= 0.0f;
            ++e;
        }
        DevPoseProb& dp = hp[k];
        dp.xw = reinterpret_cast<const float4*>(d + o_xw) + eoff[k];
        dp.uv = reinterpret_cast<const float2*>(d + o_uv) + eoff[k];
        dp.ur = stereo ? reinterpret_cast<const float*>(d + o_ur) + eoff[k] : nullptr;
        dp.outlier = reinterpret_cast<uint8_t*>(C->d_po_res.p + r_flags) + eoff[k];
        dp.out = reinterpret_cast<float*>(C->d_po_res.p + r_out) + 16 * k;
        dp.n = (int)(eoff[k + 1] - eoff[k]);
        dp.fx = q.fx; dp.fy = q.fy; dp.cx = q.cx; dp.cy = q.cy; dp.bf = q.bf;
        for (int j = 0; j < 12; ++j) dp.T[j] = q.Tcw[j];
    }
    RSC_HIP(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, C->stream));
    RSC_HIP(timed_launch(C, [&] {
        return launch_poseopt(R, reinterpret_cast<const DevPoseProb*>(d + o_probs), C->h_flag + kFaultWord, C->stream);
    }));
    RSC_HIP(hipMemcpyAsync(C->h_po_res.p, C->d_po_res.p, res_bytes, hipMemcpyDeviceToHost, C->stream));
    RSC_HIP(hipStreamSynchronize(C->stream));
    if (int e = take_fault(C)) return e;
    timing_read(C);
    const float* ho = reinterpret_cast<const float*>(C->h_po_res.p + r_out);
    const uint8_t* hf = reinterpret_cast<const uint8_t*>(C->h_po_res.p + r_flags);
    for (int k = 0; k < R; ++k) {
        const int c = run[k];
        const rsc_poseopt_problem& q = P[c];
        rsc_poseopt_result& r = out[c];
        const float* o = ho + 16 * k;
        for (int j = 0; j < 12; ++j) r.Tcw[j] = o[j];
        r.Tcw[12] = r.Tcw[13] = r.Tcw[14] = 0.0f;
        r.Tcw[15] = 1.0f;
        std::memcpy(&r.n_good, o + 12, 4);
        std::memcpy(&r.rounds, o + 13, 4);
        std::memcpy(&r.lm_iterations, o + 14, 4);
        std::memcpy(&r.lm_trials, o + 15, 4);
        if (outlier && outlier[c]) {
            size_t e = eoff[k];
            for (int i = 0; i < q.n; ++i) {
                if (q.has_mp && !q.has_mp[i]) continue;
                outlier[c][i] = hf[e++];
            }
        }
    }
    return RSC_OK;
}

// ---- Optimizer::OptimizeSim3 (src/Optimizer.cpp:1054-1250) ----
int rsc_optimize_sim3_many(rsc_context* C, const rsc_sim3opt_problem* P, int count, rsc_sim3opt_result* out,
                           uint8_t* const* keep) {
    if (!C || count < 0 || (count && (!P || !out))) return RSC_ERR_ARG;
    if (count == 0) return RSC_OK;
    // compaction of the correspondences (Optimizer.cpp:1108-1171), in slot order
    std::vector<int> run;
    std::vector<size_t> moff(1, 0);
    for (int c = 0; c < count; ++c) {
        const rsc_sim3opt_problem& q = P[c];
        if (q.n < 0 || (q.n > 0 && (!q.valid || !q.X1w || !q.X2w || !q.uv1 || !q.uv2 || !q.inv1 || !q.inv2)))
            return RSC_ERR_ARG;
        int m = 0;
        for (int i = 0; i < q.n; ++i) m += q.valid[i] ? 1 : 0;
        if (m > kSim3OptMaxCorr) {
            g_last_error = "more than 8192 correspondences in one OptimizeSim3 problem";
            return RSC_ERR_UNSUPPORTED;
        }
        rsc_sim3opt_result& r = out[c];
        std::memset(&r, 0, sizeof(r));
        r.n_correspondences = m;
        std::memcpy(r.S, q.S, sizeof(r.S));
        if (keep && keep[c]) std::memset(keep[c], 1, (size_t)q.n);
        if (m > 0) {  // m == 0: optimize() has no vertex to optimise, nCorrespondences - nBad < 10 -> 0
            run.push_back(c);
            moff.push_back(moff.back() + (size_t)m);
        }
    }
    const int R = (int)run.size();
    if (R == 0) return RSC_OK;
    const size_t M = moff.back();
    RSC_HIP(hipSetDevice(C->device));
    const size_t o_e12 = al256(sizeof(DevSim3OptProb) * R), o_e21 = o_e12 + al256(sizeof(float4) * M);
    const size_t o_uv = o_e21 + al256(sizeof(float4) * M), in_bytes = o_uv + al256(sizeof(float4) * M);
    const size_t r_keep = al256(sizeof(double) * 16 * R), res_bytes = r_keep + al256(M);
    if (int e = C->h_so_in.ensure(in_bytes)) return e;
    if (int e = C->d_so_in.ensure(in_bytes)) return e;
    if (int e = C->h_so_res.ensure(res_bytes)) return e;
    if (int e = C->d_so_res.ensure(res_bytes)) return e;
    RSC_HIP(hipStreamSynchronize(C->stream));  // the previous call's copies out of the staging are done
    char* h = C->h_so_in.p;
    char* d = C->d_so_in.p;
    DevSim3OptProb* hp = reinterpret_cast<DevSim3OptProb*>(h);
    float4* h12 = reinterpret_cast<float4*>(h + o_e12);
    float4* h21 = reinterpret_cast<float4*>(h + o_e21);
    float4* huv = reinterpret_cast<float4*>(h + o_uv);
    for (int k = 0; k < R; ++k) {
        const rsc_sim3opt_problem& q = P[run[k]];
        size_t e = moff[k];
        for (int i = 0; i < q.n; ++i) {
            if (!q.valid[i]) continue;
            // P3D1c = R1w*P3D1w + t1w, P3D2c = R2w*P3D2w + t2w (float, Optimizer.cpp:1120-1136)
            const float* a = q.X1w + 3 * (size_t)i;
            const float* b = q.X2w + 3 * (size_t)i;
            float c1[3], c2[3];
            for (int r = 0; r < 3; ++r) {
                c1[r] = q.R1w[3 * r] * a[0] + q.R1w[3 * r + 1] * a[1] + q.R1w[3 * r + 2] * a[2] + q.t1w[r];
                c2[r] = q.R2w[3 * r] * b[0] + q.R2w[3 * r + 1] * b[1] + q.R2w[3 * r + 2] * b[2] + q.t2w[r];
            }
            h12[e] = make_float4(c2[0], c2[1], c2[2], q.inv1[i]);
            h21[e] = make_float4(c1[0], c1[1], c1[2], q.inv2[i]);
            huv[e] = make_float4(q.uv1[2 * i], q.uv1[2 * i + 1], q.uv2[2 * i], q.uv2[2 * i + 1]);
            ++e;
        }
        DevSim3OptProb& dp = hp[k];
        dp.e12 = reinterpret_cast<const float4*>(d + o_e12) + moff[k];
        dp.e21 = reinterpret_cast<const float4*>(d + o_e21) + moff[k];
        dp.uv = reinterpret_cast<const float4*>(d + o_uv) + moff[k];
        dp.keep = reinterpret_cast<uint8_t*>(C->d_so_res.p + r_keep) + moff[k];
        dp.out = reinterpret_cast<double*>(C->d_so_res.p) + 16 * k;
        dp.m = (int)(moff[k + 1] - moff[k]);
        dp.th2 = q.th2;
        const float deltaHuber = std::sqrt(q.th2);  // Optimizer.cpp:1104: float sqrt
        dp.delta = deltaHuber;
        std::memcpy(dp.K1, q.K1, sizeof(dp.K1));
        std::memcpy(dp.K2, q.K2, sizeof(dp.K2));
        std::memcpy(dp.S0, q.S, sizeof(dp.S0));
    }
    // the cooperative form: helper workgroups per pair, one workgroup per CU at most (its LDS)
    const int rpad = (R + 7) / 8 * 8;
    int helpers = C->so_helpers >= 0 ? C->so_helpers : std::min(7, kSoCoopCUs / rpad - 1);
    helpers = std::max(0, helpers);
    for (int k = 0; k < R; ++k) {
        hp[k].cf = nullptr;
        hp[k].cpub = hp[k].cstore = nullptr;
        hp[k].clist = nullptr;
    }
    if (helpers > 0) {
        const size_t o_pub = al256(sizeof(SoCoopFlags) * R), o_list = o_pub + al256(sizeof(double) * kSoCoopPub * R);
        size_t o_store = o_list + al256(sizeof(int) * M), store = 0;
        for (int k = 0; k < R; ++k) {
            const size_t nch = (2 * (moff[k + 1] - moff[k]) + kSoCoopChunk - 1) / kSoCoopChunk;
            store += nch * kSoCoopJd * kSoCoopChunk;
        }
        if (int e = C->d_so_coop.ensure(o_store + sizeof(double) * store)) return e;
        char* w = C->d_so_coop.p;
        size_t so = 0;
        for (int k = 0; k < R; ++k) {
            DevSim3OptProb& dp = hp[k];
            dp.cf = reinterpret_cast<SoCoopFlags*>(w) + k;
            dp.cpub = reinterpret_cast<double*>(w + o_pub) + (size_t)kSoCoopPub * k;
            dp.clist = reinterpret_cast<int*>(w + o_list) + moff[k];
            dp.cstore = reinterpret_cast<double*>(w + o_store) + so;
            so += (2 * (moff[k + 1] - moff[k]) + kSoCoopChunk - 1) / kSoCoopChunk * kSoCoopJd * kSoCoopChunk;
        }
    }
    RSC_HIP(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, C->stream));
    if (helpers > 0) RSC_HIP(hipMemsetAsync(C->d_so_coop.p, 0, sizeof(SoCoopFlags) * R, C->stream));
    RSC_HIP(timed_launch(C, [&] {
        return launch_sim3opt(R, reinterpret_cast<const DevSim3OptProb*>(d), helpers, C->h_flag + kFaultWord, C->stream);
    }));
    RSC_HIP(hipMemcpyAsync(C->h_so_res.p, C->d_so_res.p, res_bytes, hipMemcpyDeviceToHost, C->stream));
    RSC_HIP(hipStreamSynchronize(C->stream));
    if (int e = take_fault(C)) return e;
    timing_read(C);
    const double* ho = reinterpret_cast<const double*>(C->h_so_res.p);
    const uint8_t* hk = reinterpret_cast<const uint8_t*>(C->h_so_res.p + r_keep);
    for (int k = 0; k < R; ++k) {
        const int c = run[k];
        const rsc_sim3opt_problem& q = P[c];
        rsc_sim3opt_result& r = out[c];
        const double* o = ho + 16 * k;
        std::memcpy(r.S, o, 64);
        int32_t st[4];
        std::memcpy(st, o + 8, 16);
        r.n_inliers = st[0];
        r.n_bad = st[1];
        r.lm_iterations = st[2];
        r.lm_trials = st[3];
        if (keep && keep[c]) {
            size_t e = moff[k];
            for (int i = 0; i < q.n; ++i)
                if (q.valid[i]) keep[c][i] = hk[e++];
        }
    }
    return RSC_OK;
}

int rsc_diag_poseopt_phases(rsc_context* C, uint64_t* out, int cap) {
    if (!C || !out || cap < 64 * 8) return RSC_ERR_ARG;
    RSC_HIP(hipSetDevice(C->device));
    RSC_HIP(hipStreamSynchronize(C->stream));
    RSC_HIP(read_poseopt_phases(out, cap >= 64 * 24));
    return RSC_OK;
}

int rsc_diag_sim3opt_phases(rsc_context* C, uint64_t* out, int cap) {
    if (!C || !out || cap < 64 * 8) return RSC_ERR_ARG;
    RSC_HIP(hipSetDevice(C->device));
    RSC_HIP(hipStreamSynchronize(C->stream));
    RSC_HIP(read_sim3opt_phases(out));
    return RSC_OK;
}

}  // extern "C"
