// rsc_optim.cpp — the two LM optimisers of the C ABI: PoseOptimization and OptimizeSim3.
#include <cstring>
#include "rsc_host.h"
#include "rsc_poseopt.h"
#include "rsc_sim3opt.h"

constexpr int kSoCoopCUs = 256;  // OptimizeSim3's cooperative form: workgroups per launch at most (MI355X CUs)

extern "C" {

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
