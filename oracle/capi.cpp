// TEST INFRASTRUCTURE — parity oracle, never linked into the product library.
//
// Flat C entry points of the oracle for ctypes (tests/ and bench.py's cpu_baseline leg only).
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>
#include <atomic>
#include <memory>
#include "glibc_rand.h"
#include "pnp_oracle.h"
#include "sim3_oracle.h"
#include "mlpnp_oracle.h"
#include "poseopt_oracle.h"
#include "sim3opt_oracle.h"
#include "orbmatch_oracle.h"
#include "sim3match_oracle.h"
#include "kfdb_oracle.h"
#include "../include/rsc.h"
#include "../orb-slam2-optimized_amd/csrc/rsc_math.h"
#include "ora_linalg.h"

using namespace rsc_oracle;

template <int n>
static int sym_eig_n(const double* A, double* V, double* w) {
    double M[n][n];
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) M[i][j] = A[i * n + j];
    SymEig<double, n> e = sym_eig<double, n>(M);
    for (int i = 0; i < n; ++i) { w[i] = e.w[i]; for (int j = 0; j < n; ++j) V[i * n + j] = e.V[i][j]; }
    return e.ok ? 0 : 1;
}

template <int k>
static void svd_k(const double* A, const double* b, double* x) {
    double M[6][k];
    for (int r = 0; r < 6; ++r) for (int c = 0; c < k; ++c) M[r][c] = A[r * k + c];
    jacobi_svd_solve_6xk<k>(M, b, x);
}

extern "C" {

// ---- RNG ----
void ora_glibc_rand(uint32_t seed, int n, int32_t* out) {
    GlibcRand g(seed);
    for (int i = 0; i < n; ++i) out[i] = g.rand();
}

// Sample indices of `hyps` consecutive hypotheses of `min_set` swap-remove draws over N items
// (PnPsolver.cpp:125-138 / Sim3Solver.cpp:136-149).
void ora_sample_stream(uint32_t seed, int N, int min_set, int hyps, int32_t* out) {
    GlibcRand g(seed);
    std::vector<int32_t> all(N);
    for (int i = 0; i < N; ++i) all[i] = i;
    for (int h = 0; h < hyps; ++h) {
        std::vector<int32_t> av = all;
        for (int i = 0; i < min_set; ++i) {
            int randi = g.random_int(0, (int)av.size() - 1);
            out[h * min_set + i] = av[randi];
            av[randi] = av.back();
            av.pop_back();
        }
    }
}

// ---- linear-algebra restatements (numpy cross-checks) ----
int ora_sym_eig(int n, const double* A, double* V, double* w) {
    switch (n) {
        case 3: return sym_eig_n<3>(A, V, w);
        case 4: return sym_eig_n<4>(A, V, w);
        case 12: return sym_eig_n<12>(A, V, w);
    }
    return -1;
}
int ora_sym_eig4f(const float* A, float* V, float* w) {
    float M[4][4];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) M[i][j] = A[i * 4 + j];
    SymEig<float, 4> e = sym_eig<float, 4>(M);
    for (int i = 0; i < 4; ++i) { w[i] = e.w[i]; for (int j = 0; j < 4; ++j) V[i * 4 + j] = e.V[i][j]; }
    return e.ok ? 0 : 1;
}
int ora_svd_solve(int k, const double* A, const double* b, double* x) {
    switch (k) {
        case 3: svd_k<3>(A, b, x); return 0;
        case 4: svd_k<4>(A, b, x); return 0;
        case 5: svd_k<5>(A, b, x); return 0;
    }
    return -1;
}
int ora_random_int(uint32_t seed, int n_draws, const int32_t* maxes, int32_t* out) {
    GlibcRand g(seed);
    for (int i = 0; i < n_draws; ++i) out[i] = g.random_int(0, maxes[i]);
    return 0;
}

// ---- PnP ----
void* ora_pnp_create(int n, int n_points, const float* p2d, const float* p3dw, const float* sigma2,
                     const int32_t* kp_index, float fx, float fy, float cx, float cy, uint32_t seed) {
    return new PnPOracle(n, n_points, p2d, p3dw, sigma2, kp_index, fx, fy, cx, cy, seed);
}
void ora_pnp_destroy(void* h) { delete static_cast<PnPOracle*>(h); }
// Q3 event replays: the solver draws from the process-global libc rand(); ora_libc_srand seeds it.
void ora_pnp_use_libc_rand(void* h, int on) { static_cast<PnPOracle*>(h)->use_libc_rand(on != 0); }
void ora_sim3_use_libc_rand(void* h, int on) { static_cast<Sim3Oracle*>(h)->use_libc_rand(on != 0); }
void ora_mlpnp_use_libc_rand(void* h, int on) { static_cast<MLPnPOracle*>(h)->use_libc_rand(on != 0); }
void ora_libc_srand(uint32_t seed) { ::srand(seed); }
int ora_libc_rand(void) { return ::rand(); }
void ora_pnp_set_params(void* h, double prob, int min_inliers, int max_its, int min_set, float eps, float th2) {
    static_cast<PnPOracle*>(h)->SetRansacParameters(prob, min_inliers, max_its, min_set, eps, th2);
}
// Returns iterate()'s bool; *mask_len = vbInliers.size() (0 when the reference clears it).
int ora_pnp_iterate(void* h, int n_its, int* no_more, uint8_t* inliers, int* mask_len, int* n_inliers, float* T) {
    std::vector<uint8_t> v;
    bool nm = false;
    int ni = 0;
    bool ok = static_cast<PnPOracle*>(h)->iterate(n_its, nm, v, ni, T);
    *no_more = nm;
    *n_inliers = ni;
    *mask_len = (int)v.size();
    if (!v.empty()) std::memcpy(inliers, v.data(), v.size());
    return ok;
}
void ora_pnp_info(void* h, int* out) {
    auto* s = static_cast<PnPOracle*>(h);
    out[0] = s->iterations();
    out[1] = s->max_iterations();
    out[2] = s->min_inliers();
    out[3] = s->best_inliers();
    out[4] = s->max_rows();
}
void ora_pnp_max_error(void* h, float* out) {
    auto* s = static_cast<PnPOracle*>(h);
    std::memcpy(out, s->max_error().data(), s->max_error().size() * sizeof(float));
}
double ora_pnp_compute_pose(void* h, const int* idx, int n, float* R, float* t) {
    return static_cast<PnPOracle*>(h)->compute_pose_public(idx, n, R, t);
}
int ora_pnp_check_inliers(void* h, const float* R, const float* t, uint8_t* inl) {
    std::vector<uint8_t> v;
    int c = 0;
    static_cast<PnPOracle*>(h)->check_inliers_public(R, t, v, c);
    std::memcpy(inl, v.data(), v.size());
    return c;
}
// Trace: per hypothesis {sample[8], n_inliers, refine_called, refine_inliers, refine_ok} ints and
// {R[9], t[3]} floats.  Call with enable=1 before iterate; fetch with ora_pnp_trace_get.
void ora_pnp_trace_enable(void* h) {
    auto* s = static_cast<PnPOracle*>(h);
    if (!s->trace) s->trace = new std::vector<PnPTrace>();
}
int ora_pnp_trace_get(void* h, int cap, int32_t* ints, float* floats) {
    auto* s = static_cast<PnPOracle*>(h);
    if (!s->trace) return 0;
    int n = (int)s->trace->size();
    for (int i = 0; i < n && i < cap; ++i) {
        const PnPTrace& t = (*s->trace)[i];
        for (int k = 0; k < 8; ++k) ints[12 * i + k] = t.sample[k];
        ints[12 * i + 8] = t.n_inliers;
        ints[12 * i + 9] = t.refine_called;
        ints[12 * i + 10] = t.refine_inliers;
        ints[12 * i + 11] = t.refine_ok;
        for (int k = 0; k < 9; ++k) floats[12 * i + k] = t.R[k];
        for (int k = 0; k < 3; ++k) floats[12 * i + 9 + k] = t.t[k];
    }
    return n;
}

// CPU baseline / batch reference: C independent problems, problem c = rows [off[c], off[c]+n[c]) of
// the packed arrays; each builds a PnPsolver, SetRansacParameters(params), then iterate(n_its)
// once, on `nthreads` host threads (candidates are independent, Tracking.cpp:1239-1334 runs them
// sequentially on one thread).  Results per problem: ok, no_more, n_inliers, iterations, T[16].
void ora_pnp_run_batch(int C, const int32_t* n, const int64_t* off, const float* p2d, const float* p3dw,
                       const float* sigma2, float fx, float fy, float cx, float cy, const uint32_t* seeds,
                       double prob, int min_inliers, int max_its, int min_set, float eps, float th2, int n_its,
                       int nthreads, int32_t* out_i4, float* out_T, uint8_t* out_mask /* nullable, sum n */) {
    std::atomic<int> next(0);
    auto worker = [&]() {
        for (;;) {
            int c = next.fetch_add(1);
            if (c >= C) break;
            const int64_t o = off[c];
            std::vector<int32_t> kp(n[c]);
            for (int i = 0; i < n[c]; ++i) kp[i] = i;
            PnPOracle s(n[c], n[c], p2d + 2 * o, p3dw + 3 * o, sigma2 + o, kp.data(), fx, fy, cx, cy, seeds[c]);
            s.SetRansacParameters(prob, min_inliers, max_its, min_set, eps, th2);
            std::vector<uint8_t> v;
            bool nm = false;
            int ni = 0;
            float T[16];
            for (int k = 0; k < 16; ++k) T[k] = 0.f;
            bool ok = s.iterate(n_its, nm, v, ni, T);
            out_i4[4 * c + 0] = ok;
            out_i4[4 * c + 1] = nm;
            out_i4[4 * c + 2] = ni;
            out_i4[4 * c + 3] = s.iterations();
            std::memcpy(out_T + 16 * c, T, sizeof(T));
            if (out_mask) {
                if (v.empty()) std::memset(out_mask + o, 0, n[c]);
                else std::memcpy(out_mask + o, v.data(), n[c]);
            }
        }
    };
    if (nthreads <= 1) {
        worker();
    } else {
        std::vector<std::thread> th;
        for (int i = 0; i < nthreads; ++i) th.emplace_back(worker);
        for (auto& t : th) t.join();
    }
}

// ---- Sim3 ----
void* ora_sim3_create(int n1, const uint8_t* valid, const float* Xw1, const float* Xw2, const float* s1,
                      const float* s2, const float* R1, const float* t1, const float* R2, const float* t2,
                      const float* K1, const float* K2, uint32_t seed) {
    Sim3Input in;
    in.n1 = n1; in.valid = valid; in.Xw1 = Xw1; in.Xw2 = Xw2; in.sigma2_1 = s1; in.sigma2_2 = s2;
    std::memcpy(in.R1, R1, 9 * 4); std::memcpy(in.t1, t1, 12);
    std::memcpy(in.R2, R2, 9 * 4); std::memcpy(in.t2, t2, 12);
    std::memcpy(in.K1, K1, 16); std::memcpy(in.K2, K2, 16);
    return new Sim3Oracle(in, seed);
}
void ora_sim3_destroy(void* h) { delete static_cast<Sim3Oracle*>(h); }
void ora_sim3_set_params(void* h, double prob, int min_inliers, int max_its) {
    static_cast<Sim3Oracle*>(h)->SetRansacParameters(prob, min_inliers, max_its);
}
int ora_sim3_n(void* h) { return static_cast<Sim3Oracle*>(h)->N; }
// Prepared arrays: X1c[N][3], X2c[N][3], P1im1[N][2], P2im2[N][2], maxErr1/2 (as uint64), indices.
void ora_sim3_prepared(void* h, float* X1c, float* X2c, float* P1, float* P2, uint64_t* e1, uint64_t* e2,
                       int32_t* idx) {
    auto* s = static_cast<Sim3Oracle*>(h);
    const int N = s->N;
    std::memcpy(X1c, s->mvX3Dc1.data(), 12 * N);
    std::memcpy(X2c, s->mvX3Dc2.data(), 12 * N);
    std::memcpy(P1, s->mvP1im1.data(), 8 * N);
    std::memcpy(P2, s->mvP2im2.data(), 8 * N);
    std::memcpy(e1, s->mvnMaxError1.data(), 8 * N);
    std::memcpy(e2, s->mvnMaxError2.data(), 8 * N);
    std::memcpy(idx, s->mvnIndices1.data(), 4 * N);
}
int ora_sim3_iterate(void* h, int n_its, int* no_more, uint8_t* inliers, int* n_inliers) {
    std::vector<uint8_t> v;
    bool nm = false;
    int ni = 0;
    auto* s = static_cast<Sim3Oracle*>(h);
    bool ok = s->iterate(n_its, nm, v, ni);
    *no_more = nm;
    *n_inliers = ni;
    std::memcpy(inliers, v.data(), v.size());
    return ok;
}
void ora_sim3_estimate(void* h, float* R, float* t) {
    auto* s = static_cast<Sim3Oracle*>(h);
    s->GetEstimatedRotation(R);
    s->GetEstimatedTranslation(t);
}
void ora_sim3_info(void* h, int* out) {
    auto* s = static_cast<Sim3Oracle*>(h);
    out[0] = s->iterations();
    out[1] = s->max_iterations();
    out[2] = s->N;
}
void ora_sim3_compute(void* h, const int* idx, float* R, float* t) {
    static_cast<Sim3Oracle*>(h)->compute_sim3_public(idx, R, t);
}
int ora_sim3_check_inliers(void* h, const float* R, const float* t, uint8_t* inl) {
    std::vector<uint8_t> v;
    int c = static_cast<Sim3Oracle*>(h)->check_inliers_public(R, t, v);
    std::memcpy(inl, v.data(), v.size());
    return c;
}
void ora_sim3_trace_enable(void* h) {
    auto* s = static_cast<Sim3Oracle*>(h);
    if (!s->trace) s->trace = new std::vector<Sim3Trace>();
}
int ora_sim3_trace_get(void* h, int cap, int32_t* ints, float* floats) {
    auto* s = static_cast<Sim3Oracle*>(h);
    if (!s->trace) return 0;
    int n = (int)s->trace->size();
    for (int i = 0; i < n && i < cap; ++i) {
        const Sim3Trace& t = (*s->trace)[i];
        for (int k = 0; k < 3; ++k) ints[4 * i + k] = t.sample[k];
        ints[4 * i + 3] = t.n_inliers;
        for (int k = 0; k < 9; ++k) floats[12 * i + k] = t.R[k];
        for (int k = 0; k < 3; ++k) floats[12 * i + 9 + k] = t.t[k];
    }
    return n;
}

// CPU baseline for Sim3 on prepared arrays (the per-pair solver after construction):
// each problem runs SetRansacParameters(prob,minInl,maxIts) + iterate(n_its).
void ora_sim3_run_prepared_batch(int C, const int32_t* n, const int64_t* off, const float* X1c,
                                 const float* X2c, const float* P1, const float* P2, const uint64_t* e1,
                                 const uint64_t* e2, const float* K1, const float* K2, const uint32_t* seeds,
                                 double prob, int min_inliers, int max_its, int n_its, int nthreads,
                                 int32_t* out_i4, float* out_Rt) {
    std::atomic<int> next(0);
    auto worker = [&]() {
        for (;;) {
            int c = next.fetch_add(1);
            if (c >= C) break;
            const int64_t o = off[c];
            const int nc = n[c];
            // Rebuild a solver whose ctor output equals the prepared arrays: identity poses and
            // camera-frame points as "world" points reproduce X3Dc exactly (R*X + 0 with R = I is
            // exact in float), thresholds are fed back through sigma^2 such that size_t(9.210*s2)
            // would differ, so they are installed directly below.
            std::vector<uint8_t> valid(nc, 1);
            std::vector<float> s2(nc, 1.f);
            Sim3Input in;
            in.n1 = nc; in.valid = valid.data(); in.Xw1 = X1c + 3 * o; in.Xw2 = X2c + 3 * o;
            in.sigma2_1 = s2.data(); in.sigma2_2 = s2.data();
            const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z[3] = {0, 0, 0};
            std::memcpy(in.R1, I, 36); std::memcpy(in.R2, I, 36);
            std::memcpy(in.t1, z, 12); std::memcpy(in.t2, z, 12);
            std::memcpy(in.K1, K1, 16); std::memcpy(in.K2, K2, 16);
            Sim3Oracle s(in, seeds[c]);
            for (int i = 0; i < nc; ++i) { s.mvnMaxError1[i] = e1[o + i]; s.mvnMaxError2[i] = e2[o + i]; }
            std::memcpy(s.mvP1im1.data(), P1 + 2 * o, 8 * nc);
            std::memcpy(s.mvP2im2.data(), P2 + 2 * o, 8 * nc);
            s.SetRansacParameters(prob, min_inliers, max_its);
            std::vector<uint8_t> v;
            bool nm = false;
            int ni = 0;
            bool ok = s.iterate(n_its, nm, v, ni);
            out_i4[4 * c + 0] = ok;
            out_i4[4 * c + 1] = nm;
            out_i4[4 * c + 2] = ni;
            out_i4[4 * c + 3] = s.iterations();
            float R[9], t[3];
            s.GetEstimatedRotation(R);
            s.GetEstimatedTranslation(t);
            std::memcpy(out_Rt + 12 * c, R, 36);
            std::memcpy(out_Rt + 12 * c + 9, t, 12);
        }
    };
    if (nthreads <= 1) {
        worker();
    } else {
        std::vector<std::thread> th;
        for (int i = 0; i < nthreads; ++i) th.emplace_back(worker);
        for (auto& t : th) t.join();
    }
}


// ---- MLPnPsolver (mlpnp_oracle.h) ----------------------------------------------------------------
void ora_mlpnp_set_cov(void* h, const double* cov) { static_cast<MLPnPOracle*>(h)->set_covariances(cov); }
void* ora_mlpnp_create(int n, int n_points, const float* p2d, const float* p3dw, const float* sigma2,
                       const int32_t* kp_index, float fx, float fy, float cx, float cy, uint32_t seed) {
    return new MLPnPOracle(n, n_points, p2d, p3dw, sigma2, kp_index, fx, fy, cx, cy, seed);
}
void ora_mlpnp_destroy(void* h) { delete static_cast<MLPnPOracle*>(h); }
void ora_mlpnp_set_params(void* h, double prob, int min_inliers, int max_its, int min_set, float eps, float th2) {
    static_cast<MLPnPOracle*>(h)->SetRansacParameters(prob, min_inliers, max_its, min_set, eps, th2);
}
int ora_mlpnp_iterate(void* h, int n_its, int* no_more, uint8_t* inliers, int* mask_len, int* n_inliers, float* T) {
    std::vector<uint8_t> v;
    bool nm = false;
    int ni = 0;
    bool ok = static_cast<MLPnPOracle*>(h)->iterate(n_its, nm, v, ni, T);
    *no_more = nm;
    *n_inliers = ni;
    *mask_len = (int)v.size();
    if (!v.empty()) std::memcpy(inliers, v.data(), v.size());
    return ok;
}
void ora_mlpnp_info(void* h, int* out) {
    auto* s = static_cast<MLPnPOracle*>(h);
    out[0] = s->iterations();
    out[1] = s->max_iterations();
    out[2] = s->min_inliers();
    out[3] = s->best_inliers();
}
void ora_mlpnp_compute_pose(void* h, const int* idx, int n, double* R, double* t) {
    static_cast<MLPnPOracle*>(h)->compute_pose_public(idx, n, R, t);
}
// per-hypothesis trace: ints [8 sample + count], doubles [R 9 + t 3]
void ora_mlpnp_trace_enable(void* h) {
    auto* s = static_cast<MLPnPOracle*>(h);
    if (!s->trace) s->trace = new std::vector<MLPnPOracle::Trace>();
}
int ora_mlpnp_trace_get(void* h, int cap, int32_t* ints, double* dbls) {
    auto* s = static_cast<MLPnPOracle*>(h);
    if (!s->trace) return 0;
    const int n = std::min(cap, (int)s->trace->size());
    for (int i = 0; i < n; ++i) {
        const auto& t = (*s->trace)[i];
        for (int k = 0; k < 8; ++k) ints[9 * i + k] = t.sample[k];
        ints[9 * i + 8] = t.n_inliers;
        for (int k = 0; k < 9; ++k) dbls[12 * i + k] = t.R[k];
        for (int k = 0; k < 3; ++k) dbls[12 * i + 9 + k] = t.t[k];
    }
    return n;
}
// planar-branch flag of every traced hypothesis (MLPnPsolver.cpp:354-364)
int ora_mlpnp_trace_planar(void* h, int cap, int32_t* out) {
    auto* s = static_cast<MLPnPOracle*>(h);
    if (!s->trace) return 0;
    const int n = std::min(cap, (int)s->trace->size());
    for (int i = 0; i < n; ++i) out[i] = (*s->trace)[i].planar;
    return n;
}
void ora_mlpnp_run_batch(int C, const int32_t* n, const int64_t* off, const float* p2d, const float* p3dw,
                         const float* sigma2, float fx, float fy, float cx, float cy, const uint32_t* seeds,
                         double prob, int min_inliers, int max_its, int min_set, float eps, float th2, int n_its,
                         int nthreads, int32_t* out_i4, float* out_T) {
    std::atomic<int> next(0);
    auto worker = [&]() {
        for (;;) {
            int c = next.fetch_add(1);
            if (c >= C) break;
            const int64_t o = off[c];
            std::vector<int32_t> kp(n[c]);
            for (int i = 0; i < n[c]; ++i) kp[i] = i;
            MLPnPOracle s(n[c], n[c], p2d + 2 * o, p3dw + 3 * o, sigma2 + o, kp.data(), fx, fy, cx, cy, seeds[c]);
            s.SetRansacParameters(prob, min_inliers, max_its, min_set, eps, th2);
            std::vector<uint8_t> v;
            bool nm = false;
            int ni = 0;
            float T[16];
            bool ok = s.iterate(n_its, nm, v, ni, T);
            out_i4[4 * c + 0] = ok;
            out_i4[4 * c + 1] = nm;
            out_i4[4 * c + 2] = ni;
            out_i4[4 * c + 3] = s.iterations();
            std::memcpy(out_T + 16 * c, T, sizeof(T));
        }
    };
    if (nthreads <= 1) {
        worker();
    } else {
        std::vector<std::thread> th;
        for (int i = 0; i < nthreads; ++i) th.emplace_back(worker);
        for (auto& t : th) t.join();
    }
}

// ---- Config-5 event stream (CPU baseline and reference-order replay) -------------------------------
// Tracking::Relocalization (Tracking.cpp:1225-1262) / LoopClosing::ComputeSim3 (LoopClosing.cpp:258-286):
// every candidate of an event gets its solver (params set once), then rounds of iterate(5) over the
// candidates not yet discarded; a candidate whose call returns bNoMore is discarded; the event ends at the
// first candidate (in order) whose call returns a pose.  Event e = candidates [ev_begin[e], ev_begin[e+1]);
// candidate c = rows [off[c], off[c] + n[c]) of the packed arrays.  Per event: out_rec[4] = winner
// (index within the event, -1 if none), round, hypothesis (iterations - 1 of the winner), n_inliers;
// out_T[16] = the winner's Tcw (PnP) or [R12 | t12; 0 0 0 1] (Sim3).  Events run on `nthreads` threads.
}  // extern "C"

template <typename Solver, typename Make, typename Call>
static void run_events_generic(int n_events, const int32_t* ev_begin, int nthreads, int32_t* out_rec, float* out_T,
                               Make make, Call call) {
    std::atomic<int> next(0);
    auto worker = [&]() {
        for (;;) {
            const int e = next.fetch_add(1);
            if (e >= n_events) break;
            const int c0 = ev_begin[e], nc = ev_begin[e + 1] - ev_begin[e];
            std::vector<std::unique_ptr<Solver>> sv;
            for (int i = 0; i < nc; ++i) sv.emplace_back(make(c0 + i));
            std::vector<int> active(nc);
            for (int i = 0; i < nc; ++i) active[i] = i;
            int32_t* rec = out_rec + 4 * e;
            float* T = out_T + 16 * e;
            rec[0] = rec[1] = rec[2] = -1;
            rec[3] = 0;
            std::memset(T, 0, 64);
            bool done = false;
            for (int rnd = 0; !active.empty() && !done; ++rnd) {
                std::vector<int> keep;
                for (int i : active) {
                    bool nm = false;
                    int ni = 0;
                    if (call(*sv[i], nm, ni, T)) {
                        rec[0] = i; rec[1] = rnd; rec[2] = sv[i]->iterations() - 1; rec[3] = ni;
                        done = true;
                        break;
                    }
                    if (!nm) keep.push_back(i);
                }
                active.swap(keep);
            }
        }
    };
    if (nthreads <= 1) {
        worker();
    } else {
        std::vector<std::thread> th;
        for (int i = 0; i < nthreads; ++i) th.emplace_back(worker);
        for (auto& t : th) t.join();
    }
}

extern "C" {

void ora_reloc_events_batch(int n_events, const int32_t* ev_begin, const int32_t* n, const int64_t* off,
                            const float* p2d, const float* p3dw, const float* sigma2, float fx, float fy, float cx,
                            float cy, const uint32_t* seeds, double prob, int min_inliers, int max_its, int min_set,
                            float eps, float th2, int nthreads, int32_t* out_rec, float* out_T) {
    run_events_generic<PnPOracle>(
        n_events, ev_begin, nthreads, out_rec, out_T,
        [&](int c) {
            std::vector<int32_t> kp(n[c]);
            for (int i = 0; i < n[c]; ++i) kp[i] = i;
            const int64_t o = off[c];
            auto* s = new PnPOracle(n[c], n[c], p2d + 2 * o, p3dw + 3 * o, sigma2 + o, kp.data(), fx, fy, cx, cy,
                                    seeds[c]);
            s->SetRansacParameters(prob, min_inliers, max_its, min_set, eps, th2);
            return s;
        },
        [&](PnPOracle& s, bool& nm, int& ni, float* T) {
            std::vector<uint8_t> v;
            return s.iterate(5, nm, v, ni, T);
        });
}

// Loop events on the raw KeyFrame-pair inputs (Sim3Solver.cpp:6-85 constructor included, as the
// reference builds the solvers inside ComputeSim3).  Per candidate: poses[32] = R1 9, t1 3, R2 9, t2 3,
// K1 4, K2 4.
void ora_loop_events_batch(int n_events, const int32_t* ev_begin, const int32_t* n1, const int64_t* off,
                           const uint8_t* valid, const float* Xw1, const float* Xw2, const float* s1, const float* s2,
                           const float* poses, const uint32_t* seeds, double prob, int min_inliers, int max_its,
                           int nthreads, int32_t* out_rec, float* out_T) {
    run_events_generic<Sim3Oracle>(
        n_events, ev_begin, nthreads, out_rec, out_T,
        [&](int c) {
            const int64_t o = off[c];
            const float* P = poses + 32 * (size_t)c;
            Sim3Input in;
            in.n1 = n1[c]; in.valid = valid + o; in.Xw1 = Xw1 + 3 * o; in.Xw2 = Xw2 + 3 * o;
            in.sigma2_1 = s1 + o; in.sigma2_2 = s2 + o;
            std::memcpy(in.R1, P, 36); std::memcpy(in.t1, P + 9, 12);
            std::memcpy(in.R2, P + 12, 36); std::memcpy(in.t2, P + 21, 12);
            std::memcpy(in.K1, P + 24, 16); std::memcpy(in.K2, P + 28, 16);
            auto* s = new Sim3Oracle(in, seeds[c]);
            s->SetRansacParameters(prob, min_inliers, max_its);
            return s;
        },
        [&](Sim3Oracle& s, bool& nm, int& ni, float* T) {
            std::vector<uint8_t> v;
            if (!s.iterate(5, nm, v, ni)) return false;
            float R[9], t[3];
            s.GetEstimatedRotation(R);
            s.GetEstimatedTranslation(t);
            for (int r = 0; r < 3; ++r) {
                for (int k = 0; k < 3; ++k) T[4 * r + k] = R[3 * r + k];
                T[4 * r + 3] = t[r];
            }
            T[15] = 1.f;
            return true;
        });
}

// qr_solve (PnPsolver.cpp:693-796) on one 6x4 system: A row-major (modified in place as the
// reference does), b, X = the previous X (kept on the singular bail-out).  Returns 1 / 0 (singular).
int ora_qr_solve(double* A, double* b, double* X) {
    double Am[6][4];
    for (int i = 0; i < 6; ++i) for (int j = 0; j < 4; ++j) Am[i][j] = A[4 * i + j];
    const bool ok = rsc_oracle::PnPOracle::qr_solve(Am, b, X);
    for (int i = 0; i < 6; ++i) for (int j = 0; j < 4; ++j) A[4 * i + j] = Am[i][j];
    return ok ? 1 : 0;
}

// deterministic libm (csrc/rsc_math.h) for the accuracy tests
void ora_mlpnp_jac(const double* X, const double* nr, const double* ns, const double* x, double* J) {
    rsc_oracle::mlpnp_jacobian_public(X, nr, ns, x, J);
}
double ora_dm_sin(double x) { return rsc::dm::sin(x); }
double ora_dm_cos(double x) { return rsc::dm::cos(x); }
double ora_dm_acos(double x) { return rsc::dm::acos(x); }
double ora_dm_cbrt(double x) { return rsc::dm::cbrt(x); }
double ora_dm_pow13(double x) { return rsc::dm::pow_1_3(x); }
double ora_dm_pow32(double x) { return rsc::dm::pow_3_2(x); }

// ---- Optimizer::PoseOptimization (mono + stereo edges) ----
// stats[3] = rounds, LM iterations, LM trials.  Returns nGood.
int ora_pose_optimization(int n, const uint8_t* has_mp, const float* uv, const float* Xw, const float* inv_sigma2,
                          float fx, float fy, float cx, float cy, const float* Tcw_in, float* Tcw_out,
                          uint8_t* outlier, int32_t* stats, const float* u_right, float bf) {
    PoseOptInput in{n, has_mp, uv, Xw, inv_sigma2, fx, fy, cx, cy, {}, u_right, bf};
    std::memcpy(in.Tcw, Tcw_in, sizeof(in.Tcw));
    PoseOptStats st{};
    const int r = pose_optimization(in, Tcw_out, outlier, &st);
    if (stats) { stats[0] = st.rounds; stats[1] = st.lm_iterations; stats[2] = st.lm_trials; }
    return r;
}

// ora_pose_optimization plus the call's LM branch record (lm_branches.h): branches[11] = trials, !ok2,
// non-finite tempChi, NaN rho, rejected, ended by qmax == 10 / rho == 0 / nBadLM >= 3, optimize() calls
// without an active edge, iterations entered with a non-finite currentChi, accepted !ok2 trials.  Same
// arithmetic and results.
int ora_pose_optimization_branches(int n, const uint8_t* has_mp, const float* uv, const float* Xw,
                                   const float* inv_sigma2, float fx, float fy, float cx, float cy,
                                   const float* Tcw_in, float* Tcw_out, uint8_t* outlier, int32_t* stats,
                                   const float* u_right, float bf, int32_t* branches) {
    PoseOptInput in{n, has_mp, uv, Xw, inv_sigma2, fx, fy, cx, cy, {}, u_right, bf};
    std::memcpy(in.Tcw, Tcw_in, sizeof(in.Tcw));
    PoseOptStats st{};
    LmBranches br{};
    const int r = pose_optimization(in, Tcw_out, outlier, &st, &br);
    if (stats) { stats[0] = st.rounds; stats[1] = st.lm_iterations; stats[2] = st.lm_trials; }
    static_assert(kLmBranchFields == 11, "branches[11]");
    std::memcpy(branches, &br, sizeof(br));
    return r;
}

// Batch of problems (bench cpu_baseline): problem c has edges [off[c], off[c+1]) (all with map points).
void ora_pose_optimization_batch(int count, const int64_t* off, const float* uv, const float* Xw,
                                 const float* inv_sigma2, float fx, float fy, float cx, float cy,
                                 const float* Tcw_in, float* Tcw_out, uint8_t* outlier, int32_t* n_good,
                                 const float* u_right /* nullable */, float bf) {
    for (int c = 0; c < count; ++c) {
        const int64_t o = off[c];
        const int n = (int)(off[c + 1] - o);
        PoseOptInput in{n, nullptr, uv + 2 * o, Xw + 3 * o, inv_sigma2 + o, fx, fy, cx, cy, {},
                        u_right ? u_right + o : nullptr, bf};
        std::memcpy(in.Tcw, Tcw_in + 16 * c, sizeof(in.Tcw));
        n_good[c] = pose_optimization(in, Tcw_out + 16 * c, outlier + o, nullptr);
    }
}

// ---- Optimizer::OptimizeSim3 (Optimizer.cpp:1054-1250) ----
// poses[24] = R1w 9, t1w 3, R2w 9, t2w 3; K[8] = K1 (fx, fy, cx, cy), K2; S[8] = q (x, y, z, w), t, s
// in/out; stats[4] = nCorrespondences, nBad, LM iterations, LM trials.  Returns nIn.
static int optimize_sim3_c(int n, const uint8_t* valid, const float* X1w, const float* X2w, const float* uv1,
                           const float* uv2, const float* inv1, const float* inv2, const float* poses, const float* K,
                           float th2, double* S, uint8_t* keep, int32_t* stats, LmBranches* br) {
    Sim3OptInput in;
    in.n = n; in.valid = valid; in.X1w = X1w; in.X2w = X2w; in.uv1 = uv1; in.uv2 = uv2; in.inv1 = inv1;
    in.inv2 = inv2;
    std::memcpy(in.R1w, poses, 36); std::memcpy(in.t1w, poses + 9, 12);
    std::memcpy(in.R2w, poses + 12, 36); std::memcpy(in.t2w, poses + 21, 12);
    std::memcpy(in.K1, K, 16); std::memcpy(in.K2, K + 4, 16);
    in.th2 = th2;
    Sim3Est e;
    std::memcpy(e.q, S, 32); std::memcpy(e.t, S + 4, 24); e.s = S[7];
    Sim3OptStats st{};
    const int r = optimize_sim3(in, e, keep, &st, br);
    std::memcpy(S, e.q, 32); std::memcpy(S + 4, e.t, 24); S[7] = e.s;
    if (stats) { stats[0] = st.n_correspondences; stats[1] = st.n_bad; stats[2] = st.lm_iterations; stats[3] = st.lm_trials; }
    return r;
}

int ora_optimize_sim3(int n, const uint8_t* valid, const float* X1w, const float* X2w, const float* uv1,
                      const float* uv2, const float* inv1, const float* inv2, const float* poses, const float* K,
                      float th2, double* S, uint8_t* keep, int32_t* stats) {
    return optimize_sim3_c(n, valid, X1w, X2w, uv1, uv2, inv1, inv2, poses, K, th2, S, keep, stats, nullptr);
}

// ora_optimize_sim3 plus the call's LM branch record (branches[11], as ora_pose_optimization_branches).
int ora_optimize_sim3_branches(int n, const uint8_t* valid, const float* X1w, const float* X2w, const float* uv1,
                               const float* uv2, const float* inv1, const float* inv2, const float* poses,
                               const float* K, float th2, double* S, uint8_t* keep, int32_t* stats,
                               int32_t* branches) {
    LmBranches br{};
    const int r = optimize_sim3_c(n, valid, X1w, X2w, uv1, uv2, inv1, inv2, poses, K, th2, S, keep, stats, &br);
    std::memcpy(branches, &br, sizeof(br));
    return r;
}

// ---- ORBmatcher::SearchByBoW (ORBmatcher.cpp:110-240, :354-488) ----
// a BowView with its FeatureVector rebuilt from CSR (node ids ascending, node_begin[nn+1], feat);
// arrays are copied so the handle owns its data
struct OraBow {
    std::vector<uint8_t> desc, valid;
    std::vector<float> angle;
    BowView v;
};

void* ora_bow_create(int n, const uint8_t* desc, const float* angle, const uint8_t* valid, int n_nodes,
                     const uint32_t* node_id, const int32_t* node_begin, const uint32_t* feat) {
    OraBow* b = new OraBow;
    b->desc.assign(desc, desc + 32 * (size_t)n);
    b->angle.assign(angle, angle + n);
    if (valid) b->valid.assign(valid, valid + n);
    b->v.n = n;
    b->v.desc = b->desc.data();
    b->v.angle = b->angle.data();
    b->v.valid = valid ? b->valid.data() : nullptr;
    for (int k = 0; k < n_nodes; ++k)
        b->v.fv[node_id[k]].assign(feat + node_begin[k], feat + node_begin[k + 1]);
    return b;
}

void ora_bow_destroy(void* h) { delete static_cast<OraBow*>(h); }

// frame_variant = 1: SearchByBoW(pKF = a, F = b), out[b.n]; 0: SearchByBoW(pKF1 = a, pKF2 = b), out[a.n]
int ora_search_by_bow(int frame_variant, void* a, void* b, float nnratio, int check_ori, int32_t* out) {
    const BowView& A = static_cast<OraBow*>(a)->v;
    const BowView& B = static_cast<OraBow*>(b)->v;
    return frame_variant ? search_by_bow_frame(A, B, nnratio, check_ori != 0, out)
                         : search_by_bow_kf(A, B, nnratio, check_ori != 0, out);
}

// `count` searches of a[c] against the shared b (the relocalization / loop-closure candidate loops,
// Tracking.cpp:1207-1232, LoopClosing.cpp:238-265); out rows of out_stride; returns total matches
int64_t ora_search_by_bow_many(int frame_variant, int count, void* const* a, void* b, float nnratio,
                               int check_ori, int32_t* out, int64_t out_stride, int32_t* nmatches) {
    int64_t tot = 0;
    for (int c = 0; c < count; ++c) {
        nmatches[c] = ora_search_by_bow(frame_variant, a[c], b, nnratio, check_ori, out + out_stride * c);
        tot += nmatches[c];
    }
    return tot;
}

// ---- ORBmatcher::SearchBySim3 (ORBmatcher.cpp:948-1170) ----
static Sim3KF to_kf(const rsc_sim3_kf& k) {
    Sim3KF o;
    o.n = k.n; o.kp = k.kp; o.octave = k.octave; o.desc = k.desc; o.cell_begin = k.cell_begin;
    o.cell_feat = k.cell_feat; o.min_x = k.min_x; o.max_x = k.max_x; o.min_y = k.min_y; o.max_y = k.max_y;
    o.grid_w_inv = k.grid_w_inv; o.grid_h_inv = k.grid_h_inv; o.fx = k.fx; o.fy = k.fy; o.cx = k.cx;
    o.cy = k.cy; o.scale_factors = k.scale_factors; o.n_levels = k.n_levels;
    o.log_scale_factor = k.log_scale_factor;
    std::memcpy(o.Rcw, k.Rcw, sizeof(o.Rcw));
    std::memcpy(o.tcw, k.tcw, sizeof(o.tcw));
    o.mp_state = k.mp_state; o.mp_pos = k.mp_pos; o.mp_dmax = k.mp_dmax; o.mp_dmin = k.mp_dmin;
    o.mp_desc = k.mp_desc;
    return o;
}

int ora_search_by_sim3(const rsc_sim3_kf* k1, const rsc_sim3_kf* k2, const int32_t* matched12, const float* R12,
                       const float* t12, float th, int32_t* out12) {
    return search_by_sim3(to_kf(*k1), to_kf(*k2), matched12, R12, t12, th, out12);
}

int ora_search_by_sim3_trace(const rsc_sim3_kf* k1, const rsc_sim3_kf* k2, const int32_t* matched12, const float* R12,
                             const float* t12, float th, int32_t* out12, int32_t* m1, int32_t* m2, int32_t* reason1,
                             int32_t* reason2) {
    return search_by_sim3_trace(to_kf(*k1), to_kf(*k2), matched12, R12, t12, th, out12, m1, m2, reason1, reason2);
}

int ora_predict_scale(float dmax, float dist, float log_scale_factor, int n_levels) {
    return predict_scale(dmax, dist, log_scale_factor, n_levels);
}

double ora_dm_log(double x) { return rsc::dm::log(x); }

int ora_descriptor_distance(const uint8_t* a, const uint8_t* b) { return descriptor_distance(a, b); }

void ora_compute_three_maxima(const int32_t* sizes, int L, int32_t* ind) {
    int i1 = -1, i2 = -1, i3 = -1;
    compute_three_maxima(sizes, L, i1, i2, i3);
    ind[0] = i1; ind[1] = i2; ind[2] = i3;
}

// ---- KeyFrameDatabase (kfdb_oracle.h) ----
void* ora_kfdb_create(int capacity) { return new rsc_oracle::KFDatabase(capacity); }
void ora_kfdb_destroy(void* db) { delete static_cast<rsc_oracle::KFDatabase*>(db); }
void ora_kfdb_add(void* db, int kf, int n, const uint32_t* ids, const double* vals) {
    static_cast<rsc_oracle::KFDatabase*>(db)->add(kf, n, ids, vals);
}
void ora_kfdb_erase(void* db, int kf) { static_cast<rsc_oracle::KFDatabase*>(db)->erase(kf); }
void ora_kfdb_clear(void* db) { static_cast<rsc_oracle::KFDatabase*>(db)->clear(); }
void ora_kfdb_set_covisibility(void* db, int kf, int n, const int32_t* best) {
    static_cast<rsc_oracle::KFDatabase*>(db)->set_covisibility(kf, n, best);
}
int ora_kfdb_detect_relocalization(void* db, uint64_t frame_id, int n, const uint32_t* ids, const double* vals,
                                   int32_t* out) {
    const auto r = static_cast<rsc_oracle::KFDatabase*>(db)->detect_relocalization(frame_id, n, ids, vals);
    for (size_t i = 0; i < r.size(); ++i) out[i] = r[i];
    return (int)r.size();
}
int ora_kfdb_detect_loop(void* db, uint64_t kf_id, int n, const uint32_t* ids, const double* vals, int n_connected,
                         const int32_t* connected, float min_score, int32_t* out) {
    const auto r = static_cast<rsc_oracle::KFDatabase*>(db)->detect_loop(kf_id, n, ids, vals, n_connected, connected,
                                                                         min_score);
    for (size_t i = 0; i < r.size(); ++i) out[i] = r[i];
    return (int)r.size();
}
// state: [loop_query, reloc_query] u64, [loop_words, reloc_words] i32, [loop_score, reloc_score] f32
void ora_kfdb_state(void* db, int kf, uint64_t* q, int32_t* w, float* s) {
    const auto& st = static_cast<rsc_oracle::KFDatabase*>(db)->state(kf);
    q[0] = st.loop_query;
    q[1] = st.reloc_query;
    w[0] = st.loop_words;
    w[1] = st.reloc_words;
    s[0] = st.loop_score;
    s[1] = st.reloc_score;
}
double ora_l1_score(int n1, const uint32_t* id1, const double* v1, int n2, const uint32_t* id2, const double* v2) {
    return rsc_oracle::l1_score(n1, id1, v1, n2, id2, v2);
}

}  // extern "C"
