// TEST-ONLY host build of the LocalBundleAdjustment arithmetic (rsc_localba.h), in two forms:
//   mode 0  the sequential restatement: g2o's control flow followed literally (sparse_optimizer.cpp,
//           optimization_algorithm_levenberg.cpp, block_solver.hpp, base_binary_edge.hpp) — one loop over the active
//           edges that adds into the vertices, the Schur complement landmark by landmark, the up-looking LDL^T of
//           DESIGN.md §2.17 — with a branch record of counters only.  It shares the per-edge and 3 x 3 arithmetic
//           (lba_jacobians, lba_quad_terms, po_*, inverse3) with the header and nothing else; it is also the one-core
//           CPU baseline of tools/localba_probe.py.
//   mode 1  the kernels' decomposition: the header's items in the order and grouping of localba.hip, the lanes run
//           one after another (the reduced solve right-looking, its forward substitution by columns).
// The product library never contains this code.
#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../orb-slam2-optimized_amd/csrc/rsc_localba.h"

using namespace rsc;

namespace {

// lba_solve_kernel, step by step: A is overwritten with the factor, x written only on success
bool solve_decomposed(int n, double* A, const double* bs, double* x) {
    for (int i = 0; i < n; ++i) {
        const double d = A[(size_t)i * n + i];
        if (d == 0.0) return false;
        for (int j = i + 1; j < n; ++j) lba_ldlt_scale_item(A, n, i, j, d);
        for (int j = i + 1; j < n; ++j)
            for (int k = j; k < n; ++k) lba_ldlt_update_item(A, n, i, j, k);
    }
    std::vector<double> z(bs, bs + n), pr((size_t)n);
    for (int i = 0; i < n; ++i) {
        const double zi = z[i];
        for (int j = i + 1; j < n; ++j) z[j] = z[j] - A[(size_t)j * n + i] * zi;
    }
    for (int j = 0; j < n; ++j) z[j] = (1.0 / A[(size_t)j * n + j]) * z[j];
    for (int j = n - 1; j >= 0; --j) {
        for (int i = j + 1; i < n; ++i) pr[i] = A[(size_t)i * n + j] * z[i];
        double acc = z[j];
        for (int i = j + 1; i < n; ++i) acc = acc - pr[i];
        z[j] = acc;
    }
    for (int j = 0; j < n; ++j) x[j] = z[j];
    return true;
}

// ---- mode 1: the device decomposition --------------------------------------------------------------
struct EmuBackend {
    const LbaProblem& P;
    const std::vector<LbaEdge>& E;
    std::vector<PoSE3> est_kf, bak_kf;
    std::vector<PoCam> cam;
    std::vector<double> est_pt, bak_pt, err, terms, chi, Hll, bl, Hpp, bp, Dinv, db, S, bs, x, sc;
    std::vector<uint8_t> flags;
    LbaPlan Q;
    LbaCtl ctl;
    LbaDev D;

    EmuBackend(const LbaProblem& p, const std::vector<LbaEdge>& e) : P(p), E(e) {
        lba_initial(P, est_kf, cam, est_pt);
        bak_kf = est_kf;
        bak_pt = est_pt;
        err.assign(3 * E.size(), 0.0);
        flags.assign(E.size(), 0);
        std::memset(&ctl, 0, sizeof(ctl));
        std::memset(&D, 0, sizeof(D));
    }
    int begin_phase(const LbaPlan& q, int) {
        Q = q;
        const size_t na = Q.ae.size(), F = (size_t)Q.F, L = (size_t)Q.L, n = 6 * F;
        terms.assign(kLbaTerms * na, 0.0);
        chi.assign(na, 0.0);
        Hll.assign(9 * L, 0.0); bl.assign(3 * L, 0.0); Hpp.assign(36 * F, 0.0); bp.assign(6 * F, 0.0);
        Dinv.assign(9 * L, 0.0); db.assign(3 * L, 0.0); S.assign(n * n, 0.0); bs.assign(n, 0.0);
        x.assign(n + 3 * L, 0.0); sc.assign(n + 3 * L, 0.0);
        std::memset(&ctl, 0, sizeof(ctl));
        D.edge = E.data(); D.cam = cam.data(); D.pt_bad = P.bad;
        D.est_kf = est_kf.data(); D.est_pt = est_pt.data(); D.bak_kf = bak_kf.data(); D.bak_pt = bak_pt.data();
        D.err = err.data(); D.flags = flags.data();
        D.ae = Q.ae.data(); D.robust = Q.robust.data(); D.kf_hidx = Q.kf_hidx.data(); D.pt_lidx = Q.pt_lidx.data();
        D.hk = Q.hk.data(); D.lp = Q.lp.data(); D.pe_begin = Q.pe_begin.data(); D.pe_end = Q.pe_end.data();
        D.ke_begin = Q.ke_begin.data(); D.ke_list = Q.ke_list.data(); D.kl_list = Q.kl_list.data();
        D.pf_begin = Q.pf_begin.data(); D.pf_list = Q.pf_list.data(); D.slot = Q.slot.data();
        D.terms = terms.data(); D.chi = chi.data(); D.Hll = Hll.data(); D.bl = bl.data(); D.Hpp = Hpp.data();
        D.bp = bp.data(); D.Dinv = Dinv.data(); D.db = db.data(); D.S = S.data(); D.bs = bs.data(); D.x = x.data();
        D.sc = sc.data(); D.ctl = &ctl;
        D.n_kfs = P.n_kfs; D.n_points = P.n_points; D.n_edges = (int)E.size();
        D.na = (int)na; D.F = Q.F; D.L = Q.L; D.n = 6 * Q.F;
        return 0;
    }
    int edges(bool build) {
        for (int a = 0; a < D.na; ++a) lba_edge_item(D, a, build);
        return 0;
    }
    int fold() {
        for (int i = 0; i < 12 * D.L; ++i) lba_fold_point_item(D, i / 12, i % 12);
        for (int i = 0; i < 42 * D.F; ++i) lba_fold_kf_item(D, i / 42, i % 42);
        return 0;
    }
    int ctl_begin(int it) { lba_ctl_begin(D, it); return 0; }
    int point_prep() {
        for (int l = 0; l < D.L; ++l) lba_point_prep_item(D, l);
        return 0;
    }
    int schur() {
        for (int b = 0; b < D.F * D.F; ++b) {
            const int i1 = b / D.F, i2 = b % D.F;
            if (i2 < i1) continue;
            for (int t = 0; t < 36; ++t) lba_schur_item(D, i1, i2, t / 6, t % 6);
            if (i1 == i2)
                for (int t = 0; t < 6; ++t) lba_bschur_item(D, i1, t);
        }
        return 0;
    }
    int solve() {
        ctl.ok2 = solve_decomposed(D.n, D.S, D.bs, D.x) ? 1 : 0;
        return 0;
    }
    int update() {
        for (int h = 0; h < D.F; ++h) lba_kf_update_item(D, h);
        for (int l = 0; l < D.L; ++l) lba_point_update_item(D, l);
        return 0;
    }
    int ctl_trial() { lba_ctl_trial(D); return 0; }
    int read_flags(int32_t* f) { f[0] = ctl.accepted; f[1] = ctl.again; f[2] = ctl.stop; return 0; }
    int restore() {
        for (int i = 0; i < D.F + D.L; ++i) lba_restore_item(D, i);
        return 0;
    }
    int end_phase(LbaCtl& c) { c = ctl; return 0; }
    int classify(int phase) {
        D.edge = E.data(); D.pt_bad = P.bad; D.est_kf = est_kf.data(); D.est_pt = est_pt.data();
        D.err = err.data(); D.flags = flags.data(); D.n_edges = (int)E.size();
        for (int e = 0; e < D.n_edges; ++e) lba_classify_item(D, e, phase);
        return 0;
    }
    int get_edge_flags(uint8_t* f) {
        std::copy(flags.begin(), flags.end(), f);
        return 0;
    }
    int get_state(PoSE3* kf, double* pt, uint8_t* f) {
        std::copy(est_kf.begin(), est_kf.end(), kf);
        std::copy(est_pt.begin(), est_pt.end(), pt);
        std::copy(flags.begin(), flags.end(), f);
        return 0;
    }
};

// ---- mode 0: g2o, line by line -------------------------------------------------------------------------
struct Seq {
    const LbaProblem& P;
    const std::vector<LbaEdge>& E;
    // the graph
    std::vector<PoSE3> kf;       // VertexSE3Expmap::_estimate
    std::vector<PoCam> cam;
    std::vector<double> pt;      // VertexSBAPointXYZ::_estimate
    std::vector<int> level, kernel;
    std::vector<double> err;     // the edges' _error
    // initializeOptimization
    std::vector<int> actE, ivPose, ivPoint, kfIndex, ptIndex;  // active edges; _ivMap (poses, then landmarks); hessianIndex
    int nActiveVertices = 0;
    // block solver
    std::vector<double> Hpp, Hll, Hpl, b, x;  // Hpl: one 6 x 3 block per active edge
    int sizePoses = 0;
    // Levenberg
    double lambda = 0, ni = 2;
    int nBad = 0;
    int32_t br[kLbaBranches];
    LbaPhaseStat stat[2];

    Seq(const LbaProblem& p, const std::vector<LbaEdge>& e) : P(p), E(e) {
        lba_initial(P, kf, cam, pt);
        level.assign(E.size(), 0);
        kernel.assign(E.size(), 1);
        err.assign(3 * E.size(), 0.0);
        for (int& v : br) v = 0;
    }

    bool initializeOptimization(int phase) {
        actE.clear();
        std::vector<int> kfLevelEdges((size_t)P.n_kfs, 0), ptLevelEdges((size_t)P.n_points, 0);
        std::vector<int> kfEdges((size_t)P.n_kfs, 0), ptEdges((size_t)P.n_points, 0);
        for (int e = 0; e < (int)E.size(); ++e) {
            ++kfEdges[E[e].kf];
            ++ptEdges[E[e].pt];
            if (level[e] != 0) continue;  // the point is never fixed: !allVerticesFixed()
            actE.push_back(e);
            ++kfLevelEdges[E[e].kf];
            ++ptLevelEdges[E[e].pt];
        }
        kfIndex.assign((size_t)P.n_kfs, -1);
        ptIndex.assign((size_t)P.n_points, -1);
        ivPose.clear();
        ivPoint.clear();
        nActiveVertices = 0;
        // sortVectorContainers + buildIndexMapping: by vertex id, non-marginalised first
        for (int k : lba_order_by_id(P.kf_id, P.n_kfs)) {
            if (!kfLevelEdges[k]) {
                if (kfEdges[k]) br[kLbBrVertexDropped]++;
                continue;
            }
            ++nActiveVertices;
            if (!P.kf_fixed[k]) {
                kfIndex[k] = (int)ivPose.size();
                ivPose.push_back(k);
            }
        }
        for (int p : lba_order_by_id(P.mp_id, P.n_points)) {
            if (!ptLevelEdges[p]) {
                if (ptEdges[p]) br[kLbBrVertexDropped]++;
                continue;
            }
            ++nActiveVertices;
            ptIndex[p] = (int)ivPoint.size();
            ivPoint.push_back(p);
        }
        LbaPhaseStat& st = stat[phase];
        st = LbaPhaseStat();
        st.n_vertices = nActiveVertices;
        st.n_points = (int)ivPoint.size();
        st.n_free = (int)ivPose.size();
        st.n_edges = (int)actE.size();
        return !actE.empty();
    }

    void computeActiveErrors() {
        for (int e : actE) {
            const LbaEdge& ed = E[e];
            const double Xw[3] = {pt[3 * ed.pt], pt[3 * ed.pt + 1], pt[3 * ed.pt + 2]};
            po_error(kf[ed.kf], cam[ed.kf], Xw, (double)ed.u, (double)ed.v, (double)ed.ur, lba_stereo(ed), err[3 * e],
                     err[3 * e + 1], err[3 * e + 2]);
        }
    }
    double activeRobustChi2() const {
        double chi = 0.0;
        for (int e : actE) {
            const bool st = lba_stereo(E[e]);
            const double d = lba_delta(st);
            chi += po_chi_term(kernel[e] != 0, st, (double)E[e].inv, err[3 * e], err[3 * e + 1], err[3 * e + 2], d, d * d);
        }
        return chi;
    }
    void buildSystem() {
        const size_t F = ivPose.size(), L = ivPoint.size();
        Hpp.assign(36 * F, 0.0);
        Hll.assign(9 * L, 0.0);
        Hpl.assign(18 * actE.size(), 0.0);
        b.assign(6 * F + 3 * L, 0.0);
        sizePoses = (int)(6 * F);
        for (size_t a = 0; a < actE.size(); ++a) {
            const int e = actE[a];
            const LbaEdge& ed = E[e];
            const bool st = lba_stereo(ed);
            const double Xw[3] = {pt[3 * ed.pt], pt[3 * ed.pt + 1], pt[3 * ed.pt + 2]};
            double A[3][3], B[3][6], t[kLbaTerms];
            lba_jacobians(kf[ed.kf], cam[ed.kf], Xw, st, A, B);
            const double er[3] = {err[3 * e], err[3 * e + 1], err[3 * e + 2]};
            const int h = kfIndex[ed.kf], l = ptIndex[ed.pt];
            if (st) lba_quad_terms<3>(A, B, er, (double)ed.inv, kernel[e] != 0, lba_delta(true), h >= 0, t);
            else lba_quad_terms<2>(A, B, er, (double)ed.inv, kernel[e] != 0, lba_delta(false), h >= 0, t);
            for (int k = 0; k < 3; ++k) b[sizePoses + 3 * l + k] += t[9 + k];
            for (int k = 0; k < 9; ++k) Hll[9 * l + k] += t[k];
            if (h >= 0) {
                for (int k = 0; k < 18; ++k) Hpl[18 * a + k] = t[54 + k];  // the cleared block += the product
                for (int k = 0; k < 6; ++k) b[6 * h + k] += t[48 + k];
                for (int k = 0; k < 36; ++k) Hpp[36 * h + k] += t[12 + k];
            }
        }
    }
    double computeLambdaInit() const {
        double maxDiagonal = 0.;
        for (size_t h = 0; h < ivPose.size(); ++h)
            for (int j = 0; j < 6; ++j) maxDiagonal = std::max(std::fabs(Hpp[36 * h + 7 * j]), maxDiagonal);
        for (size_t l = 0; l < ivPoint.size(); ++l)
            for (int j = 0; j < 3; ++j) maxDiagonal = std::max(std::fabs(Hll[9 * l + 4 * j]), maxDiagonal);
        return 1e-5 * maxDiagonal;
    }

    // LinearSolver::solve as DESIGN.md §2.17 states it: up-looking LDL^T without pivoting over the upper triangle
    static bool linearSolve(int n, const std::vector<double>& A, std::vector<double>& xs, const std::vector<double>& bb) {
        std::vector<double> Lm((size_t)n * n, 0.0), Dg((size_t)n, 0.0), y((size_t)n, 0.0);
        for (int k = 0; k < n; ++k) {
            for (int j = 0; j < k; ++j) {
                double v = A[(size_t)j * n + k];
                for (int i = 0; i < j; ++i) v -= Lm[(size_t)j * n + i] * y[i];
                y[j] = v;
            }
            double d = A[(size_t)k * n + k];
            for (int j = 0; j < k; ++j) {
                const double lkj = y[j] / Dg[j];
                Lm[(size_t)k * n + j] = lkj;
                d -= lkj * y[j];
            }
            Dg[k] = d;
            if (d == 0.0) return false;
        }
        std::vector<double> z(bb.begin(), bb.begin() + n);
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < j; ++i) z[j] -= Lm[(size_t)j * n + i] * z[i];
        for (int j = 0; j < n; ++j) z[j] = (1.0 / Dg[j]) * z[j];
        for (int j = n - 1; j >= 0; --j)
            for (int i = j + 1; i < n; ++i) z[j] -= Lm[(size_t)i * n + j] * z[i];
        for (int j = 0; j < n; ++j) xs[j] = z[j];
        return true;
    }

    bool solveSchur() {  // BlockSolver::solve with _doSchur
        const int F = (int)ivPose.size(), L = (int)ivPoint.size(), n = 6 * F;
        std::vector<double> Hs((size_t)n * n, 0.0), coef((size_t)n + 3 * (size_t)L, 0.0), DinvS(9 * (size_t)L, 0.0);
        for (int h = 0; h < F; ++h)  // _Hschur->clear(); _Hpp->add(_Hschur)
            for (int r = 0; r < 6; ++r)
                for (int c = 0; c < 6; ++c) Hs[(size_t)(6 * h + r) * n + 6 * h + c] += Hpp[36 * h + 6 * r + c];
        // the landmarks' columns of Hpl: (pose index, block), ascending pose index
        std::vector<std::vector<std::pair<int, int>>> col((size_t)L);
        for (size_t a = 0; a < actE.size(); ++a) {
            const int h = kfIndex[E[actE[a]].kf];
            if (h >= 0) col[ptIndex[E[actE[a]].pt]].push_back({h, (int)a});
        }
        for (auto& c : col) std::sort(c.begin(), c.end());
        for (int l = 0; l < L; ++l) {
            double Dm[3][3], Di[3][3];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) Dm[i][j] = Hll[9 * l + 3 * i + j];
            inverse3(Dm, Di);
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) DinvS[9 * l + 3 * i + j] = Di[i][j];
            const double* bl = &b[sizePoses + 3 * l];
            double dbv[3];
            for (int i = 0; i < 3; ++i) dbv[i] = emv3d_row(i, Di[i][0] * bl[0], Di[i][1] * bl[1], Di[i][2] * bl[2]);
            for (size_t o = 0; o < col[l].size(); ++o) {
                const int i1 = col[l][o].first;
                const double* Bi = &Hpl[18 * (size_t)col[l][o].second];
                double BDinv[6][3];
                for (int r = 0; r < 6; ++r)
                    for (int k = 0; k < 3; ++k)
                        BDinv[r][k] = (Bi[3 * r] * Di[0][k] + Bi[3 * r + 1] * Di[1][k]) + Bi[3 * r + 2] * Di[2][k];
                for (int r = 0; r < 6; ++r)
                    coef[6 * i1 + r] += (Bi[3 * r] * dbv[0] + Bi[3 * r + 1] * dbv[1]) + Bi[3 * r + 2] * dbv[2];
                for (size_t q = o; q < col[l].size(); ++q) {
                    const int i2 = col[l][q].first;
                    const double* Bj = &Hpl[18 * (size_t)col[l][q].second];
                    for (int r = 0; r < 6; ++r)
                        for (int c = 0; c < 6; ++c)
                            Hs[(size_t)(6 * i1 + r) * n + 6 * i2 + c] -=
                                (BDinv[r][0] * Bj[3 * c] + BDinv[r][1] * Bj[3 * c + 1]) + BDinv[r][2] * Bj[3 * c + 2];
                }
            }
        }
        std::vector<double> bschur(b.begin(), b.begin() + n);
        for (int i = 0; i < n; ++i) bschur[i] -= coef[i];
        if (!linearSolve(n, Hs, x, bschur)) return false;
        double* cp = coef.data();
        double* cl = coef.data() + n;
        for (int i = 0; i < n; ++i) cp[i] = -x[i];
        for (int i = 0; i < 3 * L; ++i) cl[i] = b[n + i];
        for (int l = 0; l < L; ++l)  // _HplCCS->rightMultiply(cl, cp)
            for (auto& rb : col[l]) {
                const double* Bi = &Hpl[18 * (size_t)rb.second];
                for (int j = 0; j < 3; ++j) {
                    double s = Bi[j] * cp[6 * rb.first];
                    for (int r = 1; r < 6; ++r) s += Bi[3 * r + j] * cp[6 * rb.first + r];
                    cl[3 * l + j] += s;
                }
            }
        for (int l = 0; l < L; ++l) {  // memset(xl, 0); _DInvSchur->multiply(xl, cl)
            const double* Di = &DinvS[9 * (size_t)l];
            for (int i = 0; i < 3; ++i)
                x[n + 3 * l + i] = 0.0 + emv3d_row(i, Di[3 * i] * cl[3 * l], Di[3 * i + 1] * cl[3 * l + 1], Di[3 * i + 2] * cl[3 * l + 2]);
        }
        return true;
    }

    // OptimizationAlgorithmLevenberg::solve; returns OK (true) or Terminate (false)
    bool solve(int iteration, LbaPhaseStat& st) {
        computeActiveErrors();
        double currentChi = activeRobustChi2();
        double tempChi = currentChi;
        const double iniChi = currentChi;
        buildSystem();
        st.its++;
        br[kLbBrIter]++;
        if (iteration == 0) {
            lambda = computeLambdaInit();
            ni = 2;
            nBad = 0;
            st.chi_first = currentChi;
        }
        st.chi_last = currentChi;
        double rho = 0;
        int qmax = 0;
        const int F = (int)ivPose.size(), L = (int)ivPoint.size();
        do {
            const std::vector<PoSE3> kfBackup = kf;  // push()
            const std::vector<double> ptBackup = pt;
            st.trials++;
            br[kLbBrTrial]++;
            // setLambda(_currentLambda, true)
            std::vector<double> backupPose((size_t)6 * F), backupLandmark((size_t)3 * L);
            for (int h = 0; h < F; ++h)
                for (int j = 0; j < 6; ++j) {
                    backupPose[6 * h + j] = Hpp[36 * h + 7 * j];
                    Hpp[36 * h + 7 * j] += lambda;
                }
            for (int l = 0; l < L; ++l)
                for (int j = 0; j < 3; ++j) {
                    backupLandmark[3 * l + j] = Hll[9 * l + 4 * j];
                    Hll[9 * l + 4 * j] += lambda;
                }
            const bool ok2 = solveSchur();
            // _optimizer->update(_solver->x())
            for (int h = 0; h < F; ++h) {
                const double u[6] = {x[6 * h], x[6 * h + 1], x[6 * h + 2], x[6 * h + 3], x[6 * h + 4], x[6 * h + 5]};
                kf[ivPose[h]] = po_mul(po_exp(u), kf[ivPose[h]]);
            }
            for (int l = 0; l < L; ++l)
                for (int j = 0; j < 3; ++j) pt[3 * ivPoint[l] + j] += x[6 * F + 3 * l + j];
            // restoreDiagonal
            for (int h = 0; h < F; ++h)
                for (int j = 0; j < 6; ++j) Hpp[36 * h + 7 * j] = backupPose[6 * h + j];
            for (int l = 0; l < L; ++l)
                for (int j = 0; j < 3; ++j) Hll[9 * l + 4 * j] = backupLandmark[3 * l + j];
            computeActiveErrors();
            tempChi = activeRobustChi2();
            if (!ok2) {
                tempChi = DBL_MAX;
                br[kLbBrNotOk2]++;
            }
            if (!std::isfinite(tempChi)) br[kLbBrChiNonFinite]++;
            rho = (currentChi - tempChi);
            double scale = 0.;  // computeScale
            for (size_t j = 0; j < x.size(); ++j) scale += x[j] * (lambda * x[j] + b[j]);
            scale += 1e-3;
            rho /= scale;
            if (rho != rho) br[kLbBrRhoNaN]++;
            if (rho > 0 && std::isfinite(tempChi)) {
                double alpha = 1. - po_cube(2 * rho - 1);
                alpha = (std::min)(alpha, 2. / 3.);
                const double scaleFactor = (std::max)(1. / 3., alpha);
                lambda *= scaleFactor;
                ni = 2;
                currentChi = tempChi;
            } else {
                lambda *= ni;
                ni *= 2;
                kf = kfBackup;  // pop()
                pt = ptBackup;
                br[kLbBrRejected]++;
            }
            qmax++;
            st.chi_last = currentChi;
        } while (rho < 0 && qmax < 10);
        if (qmax == 10 || rho == 0) {
            br[qmax == 10 ? kLbBrQmax : kLbBrRhoZero]++;
            return false;
        }
        if ((iniChi - currentChi) * 1e3 < iniChi) nBad++;
        else nBad = 0;
        if (nBad >= 3) {
            br[kLbBrNBad]++;
            return false;
        }
        return true;
    }

    void optimize(int iterations, int phase) {
        LbaPhaseStat& st = stat[phase];
        if (ivPose.empty() && ivPoint.empty()) return;  // _ivMap.size() == 0
        st.ran = 1;
        x.assign(6 * ivPose.size() + 3 * ivPoint.size(), 0.0);
        bool ok = true;
        for (int i = 0; i < iterations && ok; ++i) ok = solve(i, st);
    }

    void classify(int phase) {
        for (int pass = 0; pass < 2; ++pass)  // the mono loop, then the stereo loop
            for (int e = 0; e < (int)E.size(); ++e) {
                const LbaEdge& ed = E[e];
                const bool st = lba_stereo(ed);
                if ((int)st != pass) continue;
                if (P.bad[ed.pt]) continue;
                const double chi2 = po_chi2((double)ed.inv, st, err[3 * e], err[3 * e + 1], err[3 * e + 2]);
                const double Xw[3] = {pt[3 * ed.pt], pt[3 * ed.pt + 1], pt[3 * ed.pt + 2]};
                double pc[3];
                po_map(kf[ed.kf], Xw, pc);
                const bool isDepthPositive = pc[2] > 0.0;
                if (chi2 > (st ? 7.815 : 5.991) || !isDepthPositive) {
                    if (phase == 0) level[e] = 1;
                    else erase[e] = 1;
                }
                if (phase == 0) kernel[e] = 0;
            }
    }
    std::vector<uint8_t> erase;

    void run() {
        erase.assign(E.size(), 0);
        if (!initializeOptimization(0)) br[kLbBrNoActive]++;
        optimize(5, 0);
        classify(0);
        if (!initializeOptimization(1)) br[kLbBrNoActive]++;
        optimize(10, 1);
        classify(1);
    }
};

int run_sequential(const LbaProblem& P, const std::vector<LbaEdge>& E, const rsc_localba_out* out, rsc_localba_result* res) {
    Seq s(P, E);
    s.run();
    std::vector<uint8_t> flags(E.size());
    for (size_t e = 0; e < E.size(); ++e) flags[e] = (uint8_t)((s.level[e] ? 1 : 0) | (s.erase[e] ? 2 : 0));
    LbaOut o{nullptr, nullptr, nullptr, nullptr};
    if (out) o = LbaOut{out->Tcw, out->pos, out->edge_flags, out->erase};
    int32_t n_erase, n_level1, stale;
    lba_finish(P, E, s.kf.data(), s.pt.data(), flags.data(), o, n_erase, n_level1, stale);
    if (res) {
        std::memset(res, 0, sizeof(*res));
        res->n_erase = n_erase;
        res->n_level1 = n_level1;
        res->status = (s.stat[0].ran ? 0 : RSC_LOCALBA_NO_EDGE_1) | (s.stat[1].ran ? 0 : RSC_LOCALBA_NO_EDGE_2) |
                      (s.stat[0].ran && s.stat[0].n_free == 0 ? RSC_LOCALBA_NO_FREE_KF : 0);
        for (int p = 0; p < 2; ++p) {
            rsc_localba_phase& q = res->phase[p];
            q.n_vertices = s.stat[p].n_vertices; q.n_points = s.stat[p].n_points; q.n_edges = s.stat[p].n_edges;
            q.lm_iterations = s.stat[p].its; q.lm_trials = s.stat[p].trials;
            q.chi2_first = s.stat[p].chi_first; q.chi2_last = s.stat[p].chi_last;
        }
        s.br[kLbBrStaleKept] = stale;
        for (int k = 0; k < kLbaBranches; ++k) res->branches[k] = s.br[k];
    }
    return 0;
}

}  // namespace

extern "C" {

// mode 0 sequential, 1 decomposed; the status of rsc_local_bundle_adjustment_many's argument check
int lbae_run(const rsc_localba_problem* q, int mode, const rsc_localba_out* out, rsc_localba_result* res) {
    if (!q) return RSC_ERR_ARG;
    const LbaProblem P = lba_problem(*q);
    int status = 0;
    if (lba_check(P, status)) return status;
    const std::vector<LbaEdge> E = lba_edges(P);
    if (mode == 0) return run_sequential(P, E, out, res);
    EmuBackend be(P, E);
    return lba_run(be, P, E, out, res);
}

// The reduced solve alone on the upper triangle of the row-major n x n matrix A: 1 solved (x written), 0 a zero pivot
// (x untouched); mode as above
int lbae_solve(int n, const double* A, const double* b, int mode, double* x) {
    if (n < 0 || (n && (!A || !b || !x))) return RSC_ERR_ARG;
    std::vector<double> M(A, A + (size_t)n * n), bb(b, b + n), xs(x, x + n);
    const bool ok = mode == 0 ? Seq::linearSolve(n, M, xs, bb) : solve_decomposed(n, M.data(), bb.data(), xs.data());
    if (ok) std::memcpy(x, xs.data(), 8 * (size_t)n);
    return ok ? 1 : 0;
}

// One edge's arithmetic as the kernels and the sequential form run it: the pose (q x y z w, t) moved by exp(upd), the
// point by dX; e = computeError, A / B = linearizeOplus (row-major 3 x 3 and 3 x 6), t = the 72 terms of
// constructQuadraticForm (robust: with the edge's Huber kernel)
void lbae_edge(const double* pose, const double* cam, const double* X, const double* upd, const double* dX,
               const double* obs, double inv, int stereo, int robust, double* e, double* A, double* B, double* t) {
    PoSE3 T;
    T.r = PoQuat{pose[0], pose[1], pose[2], pose[3]};
    for (int i = 0; i < 3; ++i) T.t[i] = pose[4 + i];
    const double u[6] = {upd[0], upd[1], upd[2], upd[3], upd[4], upd[5]};
    T = po_mul(po_exp(u), T);
    const PoCam K{cam[0], cam[1], cam[2], cam[3], cam[4]};
    const double Xw[3] = {X[0] + dX[0], X[1] + dX[1], X[2] + dX[2]};
    double er[3], Am[3][3], Bm[3][6];
    po_error(T, K, Xw, obs[0], obs[1], obs[2], stereo != 0, er[0], er[1], er[2]);
    lba_jacobians(T, K, Xw, stereo != 0, Am, Bm);
    for (int i = 0; i < 3; ++i) {
        e[i] = er[i];
        for (int j = 0; j < 3; ++j) A[3 * i + j] = Am[i][j];
        for (int j = 0; j < 6; ++j) B[6 * i + j] = Bm[i][j];
    }
    if (stereo) lba_quad_terms<3>(Am, Bm, er, inv, robust != 0, lba_delta(true), true, t);
    else lba_quad_terms<2>(Am, Bm, er, inv, robust != 0, lba_delta(false), true, t);
}

}  // extern "C"
