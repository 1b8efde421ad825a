// rsc_localba.h — Optimizer::LocalBundleAdjustment (src/Optimizer.cpp:426-787) on the GPU: the g2o
// Levenberg-Marquardt over many VertexSE3Expmap (KeyFrames) and marginalised VertexSBAPointXYZ (MapPoints)
// with EdgeSE3ProjectXYZ (mono) / EdgeStereoSE3ProjectXYZ (stereo) edges, BlockSolver_6_3's Schur complement
// and a dense LDL^T of the reduced pose system; optimize(5) with Huber kernels, classification,
// optimize(10) over the level-0 edges, final classification.
//
// This header holds (a) the per-item arithmetic of every stage as __host__ __device__ functions over an
// LbaDev (the kernels of localba.hip call one item per lane; tests/localba_emu runs the same items one after
// another), (b) the host-side plan of a phase (active sets, Hessian indices, the walk lists) and (c) the driver
// of the two phases over a backend that runs the stages (the device backend of rsc_optim.cpp enqueues kernels
// and reads the LbaCtl record once per LM trial; the emulation's backend loops).  tests/localba_emu also holds
// the sequential restatement that follows g2o's control flow literally; it shares only the per-edge and 3x3
// arithmetic with this file.
//
// g2o source followed (Thirdparty/g2o/g2o): core/sparse_optimizer.cpp:166-267,354-435,
// core/optimization_algorithm_levenberg.cpp:61-189, core/block_solver.hpp:354-604,
// core/base_binary_edge.hpp:55-115, core/sparse_block_matrix_ccs.h:103-128, core/robust_kernel_impl.cpp,
// types/types_six_dof_expmap.cpp:103-157,188-234, types/types_sba.h (VertexSBAPointXYZ::oplusImpl).
// Sums of fixed-size products run left to right (as rsc_poseopt.h); Matrix3d * Vector3d follows
// emv3d_row; Matrix3d::inverse is inverse3.  The reduced solve is stated in DESIGN.md §2.17, not taken from
// Eigen's SimplicialLDLT (whose AMD permutation cannot be pinned here).
#pragma once
#include "rsc_poseopt.h"
#if defined(__HIPCC__)
#include "rsc_fold.h"
#endif
#include <algorithm>
#include <cstring>
#include <vector>
#include "../../include/rsc.h"

namespace rsc {

constexpr int kLbaMaxFree = 64;         // free KeyFrames: a 384 x 384 reduced system
constexpr int kLbaMaxKFs = 64 + 4096;   // KeyFrames in all (free + fixed)
constexpr int kLbaMaxPoints = 16384;
constexpr int kLbaMaxEdges = 131072;
constexpr int kLbaTerms = 72;           // per active edge: Hll 9 | b_l 3 | Hpp 36 | b_p 6 | Hpl 18 (6 x 3)
constexpr int kLbaBranches = 12;

// branch record (counters only)
enum {
    kLbBrIter = 0,      // LM iterations
    kLbBrTrial,         // trials
    kLbBrNotOk2,        // reduced LDL^T met a zero pivot
    kLbBrChiNonFinite,  // tempChi NaN / Inf
    kLbBrRhoNaN,
    kLbBrRejected,
    kLbBrQmax,          // qmax == 10
    kLbBrRhoZero,
    kLbBrNBad,          // _nBad >= 3
    kLbBrNoActive,      // a phase without an active vertex (optimize() returns at once)
    kLbBrVertexDropped, // a vertex without a level-0 edge left the active set
    kLbBrStaleKept      // a level-1 edge that is not in vToErase (depth came back in phase 2)
};

struct LbaEdge {
    int32_t pt, kf;     // indices into the caller's lists
    float u, v, ur, inv;  // ur < 0: mono
};

// LM state of one optimize() and what the host reads of it after a trial
struct LbaCtl {
    double lambda, ni, currentChi, iniChi, tempChi, rho, scale;
    double chi_first, chi_last;
    int32_t nBad, qmax, ok2, accepted, again, stop, its, trials;
    int32_t br[kLbaBranches];
};

struct LbaDev {
    // the problem
    const LbaEdge* edge;     // [n_edges]
    const PoCam* cam;        // [n_kfs]
    const uint8_t* pt_bad;   // [n_points]
    // estimates, the backup of push(), the edges' _error and flags
    PoSE3* est_kf;           // [n_kfs]
    double* est_pt;          // [n_points][3]
    PoSE3* bak_kf;
    double* bak_pt;
    double* err;             // [n_edges][3]
    uint8_t* flags;          // [n_edges] bit 0 level 1, bit 1 in vToErase
    // the phase's plan
    const int32_t* ae;       // [na] active edges, ascending
    const uint8_t* robust;   // [na] the edge still has its kernel
    const int32_t* kf_hidx;  // [n_kfs] Hessian index of a free active KeyFrame, else -1
    const int32_t* pt_lidx;  // [n_points] landmark index of an active point, else -1
    const int32_t* hk;       // [F] KeyFrame of a Hessian index
    const int32_t* lp;       // [L] point of a landmark index
    const int32_t* pe_begin; // [L] the point's active edges are ae[pe_begin .. pe_end)
    const int32_t* pe_end;
    const int32_t* ke_begin; // [F + 1] ranges of ke_list / kl_list
    const int32_t* ke_list;  // active-edge positions of a free KeyFrame in edge order
    const int32_t* kl_list;  //   ... in ascending landmark index
    const int32_t* pf_begin; // [L + 1]
    const int32_t* pf_list;  // active-edge positions of a point's free-KeyFrame edges in ascending Hessian index
    const int32_t* slot;     // [F][L] active-edge position of (KeyFrame, point), else -1
    // work
    double* terms;           // [na][72]
    double* chi;             // [na] activeRobustChi2 terms
    double* Hll;             // [L][9]
    double* bl;              // [L][3]
    double* Hpp;             // [F][36]
    double* bp;              // [F][6]
    double* Dinv;            // [L][9]
    double* db;              // [L][3]
    double* S;               // [n][n] reduced system, then its factor
    double* bs;              // [n] bschur
    double* x;               // [n + 3L]
    double* sc;              // [n + 3L] computeScale terms
    LbaCtl* ctl;
    int32_t n_kfs, n_points, n_edges, na, F, L, n;  // n = 6 F
};

RSC_HD bool lba_stereo(const LbaEdge& e) { return !(e.ur < 0.0f); }

// Huber deltas: const float thHuberMono = sqrt(5.991), thHuberStereo = sqrt(7.815) (Optimizer.cpp:554-555)
RSC_HD double lba_delta(bool stereo) { return stereo ? (double)(float)sqrt(7.815) : (double)(float)sqrt(5.991); }

// computeError of the edge at the current estimates into D.err (and the caller's e)
RSC_HD void lba_error(const LbaDev& D, int ei, double (&e)[3]) {
    const LbaEdge ed = D.edge[ei];
    const double Xw[3] = {D.est_pt[3 * ed.pt], D.est_pt[3 * ed.pt + 1], D.est_pt[3 * ed.pt + 2]};
    po_error(D.est_kf[ed.kf], D.cam[ed.kf], Xw, (double)ed.u, (double)ed.v, (double)ed.ur, lba_stereo(ed), e[0], e[1],
             e[2]);
}

// linearizeOplus of EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ: A = _jacobianOplusXi (D x 3), B = _jacobianOplusXj
RSC_HD void lba_jacobians(const PoSE3& T, const PoCam& K, const double (&Xw)[3], bool stereo, double (&A)[3][3],
                          double (&B)[3][6]) {
    double p[3], R[3][3];
    po_map(T, Xw, p);
    po_quat_to_R(T.r, R);
    const double x = p[0], y = p[1], z = p[2];
    const double z_2 = z * z;
    const double fx = K.fx, fy = K.fy, bf = K.bf;
    if (!stereo) {
        // -1./z * tmp * R, tmp = [fx 0 -x/z*fx; 0 fy -y/z*fy]
        const double s = -1. / z;
        const double tmp[2][3] = {{fx, 0, -x / z * fx}, {0, fy, -y / z * fy}};
        RSC_UNROLL for (int r = 0; r < 2; ++r)
            RSC_UNROLL for (int c = 0; c < 3; ++c) {
                const double m0 = s * tmp[r][0], m1 = s * tmp[r][1], m2 = s * tmp[r][2];
                A[r][c] = (m0 * R[0][c] + m1 * R[1][c]) + m2 * R[2][c];
            }
        RSC_UNROLL for (int c = 0; c < 3; ++c) A[2][c] = 0.0;
    } else {
        RSC_UNROLL for (int c = 0; c < 3; ++c) {
            A[0][c] = -fx * R[0][c] / z + fx * x * R[2][c] / z_2;
            A[1][c] = -fy * R[1][c] / z + fy * y * R[2][c] / z_2;
            A[2][c] = A[0][c] - bf * R[2][c] / z_2;
        }
    }
    B[0][0] = x * y / z_2 * fx;
    B[0][1] = -(1 + (x * x / z_2)) * fx;
    B[0][2] = y / z * fx;
    B[0][3] = -1. / z * fx;
    B[0][4] = 0;
    B[0][5] = x / z_2 * fx;
    B[1][0] = (1 + y * y / z_2) * fy;
    B[1][1] = -x * y / z_2 * fy;
    B[1][2] = -x / z * fy;
    B[1][3] = 0;
    B[1][4] = -1. / z * fy;
    B[1][5] = y / z_2 * fy;
    if (stereo) {
        B[2][0] = B[0][0] - bf * y / z_2;
        B[2][1] = B[0][1] + bf * x / z_2;
        B[2][2] = B[0][2];
        B[2][3] = B[0][3];
        B[2][4] = 0;
        B[2][5] = B[0][5] - bf / z_2;
    } else {
        RSC_UNROLL for (int c = 0; c < 6; ++c) B[2][c] = 0.0;
    }
}

// sum over k < DD of a(k) * b(k), left to right
#define LBA_DOT(DD, a, b) ((DD) == 2 ? ((a(0)) * (b(0)) + (a(1)) * (b(1))) : (((a(0)) * (b(0)) + (a(1)) * (b(1))) + (a(2)) * (b(2))))

// BaseBinaryEdge::constructQuadraticForm (vertex 0 the point, vertex 1 the KeyFrame), as terms:
// t[0..8] A^T W A, t[9..11] A^T omega_r, and for a free KeyFrame t[12..47] B^T W B, t[48..53] B^T omega_r,
// t[54..71] the 6 x 3 block of Hpl, which the edge writes transposed (_hessianRowMajor): B^T (A^T omega)^T
// without a kernel, (B^T W) A with one.
template <int DD>
RSC_HD void lba_quad_terms(const double (&A)[3][3], const double (&B)[3][6], const double (&e)[3], double inv,
                           bool robust, double delta, bool kf_free, double* t) {
    double om[3][3];
    RSC_UNROLL for (int i = 0; i < 3; ++i)
        RSC_UNROLL for (int j = 0; j < 3; ++j) om[i][j] = (i == j) ? inv : 0.0;
    double orr[3] = {0.0, 0.0, 0.0};  // omega_r = -omega * _error
    RSC_UNROLL for (int i = 0; i < DD; ++i) {
#define LBA_A_(k) om[i][k]
#define LBA_B_(k) e[k]
        orr[i] = -LBA_DOT(DD, LBA_A_, LBA_B_);
#undef LBA_A_
#undef LBA_B_
    }
    double W[3][3];
    RSC_UNROLL for (int i = 0; i < 3; ++i)
        RSC_UNROLL for (int j = 0; j < 3; ++j) W[i][j] = om[i][j];
    if (robust) {
        double rho0, rho1;
        po_huber(po_chi2(inv, DD == 3, e[0], e[1], e[2]), delta, delta * delta, rho0, rho1);
        RSC_UNROLL for (int i = 0; i < 3; ++i)
            RSC_UNROLL for (int j = 0; j < 3; ++j) W[i][j] = rho1 * om[i][j];
        RSC_UNROLL for (int i = 0; i < DD; ++i) orr[i] *= rho1;
    }
    double AtW[3][3];  // A^T W (A^T omega without a kernel: W == omega then)
    RSC_UNROLL for (int i = 0; i < 3; ++i)
        RSC_UNROLL for (int k = 0; k < DD; ++k) {
#define LBA_A_(m) A[m][i]
#define LBA_B_(m) W[m][k]
            AtW[i][k] = LBA_DOT(DD, LBA_A_, LBA_B_);
#undef LBA_A_
#undef LBA_B_
        }
    RSC_UNROLL for (int i = 0; i < 3; ++i)
        RSC_UNROLL for (int j = 0; j < 3; ++j) {
#define LBA_A_(k) AtW[i][k]
#define LBA_B_(k) A[k][j]
            t[3 * i + j] = LBA_DOT(DD, LBA_A_, LBA_B_);
#undef LBA_A_
#undef LBA_B_
        }
    RSC_UNROLL for (int i = 0; i < 3; ++i) {
#define LBA_A_(k) A[k][i]
#define LBA_B_(k) orr[k]
        t[9 + i] = LBA_DOT(DD, LBA_A_, LBA_B_);
#undef LBA_A_
#undef LBA_B_
    }
    if (!kf_free) return;
    double BtW[6][3];
    RSC_UNROLL for (int i = 0; i < 6; ++i)
        RSC_UNROLL for (int k = 0; k < DD; ++k) {
#define LBA_A_(m) B[m][i]
#define LBA_B_(m) W[m][k]
            BtW[i][k] = LBA_DOT(DD, LBA_A_, LBA_B_);
#undef LBA_A_
#undef LBA_B_
        }
    RSC_UNROLL for (int i = 0; i < 6; ++i)
        RSC_UNROLL for (int j = 0; j < 6; ++j) {
#define LBA_A_(k) BtW[i][k]
#define LBA_B_(k) B[k][j]
            t[12 + 6 * i + j] = LBA_DOT(DD, LBA_A_, LBA_B_);
#undef LBA_A_
#undef LBA_B_
        }
    RSC_UNROLL for (int i = 0; i < 6; ++i) {
#define LBA_A_(k) B[k][i]
#define LBA_B_(k) orr[k]
        t[48 + i] = LBA_DOT(DD, LBA_A_, LBA_B_);
#undef LBA_A_
#undef LBA_B_
    }
    RSC_UNROLL for (int i = 0; i < 6; ++i)
        RSC_UNROLL for (int j = 0; j < 3; ++j) {
            // onto the block buildSystem cleared: 0.0 + the product
            if (robust) {
#define LBA_A_(k) BtW[i][k]
#define LBA_B_(k) A[k][j]
                t[54 + 3 * i + j] = 0.0 + LBA_DOT(DD, LBA_A_, LBA_B_);
#undef LBA_A_
#undef LBA_B_
            } else {
#define LBA_A_(k) B[k][i]
#define LBA_B_(k) AtW[j][k]
                t[54 + 3 * i + j] = 0.0 + LBA_DOT(DD, LBA_A_, LBA_B_);
#undef LBA_A_
#undef LBA_B_
            }
        }
}

// One active edge (position a of the phase's list): computeError, the edge's activeRobustChi2 term and,
// with `build`, linearizeOplus + constructQuadraticForm into its 72 terms.
RSC_HD void lba_edge_item(const LbaDev& D, int a, bool build) {
    const int ei = D.ae[a];
    const LbaEdge ed = D.edge[ei];
    const bool stereo = lba_stereo(ed), robust = D.robust[a] != 0;
    const double delta = lba_delta(stereo), inv = (double)ed.inv;
    double e[3];
    lba_error(D, ei, e);
    RSC_UNROLL for (int k = 0; k < 3; ++k) D.err[3 * (size_t)ei + k] = e[k];
    D.chi[a] = po_chi_term(robust, stereo, inv, e[0], e[1], e[2], delta, delta * delta);
    if (!build) return;
    const double Xw[3] = {D.est_pt[3 * ed.pt], D.est_pt[3 * ed.pt + 1], D.est_pt[3 * ed.pt + 2]};
    double A[3][3], B[3][6];
    lba_jacobians(D.est_kf[ed.kf], D.cam[ed.kf], Xw, stereo, A, B);
    // straight into the edge's terms (those of a fixed KeyFrame's pose part are never read)
    double* o = D.terms + (size_t)kLbaTerms * a;
    const bool kf_free = D.kf_hidx[ed.kf] >= 0;
    if (stereo) lba_quad_terms<3>(A, B, e, inv, robust, delta, kf_free, o);
    else lba_quad_terms<2>(A, B, e, inv, robust, delta, kf_free, o);
}

// Hll / b_l of landmark l, entry k of 12: the vertex's A() and b() summed over its edges in active-edge order
RSC_HD void lba_fold_point_item(const LbaDev& D, int l, int k) {
    double acc = 0.0;
    for (int a = D.pe_begin[l]; a < D.pe_end[l]; ++a) acc = acc + D.terms[(size_t)kLbaTerms * a + k];
    if (k < 9) D.Hll[9 * (size_t)l + k] = acc;
    else D.bl[3 * (size_t)l + (k - 9)] = acc;
}

// Hpp / b_p of pose h, entry k of 42
RSC_HD void lba_fold_kf_item(const LbaDev& D, int h, int k) {
    double acc = 0.0;
    for (int q = D.ke_begin[h]; q < D.ke_begin[h + 1]; ++q) acc = acc + D.terms[(size_t)kLbaTerms * D.ke_list[q] + 12 + k];
    if (k < 36) D.Hpp[36 * (size_t)h + k] = acc;
    else D.bp[6 * (size_t)h + (k - 36)] = acc;
}

// A left-to-right sum from 0.0
RSC_HD double lba_sum(const double* c, int m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return fold_run<false>(0.0, c, m);
#else
    double acc = 0.0;
    for (int i = 0; i < m; ++i) acc = acc + c[i];
    return acc;
#endif
}

// Head of OptimizationAlgorithmLevenberg::solve (one lane): currentChi, and at iteration 0 computeLambdaInit
RSC_HD void lba_ctl_begin(const LbaDev& D, int it) {
    LbaCtl& c = *D.ctl;
    const double chi = lba_sum(D.chi, D.na);
    c.currentChi = c.tempChi = c.iniChi = chi;
    if (it == 0) {
        double maxDiagonal = 0.;
        for (int h = 0; h < D.F; ++h)
            for (int j = 0; j < 6; ++j) {
                const double a = rabs(D.Hpp[36 * (size_t)h + 7 * j]);
                maxDiagonal = (a < maxDiagonal) ? maxDiagonal : a;  // std::max(fabs(..), maxDiagonal)
            }
        for (int l = 0; l < D.L; ++l)
            for (int j = 0; j < 3; ++j) {
                const double a = rabs(D.Hll[9 * (size_t)l + 4 * j]);
                maxDiagonal = (a < maxDiagonal) ? maxDiagonal : a;
            }
        c.lambda = 1e-5 * maxDiagonal;
        c.ni = 2;
        c.nBad = 0;
        c.chi_first = chi;
    }
    c.chi_last = chi;
    c.rho = 0;
    c.qmax = 0;
    c.its++;
    c.br[kLbBrIter]++;
}

// Dinv = (Hll + lambda I)^-1 and db = Dinv * b_l of landmark l
RSC_HD void lba_point_prep_item(const LbaDev& D, int l) {
    const double lambda = D.ctl->lambda;
    double M[3][3], Mi[3][3];
    RSC_UNROLL for (int i = 0; i < 3; ++i)
        RSC_UNROLL for (int j = 0; j < 3; ++j) {
            const double h = D.Hll[9 * (size_t)l + 3 * i + j];
            M[i][j] = (i == j) ? h + lambda : h;
        }
    inverse3(M, Mi);
    const double b0 = D.bl[3 * (size_t)l], b1 = D.bl[3 * (size_t)l + 1], b2 = D.bl[3 * (size_t)l + 2];
    RSC_UNROLL for (int i = 0; i < 3; ++i) {
        RSC_UNROLL for (int j = 0; j < 3; ++j) D.Dinv[9 * (size_t)l + 3 * i + j] = Mi[i][j];
        D.db[3 * (size_t)l + i] = emv3d_row(i, Mi[i][0] * b0, Mi[i][1] * b1, Mi[i][2] * b2);
    }
}

// Entry (r, c) of block (i1, i2 >= i1) of the reduced system: Hpp (+ lambda) on the diagonal block, then
// -= ((Bi Dinv) Bj^T)(r, c) over the landmarks both poses see, in ascending landmark index
RSC_HD void lba_schur_item(const LbaDev& D, int i1, int i2, int r, int c) {
    double acc = 0.0;
    if (i1 == i2) {
        const double h = D.Hpp[36 * (size_t)i1 + 6 * r + c];
        acc = acc + ((r == c) ? h + D.ctl->lambda : h);  // _Hpp->add(_Hschur) onto the cleared block
    }
    for (int q = D.ke_begin[i1]; q < D.ke_begin[i1 + 1]; ++q) {
        const int a1 = D.kl_list[q];
        const int l = D.pt_lidx[D.edge[D.ae[a1]].pt];
        const int a2 = (i1 == i2) ? a1 : D.slot[(size_t)i2 * D.L + l];
        if (a2 < 0) continue;
        const double* Bi = D.terms + (size_t)kLbaTerms * a1 + 54 + 3 * r;
        const double* Bj = D.terms + (size_t)kLbaTerms * a2 + 54 + 3 * c;
        const double* Di = D.Dinv + 9 * (size_t)l;
        double bd[3];
        RSC_UNROLL for (int k = 0; k < 3; ++k) bd[k] = (Bi[0] * Di[k] + Bi[1] * Di[3 + k]) + Bi[2] * Di[6 + k];
        acc = acc - ((bd[0] * Bj[0] + bd[1] * Bj[1]) + bd[2] * Bj[2]);
    }
    D.S[(size_t)(6 * i1 + r) * D.n + 6 * i2 + c] = acc;
}

// bschur entry r of pose i1: b_p - coefficients, coefficients += Bi db in ascending landmark index
RSC_HD void lba_bschur_item(const LbaDev& D, int i1, int r) {
    double acc = 0.0;
    for (int q = D.ke_begin[i1]; q < D.ke_begin[i1 + 1]; ++q) {
        const int a1 = D.kl_list[q];
        const int l = D.pt_lidx[D.edge[D.ae[a1]].pt];
        const double* Bi = D.terms + (size_t)kLbaTerms * a1 + 54 + 3 * r;
        const double* d = D.db + 3 * (size_t)l;
        acc = acc + ((Bi[0] * d[0] + Bi[1] * d[1]) + Bi[2] * d[2]);
    }
    D.bs[6 * i1 + r] = D.bp[6 * (size_t)i1 + r] - acc;
}

// ---- the reduced solve: LDL^T without pivoting over the upper triangle of S, in index
// order.  Right-looking form: step i divides row i by the pivot into column i below the diagonal
// (L(j, i) = U(i, j) / D_i) and subtracts L(j, i) U(i, k) from every U(j, k), i < j <= k: each entry meets
// its terms in ascending i, which is the order of the up-looking statement.
RSC_HD void lba_ldlt_scale_item(double* S, int n, int i, int j, double d) { S[(size_t)j * n + i] = S[(size_t)i * n + j] / d; }
RSC_HD void lba_ldlt_update_item(double* S, int n, int i, int j, int k) {
    S[(size_t)j * n + k] = S[(size_t)j * n + k] - S[(size_t)j * n + i] * S[(size_t)i * n + k];
}

// Back-substitution cl = b_l - Hpl^T (-x_p), x_l = Dinv cl of landmark l, the update of its estimate (push
// first) and its computeScale terms.  `solved` false: x keeps what it held (the solver returned before
// writing it).
RSC_HD void lba_point_update_item(const LbaDev& D, int l) {
    const int n = D.n;
    const bool solved = D.ctl->ok2 != 0;
    double* xl = D.x + n + 3 * (size_t)l;
    if (solved) {
        double cl[3] = {D.bl[3 * (size_t)l], D.bl[3 * (size_t)l + 1], D.bl[3 * (size_t)l + 2]};
        for (int q = D.pf_begin[l]; q < D.pf_begin[l + 1]; ++q) {
            const int a = D.pf_list[q];
            const int h = D.kf_hidx[D.edge[D.ae[a]].kf];
            const double* Bi = D.terms + (size_t)kLbaTerms * a + 54;
            RSC_UNROLL for (int j = 0; j < 3; ++j) {  // atxpy: y += A^T x
                double s = Bi[j] * (-D.x[6 * h]);
                RSC_UNROLL for (int r = 1; r < 6; ++r) s = s + Bi[3 * r + j] * (-D.x[6 * h + r]);
                cl[j] = cl[j] + s;
            }
        }
        const double* Di = D.Dinv + 9 * (size_t)l;
        RSC_UNROLL for (int i = 0; i < 3; ++i)
            xl[i] = 0.0 + emv3d_row(i, Di[3 * i] * cl[0], Di[3 * i + 1] * cl[1], Di[3 * i + 2] * cl[2]);
    }
    const int p = D.lp[l];
    const double lambda = D.ctl->lambda;
    RSC_UNROLL for (int i = 0; i < 3; ++i) {
        D.bak_pt[3 * (size_t)p + i] = D.est_pt[3 * (size_t)p + i];
        D.est_pt[3 * (size_t)p + i] = D.est_pt[3 * (size_t)p + i] + xl[i];  // VertexSBAPointXYZ::oplusImpl
        D.sc[n + 3 * (size_t)l + i] = xl[i] * (lambda * xl[i] + D.bl[3 * (size_t)l + i]);
    }
}

// Pose h: push, VertexSE3Expmap::oplusImpl, computeScale terms
RSC_HD void lba_kf_update_item(const LbaDev& D, int h) {
    const int k = D.hk[h];
    const double lambda = D.ctl->lambda;
    double u[6];
    RSC_UNROLL for (int i = 0; i < 6; ++i) {
        u[i] = D.x[6 * h + i];
        D.sc[6 * h + i] = u[i] * (lambda * u[i] + D.bp[6 * (size_t)h + i]);
    }
    const PoSE3 est = D.est_kf[k];
    D.bak_kf[k] = est;
    D.est_kf[k] = po_mul(po_exp(u), est);
}

// pop(): the estimates of before the trial
RSC_HD void lba_restore_item(const LbaDev& D, int i) {
    if (i < D.F) {
        const int k = D.hk[i];
        D.est_kf[k] = D.bak_kf[k];
    } else {
        const int p = D.lp[i - D.F];
        RSC_UNROLL for (int j = 0; j < 3; ++j) D.est_pt[3 * (size_t)p + j] = D.bak_pt[3 * (size_t)p + j];
    }
}

// Tail of one Levenberg trial (one lane): tempChi, rho, the lambda schedule and the exits of solve()
RSC_HD void lba_ctl_trial(const LbaDev& D) {
    LbaCtl& c = *D.ctl;
    c.trials++;
    c.br[kLbBrTrial]++;
    const double chiT = lba_sum(D.chi, D.na);
    c.tempChi = c.ok2 ? chiT : DBL_MAX;
    if (!c.ok2) c.br[kLbBrNotOk2]++;
    if (!(rabs(c.tempChi) <= DBL_MAX)) c.br[kLbBrChiNonFinite]++;
    double rho = c.currentChi - c.tempChi;
    double scale = lba_sum(D.sc, D.n + 3 * D.L);
    scale += 1e-3;
    rho /= scale;
    c.scale = scale;
    if (rho != rho) c.br[kLbBrRhoNaN]++;
    if (rho > 0 && rabs(c.tempChi) <= DBL_MAX) {
        double alpha = 1. - po_cube(2 * rho - 1);
        alpha = (2. / 3. < alpha) ? 2. / 3. : alpha;
        const double scaleFactor = (1. / 3. < alpha) ? alpha : 1. / 3.;
        c.lambda *= scaleFactor;
        c.ni = 2;
        c.currentChi = c.tempChi;
        c.accepted = 1;
    } else {
        c.lambda *= c.ni;
        c.ni *= 2;
        c.accepted = 0;
        c.br[kLbBrRejected]++;
    }
    c.rho = rho;
    c.qmax++;
    c.chi_last = c.currentChi;
    c.again = (rho < 0 && c.qmax < 10) ? 1 : 0;
    c.stop = 0;
    if (!c.again) {
        if (c.qmax == 10 || rho == 0) {
            c.stop = 1;
            c.br[c.qmax == 10 ? kLbBrQmax : kLbBrRhoZero]++;
        } else {
            if ((c.iniChi - c.currentChi) * 1e3 < c.iniChi) c.nBad++;
            else c.nBad = 0;
            if (c.nBad >= 3) {
                c.stop = 1;
                c.br[kLbBrNBad]++;
            }
        }
    }
}

// The classification loops (Optimizer.cpp:665-697 after phase 1, :712-741 at the end) for edge ei: chi2() of the
// edge's stored _error, isDepthPositive() at the current estimates.
RSC_HD void lba_classify_item(const LbaDev& D, int ei, int phase) {
    const LbaEdge ed = D.edge[ei];
    if (D.pt_bad[ed.pt]) return;
    const bool stereo = lba_stereo(ed);
    const double chi2 = po_chi2((double)ed.inv, stereo, D.err[3 * (size_t)ei], D.err[3 * (size_t)ei + 1], D.err[3 * (size_t)ei + 2]);
    const double Xw[3] = {D.est_pt[3 * ed.pt], D.est_pt[3 * ed.pt + 1], D.est_pt[3 * ed.pt + 2]};
    double p[3];
    po_map(D.est_kf[ed.kf], Xw, p);
    const bool out = chi2 > (stereo ? 7.815 : 5.991) || !(p[2] > 0.0);
    if (out) D.flags[ei] = (uint8_t)(D.flags[ei] | (phase == 0 ? 1 : 2));
}

// Converter::toSE3Quat of a float pose (rows 0..2 of the row-major Tcw)
RSC_HD PoSE3 lba_pose_in(const float* T) {
    double R[3][3], t[3];
    RSC_UNROLL for (int r = 0; r < 3; ++r) {
        RSC_UNROLL for (int c = 0; c < 3; ++c) R[r][c] = (double)T[4 * r + c];
        t[r] = (double)T[4 * r + 3];
    }
    return po_from_Rt(R, t);
}

// Converter::toIso of an estimate, as float
RSC_HD void lba_pose_out(const PoSE3& s, float* T) {
    double R[3][3];
    po_quat_to_R(s.r, R);
    RSC_UNROLL for (int r = 0; r < 3; ++r) {
        RSC_UNROLL for (int c = 0; c < 3; ++c) T[4 * r + c] = (float)R[r][c];
        T[4 * r + 3] = (float)s.t[r];
    }
    T[12] = T[13] = T[14] = 0.0f;
    T[15] = 1.0f;
}

// ---- host: the problem as plain arrays, the plan of a phase, the driver ---------------------------
struct LbaProblem {  // mirrors rsc_localba_problem
    int n_kfs = 0;
    const int64_t* kf_id = nullptr;
    const uint8_t* kf_fixed = nullptr;
    const float* Tcw = nullptr;   // [n_kfs][16]
    const float* cam = nullptr;   // [n_kfs][5] fx fy cx cy bf
    int n_points = 0;
    const int64_t* mp_id = nullptr;
    const float* pos = nullptr;
    const uint8_t* bad = nullptr;
    const int32_t* obs_begin = nullptr;
    const int32_t* obs_kf = nullptr;
    const float* uv = nullptr;
    const float* u_right = nullptr;
    const float* inv_sigma2 = nullptr;
};

struct LbaPhaseStat {
    int32_t n_vertices = 0, n_points = 0, n_edges = 0, n_free = 0, its = 0, trials = 0, ran = 0;
    double chi_first = 0.0, chi_last = 0.0;
};

// The active sets and index maps of initializeOptimization(level 0) + buildIndexMapping, and the walk lists
struct LbaPlan {
    std::vector<int32_t> ae, kf_hidx, pt_lidx, hk, lp, pe_begin, pe_end, ke_begin, ke_list, kl_list, pf_begin, pf_list, slot;
    std::vector<uint8_t> robust;
    int F = 0, L = 0, n_active_kfs = 0, dropped = 0;
};

// rank of every element by id (ids unique)
inline std::vector<int32_t> lba_order_by_id(const int64_t* id, int n) {
    std::vector<int32_t> o((size_t)n);
    for (int i = 0; i < n; ++i) o[i] = i;
    std::sort(o.begin(), o.end(), [&](int a, int b) { return id[a] < id[b]; });
    return o;
}

// flags: bit 0 = level 1.  phase 0: every edge has its kernel; phase 1: only the edges of bad points keep it.
inline void lba_plan(const LbaProblem& P, const std::vector<LbaEdge>& E, const uint8_t* flags, int phase, LbaPlan& Q) {
    const int ne = (int)E.size();
    Q = LbaPlan();
    std::vector<int32_t> kf_edges((size_t)P.n_kfs, 0), pt_edges((size_t)P.n_points, 0);
    std::vector<int32_t> kf_all((size_t)P.n_kfs, 0), pt_all((size_t)P.n_points, 0);
    for (int e = 0; e < ne; ++e) {
        ++kf_all[E[e].kf];
        ++pt_all[E[e].pt];
        if (flags[e] & 1) continue;
        Q.ae.push_back(e);
        Q.robust.push_back((phase == 0 || P.bad[E[e].pt]) ? 1 : 0);
        ++kf_edges[E[e].kf];
        ++pt_edges[E[e].pt];
    }
    // Hessian indices: the active vertices sorted by id, poses first (buildIndexMapping)
    Q.kf_hidx.assign((size_t)P.n_kfs, -1);
    Q.pt_lidx.assign((size_t)P.n_points, -1);
    for (int k : lba_order_by_id(P.kf_id, P.n_kfs)) {
        if (kf_edges[k] == 0) {
            Q.dropped += (kf_all[k] > 0);
            continue;
        }
        ++Q.n_active_kfs;
        if (P.kf_fixed[k]) continue;
        Q.kf_hidx[k] = (int)Q.hk.size();
        Q.hk.push_back(k);
    }
    for (int p : lba_order_by_id(P.mp_id, P.n_points)) {
        if (pt_edges[p] == 0) {
            Q.dropped += (pt_all[p] > 0);
            continue;
        }
        Q.pt_lidx[p] = (int)Q.lp.size();
        Q.lp.push_back(p);
    }
    Q.F = (int)Q.hk.size();
    Q.L = (int)Q.lp.size();
    const int na = (int)Q.ae.size();
    Q.pe_begin.assign((size_t)Q.L, 0);
    Q.pe_end.assign((size_t)Q.L, 0);
    Q.ke_begin.assign((size_t)Q.F + 1, 0);
    Q.pf_begin.assign((size_t)Q.L + 1, 0);
    Q.slot.assign((size_t)Q.F * Q.L, -1);
    for (int a = na - 1; a >= 0; --a) Q.pe_begin[Q.pt_lidx[E[Q.ae[a]].pt]] = a;  // the point's edges are contiguous
    for (int a = 0; a < na; ++a) Q.pe_end[Q.pt_lidx[E[Q.ae[a]].pt]] = a + 1;
    for (int a = 0; a < na; ++a) {
        const int h = Q.kf_hidx[E[Q.ae[a]].kf], l = Q.pt_lidx[E[Q.ae[a]].pt];
        if (h < 0) continue;
        ++Q.ke_begin[h + 1];
        ++Q.pf_begin[l + 1];
        Q.slot[(size_t)h * Q.L + l] = a;
    }
    for (int h = 0; h < Q.F; ++h) Q.ke_begin[h + 1] += Q.ke_begin[h];
    for (int l = 0; l < Q.L; ++l) Q.pf_begin[l + 1] += Q.pf_begin[l];
    Q.ke_list.assign((size_t)Q.ke_begin[Q.F], 0);
    Q.kl_list.assign((size_t)Q.ke_begin[Q.F], 0);
    Q.pf_list.assign((size_t)Q.pf_begin[Q.L], 0);
    std::vector<int32_t> cur(Q.ke_begin.begin(), Q.ke_begin.end() - 1);
    for (int a = 0; a < na; ++a) {
        const int h = Q.kf_hidx[E[Q.ae[a]].kf];
        if (h >= 0) Q.ke_list[cur[h]++] = a;
    }
    // by ascending landmark / Hessian index: the slot table read in index order
    int q = 0;
    for (int h = 0; h < Q.F; ++h)
        for (int l = 0; l < Q.L; ++l)
            if (Q.slot[(size_t)h * Q.L + l] >= 0) Q.kl_list[q++] = Q.slot[(size_t)h * Q.L + l];
    q = 0;
    for (int l = 0; l < Q.L; ++l)
        for (int h = 0; h < Q.F; ++h)
            if (Q.slot[(size_t)h * Q.L + l] >= 0) Q.pf_list[q++] = Q.slot[(size_t)h * Q.L + l];
}

// What the argument check refuses (0: fine; else a text for rsc_status_string and the status)
inline const char* lba_check(const LbaProblem& P, int& status) {
    status = -1;  // RSC_ERR_ARG
    if (P.n_kfs < 0 || P.n_points < 0) return "negative count";
    if (P.n_kfs && (!P.kf_id || !P.kf_fixed || !P.Tcw || !P.cam)) return "a KeyFrame array is NULL";
    if (P.n_points && (!P.mp_id || !P.pos || !P.bad || !P.obs_begin)) return "a point array is NULL";
    const int ne = P.n_points ? P.obs_begin[P.n_points] : 0;
    if (P.n_points) {
        if (P.obs_begin[0] != 0) return "obs_begin[0] is not 0";
        for (int p = 0; p < P.n_points; ++p)
            if (P.obs_begin[p + 1] < P.obs_begin[p]) return "obs_begin not ascending";
    }
    if (ne && (!P.obs_kf || !P.uv || !P.u_right || !P.inv_sigma2)) return "an edge array is NULL";
    {
        std::vector<int64_t> ids(P.kf_id, P.kf_id + P.n_kfs);
        std::sort(ids.begin(), ids.end());
        if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return "kf_id not unique";
        ids.assign(P.mp_id, P.mp_id + P.n_points);
        std::sort(ids.begin(), ids.end());
        if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return "mp_id not unique";
    }
    std::vector<int32_t> seen((size_t)P.n_kfs, -1);
    for (int p = 0; p < P.n_points; ++p)
        for (int e = P.obs_begin[p]; e < P.obs_begin[p + 1]; ++e) {
            const int k = P.obs_kf[e];
            if (k < 0 || k >= P.n_kfs) return "obs_kf out of range";
            if (seen[k] == p) return "a point names a KeyFrame twice";
            seen[k] = p;
        }
    status = -4;  // RSC_ERR_UNSUPPORTED
    int nfree = 0;
    for (int k = 0; k < P.n_kfs; ++k) nfree += P.kf_fixed[k] ? 0 : 1;
    if (nfree > kLbaMaxFree) return "more than RSC_LOCALBA_MAX_FREE_KFS (64) free KeyFrames";
    if (P.n_kfs > kLbaMaxKFs) return "more than RSC_LOCALBA_MAX_KFS (4160) KeyFrames";
    if (P.n_points > kLbaMaxPoints) return "more than RSC_LOCALBA_MAX_POINTS (16384) points";
    if (ne > kLbaMaxEdges) return "more than RSC_LOCALBA_MAX_EDGES (131072) edges";
    status = 0;
    return nullptr;
}

inline std::vector<LbaEdge> lba_edges(const LbaProblem& P) {
    std::vector<LbaEdge> E;
    for (int p = 0; p < P.n_points; ++p)
        for (int e = P.obs_begin[p]; e < P.obs_begin[p + 1]; ++e)
            E.push_back(LbaEdge{p, P.obs_kf[e], P.uv[2 * e], P.uv[2 * e + 1], P.u_right[e], P.inv_sigma2[e]});
    return E;
}

// The two optimize() calls over a backend B:
//   int  begin_phase(const LbaPlan&, int phase)   the plan reaches the stages; LbaCtl cleared
//   void edges(bool build) / fold() / ctl_begin(int it) / point_prep() / schur() / solve() / update() / ctl_trial()
//   void restore() / classify(int phase)
//   int  read_flags(int32_t out[3])               accepted, again, stop of the trial just closed
//   int  end_phase(LbaCtl&)                       the phase's LM record
//   int  get_edge_flags(uint8_t*)                 the level bits, for the second plan
// Every call returns a status (0 fine) that ends the run.
template <class B>
inline int lba_drive(B& be, const LbaProblem& P, const std::vector<LbaEdge>& E, LbaPhaseStat (&stat)[2], int32_t (&br)[kLbaBranches]) {
    std::vector<uint8_t> flags(E.size(), 0);
    for (int k = 0; k < kLbaBranches; ++k) br[k] = 0;
    for (int phase = 0; phase < 2; ++phase) {
        LbaPlan Q;
        lba_plan(P, E, flags.data(), phase, Q);
        LbaPhaseStat& st = stat[phase];
        st = LbaPhaseStat();
        st.n_vertices = Q.n_active_kfs + Q.L;
        st.n_points = Q.L;
        st.n_free = Q.F;
        st.n_edges = (int)Q.ae.size();
        br[kLbBrVertexDropped] += Q.dropped;
        // initializeOptimization() fails without an edge, optimize() returns without an index mapping
        if (Q.ae.empty()) {
            br[kLbBrNoActive]++;
        } else {
            st.ran = 1;
            if (int e = be.begin_phase(Q, phase)) return e;
            const int iters = phase == 0 ? 5 : 10;
            bool ok = true;
            for (int it = 0; it < iters && ok; ++it) {
                if (int e = be.edges(true)) return e;
                if (int e = be.fold()) return e;
                if (int e = be.ctl_begin(it)) return e;
                int32_t f[3] = {0, 0, 0};
                do {
                    if (int e = be.point_prep()) return e;
                    if (int e = be.schur()) return e;
                    if (int e = be.solve()) return e;
                    if (int e = be.update()) return e;
                    if (int e = be.edges(false)) return e;
                    if (int e = be.ctl_trial()) return e;
                    if (int e = be.read_flags(f)) return e;
                    if (!f[0])
                        if (int e = be.restore()) return e;
                } while (f[1]);
                ok = !f[2];
            }
            LbaCtl c;
            if (int e = be.end_phase(c)) return e;
            st.its = c.its;
            st.trials = c.trials;
            st.chi_first = c.chi_first;
            st.chi_last = c.chi_last;
            for (int k = 0; k < kLbaBranches; ++k) br[k] += c.br[k];
        }
        if (int e = be.classify(phase)) return e;
        if (phase == 0)
            if (int e = be.get_edge_flags(flags.data())) return e;
    }
    return 0;
}

struct LbaOut {  // any member may be null
    float* Tcw;
    float* pos;
    uint8_t* edge_flags;
    int32_t* erase;
};

// Recovery (Optimizer.cpp:768-784) and vToErase (:708-741: the mono edges, then the stereo ones, each in edge order)
inline void lba_finish(const LbaProblem& P, const std::vector<LbaEdge>& E, const PoSE3* est_kf, const double* est_pt,
                       const uint8_t* flags, const LbaOut& out, int32_t& n_erase, int32_t& n_level1, int32_t& stale_kept) {
    if (out.Tcw)
        for (int k = 0; k < P.n_kfs; ++k) {
            if (P.kf_fixed[k]) std::memcpy(out.Tcw + 16 * (size_t)k, P.Tcw + 16 * (size_t)k, 64);
            else lba_pose_out(est_kf[k], out.Tcw + 16 * (size_t)k);
        }
    if (out.pos)
        for (size_t i = 0; i < 3 * (size_t)P.n_points; ++i) out.pos[i] = (float)est_pt[i];
    n_erase = n_level1 = stale_kept = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (int e = 0; e < (int)E.size(); ++e) {
            if ((int)lba_stereo(E[e]) != pass) continue;
            if (out.edge_flags) out.edge_flags[e] = flags[e];
            n_level1 += flags[e] & 1;
            if ((flags[e] & 3) == 1) ++stale_kept;
            if (flags[e] & 2) {
                if (out.erase) out.erase[n_erase] = e;
                ++n_erase;
            }
        }
}

inline LbaProblem lba_problem(const rsc_localba_problem& q) {
    LbaProblem P;
    P.n_kfs = q.n_kfs; P.kf_id = q.kf_id; P.kf_fixed = q.fixed; P.Tcw = q.Tcw; P.cam = q.cam;
    P.n_points = q.n_points; P.mp_id = q.mp_id; P.pos = q.pos; P.bad = q.bad;
    P.obs_begin = q.obs_begin; P.obs_kf = q.obs_kf; P.uv = q.uv; P.u_right = q.u_right; P.inv_sigma2 = q.inv_sigma2;
    return P;
}

// The initial estimates: Converter::toSE3Quat(GetPose()), GetWorldPos().cast<double>()
inline void lba_initial(const LbaProblem& P, std::vector<PoSE3>& kf, std::vector<PoCam>& cam, std::vector<double>& pt) {
    kf.resize((size_t)P.n_kfs);
    cam.resize((size_t)P.n_kfs);
    for (int k = 0; k < P.n_kfs; ++k) {
        kf[k] = lba_pose_in(P.Tcw + 16 * (size_t)k);
        const float* c = P.cam + 5 * (size_t)k;
        cam[k] = PoCam{(double)c[0], (double)c[1], (double)c[2], (double)c[3], (double)c[4]};
    }
    pt.resize(3 * (size_t)P.n_points);
    for (size_t i = 0; i < pt.size(); ++i) pt[i] = (double)P.pos[i];
}

// One checked problem over a backend (see lba_drive; plus int get_state(PoSE3* kf, double* pt, uint8_t* flags))
template <class B>
inline int lba_run(B& be, const LbaProblem& P, const std::vector<LbaEdge>& E, const rsc_localba_out* out,
                   rsc_localba_result* res) {
    LbaPhaseStat st[2];
    int32_t br[kLbaBranches];
    if (int e = lba_drive(be, P, E, st, br)) return e;
    std::vector<PoSE3> kf((size_t)P.n_kfs);
    std::vector<double> pt(3 * (size_t)P.n_points);
    std::vector<uint8_t> flags(E.size());
    if (int e = be.get_state(kf.data(), pt.data(), flags.data())) return e;
    LbaOut o{nullptr, nullptr, nullptr, nullptr};
    if (out) o = LbaOut{out->Tcw, out->pos, out->edge_flags, out->erase};
    int32_t n_erase, n_level1, stale;
    lba_finish(P, E, kf.data(), pt.data(), flags.data(), o, n_erase, n_level1, stale);
    if (res) {
        std::memset(res, 0, sizeof(*res));
        res->n_erase = n_erase;
        res->n_level1 = n_level1;
        res->status = (st[0].ran ? 0 : RSC_LOCALBA_NO_EDGE_1) | (st[1].ran ? 0 : RSC_LOCALBA_NO_EDGE_2) |
                      (st[0].ran && st[0].n_free == 0 ? RSC_LOCALBA_NO_FREE_KF : 0);
        for (int p = 0; p < 2; ++p) {
            rsc_localba_phase& q = res->phase[p];
            q.n_vertices = st[p].n_vertices; q.n_points = st[p].n_points; q.n_edges = st[p].n_edges;
            q.lm_iterations = st[p].its; q.lm_trials = st[p].trials;
            q.chi2_first = st[p].chi_first; q.chi2_last = st[p].chi_last;
        }
        br[kLbBrStaleKept] = stale;
        for (int k = 0; k < kLbaBranches; ++k) res->branches[k] = br[k];
    }
    return 0;
}

#if defined(__HIPCC__)
// stage launchers (localba.hip)
hipError_t launch_lba_edges(const LbaDev& D, bool build, hipStream_t st);
hipError_t launch_lba_fold(const LbaDev& D, hipStream_t st);
hipError_t launch_lba_ctl_begin(const LbaDev& D, int it, hipStream_t st);
hipError_t launch_lba_point_prep(const LbaDev& D, hipStream_t st);
hipError_t launch_lba_schur(const LbaDev& D, hipStream_t st);
hipError_t launch_lba_solve(const LbaDev& D, hipStream_t st);
hipError_t launch_lba_update(const LbaDev& D, hipStream_t st);
hipError_t launch_lba_ctl_trial(const LbaDev& D, hipStream_t st);
hipError_t launch_lba_restore(const LbaDev& D, hipStream_t st);
hipError_t launch_lba_classify(const LbaDev& D, int phase, hipStream_t st);
#endif

}  // namespace rsc
