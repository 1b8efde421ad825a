/*
 * rsc.h — C ABI of the MI355X RANSAC pose engine (librsc.so).
 *
 * Drop-in boundary for the hot path of Luigi940260/orb-slam2-optimized: the geometric RANSAC
 * solvers called by Tracking::Relocalization() and LoopClosing::ComputeSim3().  Every entry point
 * below replaces one member of the reference classes (file:line of the reference cited per
 * function); the C++ facade in orb-slam2-optimized_amd/csrc/facade/ re-exposes them with the
 * reference's exact class signatures.  Plain pointers and sizes only; no torch / HIP types.
 *
 * Semantics are the reference's, including its quirks.  rand(): by default
 * every solver owns a glibc stream seeded with `seed` (H4: identical to srand(seed) right before that
 * solver runs alone); solvers bound to an rsc_stream (rsc_*_bind_stream) instead draw from ONE shared
 * stream in call order, the reference's process-global rand() (Q3, Random.cpp:47-50).
 *
 * Status codes: 0 = ok, < 0 = error (see rsc_status_string).  The library fails loudly: when no
 * HIP device is present, rsc_context_create returns RSC_ERR_NODEVICE; there is no CPU fallback.
 */
#ifndef RSC_H_
#define RSC_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSC_OK 0
#define RSC_ERR_ARG (-1)
#define RSC_ERR_HIP (-2)
#define RSC_ERR_OOM (-3)
#define RSC_ERR_UNSUPPORTED (-4)
#define RSC_ERR_NODEVICE (-5)
#define RSC_ERR_INTERNAL (-6) /* an engine invariant failed (a bug; rsc_status_string says which) */

typedef struct rsc_context rsc_context;
typedef struct rsc_pnp rsc_pnp;
typedef struct rsc_sim3 rsc_sim3;
typedef struct rsc_mlpnp rsc_mlpnp;
typedef struct rsc_stream rsc_stream;

/* ---- library / context ------------------------------------------------------------------ */
int rsc_version(void);
const char* rsc_status_string(int status);
/* One context per host thread (reference: the Tracking and LoopClosing threads each own their
 * solvers, System.cpp:58-69).  Owns a HIP stream, the rand() jump table and work buffers. */
int rsc_context_create(int device, rsc_context** out);
void rsc_context_destroy(rsc_context* ctx);
/* Use a caller-owned hipStream_t (e.g. torch's current stream) instead of the private one. */
int rsc_context_set_stream(rsc_context* ctx, void* hip_stream);
int rsc_context_synchronize(rsc_context* ctx);
/* Per-kernel timing of the last iterate call, in milliseconds (HIP events on the context stream):
 * out[0] = hypothesis-solve kernels, out[1] = inlier-scan kernels, out[2] = refine kernels,
 * out[3] = number of solve launches, out[4] = hypotheses solved. */
int rsc_context_last_timing(rsc_context* ctx, double out[5]);
/* As above plus out[5] = eigen-stage kernel (pnp_eig_group/lane_kernel) alone, split solve modes. */
int rsc_context_last_kernel_timing(rsc_context* ctx, double out[6]);
/* Diagnostic: host clock of the last rsc_pnp_iterate_many in microseconds from entry to
 * [0] first launch, [1] kernels enqueued, [2] results back on the host, [3] return. */
int rsc_diag_host_timing(rsc_context* ctx, double out[4]);
int rsc_context_enable_timing(rsc_context* ctx, int enable);
/* Eigen-stage form of the EPnP hypothesis solve (no effect on results): launches whose eigen stage
 * has at most max_workgroups workgroups of 20 hypotheses run it in the Refine's rows form (a 12-lane
 * group per hypothesis, Q rows in VGPRs: lower latency for small, latency-bound launches such as one
 * relocalization event); larger launches use the split form (below).  Default 64 (env RSC_EIG_ROWS
 * overrides); 0 = never the rows form. */
int rsc_context_set_eig_rows(rsc_context* ctx, int max_workgroups);
/* Eigen-stage form of the launches the rows form does not take: 1 (default; env RSC_EIG_SPLIT) the
 * split form — the QR chase and the Q rotations on two waves of one SIMD (pnp_eig_split_kernel) — or
 * 0 the lane-pair form (pnp_eig_group_kernel).  Both are bit-identical. */
int rsc_context_set_eig_split(rsc_context* ctx, int on);
/* Descriptor path of the PnP speculation round (no effect on results): 1 (default; env
 * RSC_ROUND_ARGS) the round's per-solver records travel in the kernels' argument blocks, the 31-word
 * rand() windows follow from the seeds on the device and the problem table stays resident between
 * rounds (uploaded only when it changes); 0 every round uploads its descriptors as one blob.  Rounds
 * of more than 64 solvers, and rounds with a solver whose rand() window has moved off its seed (or
 * that is bound to a shared stream), take the blob path whatever the setting. */
int rsc_context_set_round_args(rsc_context* ctx, int on);
/* PnP inlier scan (no effect on results): 1 (default; env RSC_SCAN_BOUND) a hypothesis that can no
 * longer reach mRansacMinInliers after the first half of the scan thread's point slices (the first
 * min(N, 128 PPT) correspondences) is not tested against the rest, and its stored count is the count
 * so far, which is below mRansacMinInliers; iterate() only ever tests a count against that bound
 * (PnPsolver.cpp:147).  0: every hypothesis is counted over all correspondences. */
int rsc_context_set_scan_bound(rsc_context* ctx, int on);
/* Diagnostic: PnP speculation rounds of the context so far on [0] the argument path, [1] the blob
 * path, and [2] uploads of the resident problem table. */
int rsc_diag_round_paths(rsc_context* ctx, int64_t out[3]);
/* Form of rsc_optimize_sim3_many (no effect on results): helpers > 0 runs each pair on one master
 * workgroup plus that many helper workgroups that evaluate the edges' numeric Jacobians in chunks
 * (the cooperative form); 0 one workgroup per pair; -1 (default; env RSC_SO_HELPERS) as many helpers
 * as fit one workgroup per CU, at most 7 per pair.  Bit-identical results. */
int rsc_context_set_sim3opt_helpers(rsc_context* ctx, int helpers);
/* Self-test of the device libm restatement (rsc_math.h, used by Sim3 angles, MLPnP, SearchBySim3):
 * out[i] = f(x[i]) computed ON THE GPU, f = 0 sin, 1 cos, 2 acos, 3 cbrt, 4 log, 5 logf
 * ((float)x[i] in, float result widened); and the eigen-solver chase's short-chain forms
 * (rsc_core.h): 6 sqrt for x in [1,4), 7 1/x for |x| in [1,2), 8 / 9 make_givens(x[i],
 * x[(i+n/2)%n]) c / s; 10 qr_solve_6x4 (PnPsolver.cpp:693-796) on records of 34 doubles
 * (A[6][4] row-major, b[6], previous X[4]) -> X in out[0..3], 1/0 success in out[4] of each record
 * (n a multiple of 34); 11 pow(x, 1.0/3.0), 12 pow(x, 3.0/2.0) as MLPnP computes them (x >= 0;
 * MLPnPsolver.cpp:567, :839, :901); 13 the PnP scan's float reciprocal of (float)x (v_rcp_f32 + one
 * Newton step, PnPsolver.cpp:251); (14, 15 unused); 16 the LM steps' 6 x 6 LDLT solve in its scalar and row-per-lane forms
 * (records of 42: matrix row-major + b in, x / ok of each form out; n a multiple of 42).  Host
 * pointers, n >= 0.  Tests compare with glibc / IEEE numpy / the oracle. */
int rsc_selftest_math(rsc_context* ctx, int fn, const double* x, int n, double* out);

/* ---- PnPsolver (include/PnPsolver.hpp:21-138, src/PnPsolver.cpp) ------------------------------ */
typedef struct {
    int32_t n;               /* compacted valid matches N (PnPsolver.cpp:22-44) */
    int32_t n_points;        /* vpMapPointMatches.size(): length of the returned inlier vector */
    const float* p2d;        /* [n][2] mvP2D = mvKeysUn[i].pt                       (:33) */
    const float* p3dw;       /* [n][3] mvP3Dw = MapPoint::GetWorldPos()             (:36) */
    const float* sigma2;     /* [n] mvSigma2 = mvLevelSigma2[kp.octave]             (:34) */
    const int32_t* kp_index; /* [n] mvKeyPointIndices; NULL = identity               (:38) */
    float fx, fy, cx, cy;    /* Frame::fx,fy,cx,cy (static float members, :47-50)       */
} rsc_pnp_problem;

typedef struct {
    int32_t ok;         /* iterate()/find() return value */
    int32_t no_more;    /* bNoMore */
    int32_t n_inliers;  /* nInliers */
    int32_t iterations; /* mnIterations after the call */
    float T[16];        /* row-major Tcw; written only when ok (PnPsolver.cpp:166,185) */
} rsc_pnp_result;

/* PnPsolver::PnPsolver (PnPsolver.cpp:11-55).  Copies the arrays to HBM. */
int rsc_pnp_create(rsc_context* ctx, const rsc_pnp_problem* problem, uint32_t seed, rsc_pnp** out);
void rsc_pnp_destroy(rsc_pnp* s);
/* PnPsolver::SetRansacParameters (PnPsolver.cpp:58-94; defaults 0.99, 8, 300, 4, 0.4, 5.991). */
int rsc_pnp_set_ransac_parameters(rsc_pnp* s, double probability, int min_inliers, int max_iterations,
                                  int min_set, float epsilon, float th2);
/* PnPsolver::iterate (PnPsolver.cpp:102-191).  `inliers` receives n_points bytes (vbInliers) or
 * is left untouched when the reference returns an empty vector (:105); may be NULL. */
int rsc_pnp_iterate(rsc_pnp* s, int n_iterations, rsc_pnp_result* out, uint8_t* inliers);
/* PnPsolver::find (PnPsolver.cpp:96-100). */
int rsc_pnp_find(rsc_pnp* s, rsc_pnp_result* out, uint8_t* inliers);
/* vbInliers of the last iterate() / find() of this solver (n_points bytes; mvbRefinedInliers or
 * mvbBestInliers scattered through the keypoint indices, PnPsolver.cpp:159-166, :176-186), fetched
 * after the call — e.g. for the candidate a rank contributes to the multi-GPU winner exchange.
 * Returns 1, or 0 with all-zero bytes when that call returned false (vbInliers empty, :105). */
int rsc_pnp_last_inliers(rsc_pnp* s, uint8_t* out);
/* iterate() on `count` solvers of ONE context at once (the relocalization candidates of
 * Tracking.cpp:1239-1334); all hypotheses of all solvers run in the same kernel launches.
 * Results are identical to calling rsc_pnp_iterate on each solver in order. */
int rsc_pnp_iterate_many(rsc_pnp* const* solvers, int count, const int32_t* n_iterations, rsc_pnp_result* out,
                         uint8_t* const* inliers);
/* Back to the freshly constructed state with a new rand() stream (reuse HBM-resident data). */
int rsc_pnp_reset(rsc_pnp* s, uint32_t seed);
/* rsc_pnp_reset / rsc_pnp_set_ransac_parameters over `count` solvers in one call. */
int rsc_pnp_reset_many(rsc_pnp* const* solvers, int count, const uint32_t* seeds);
int rsc_pnp_set_ransac_parameters_many(rsc_pnp* const* solvers, int count, double probability, int min_inliers,
                                       int max_iterations, int min_set, float epsilon, float th2);
/* out: [0] mnIterations [1] mRansacMaxIts [2] mRansacMinInliers [3] mnBestInliers
 *      [4] maximum_number_of_correspondences [5] N [6] N_points [7] mRansacMinSet */
int rsc_pnp_get_state(const rsc_pnp* s, int32_t out[8]);
/* Debug/parity hook: sample indices (8 per hypothesis) of the last launch for this solver. */
int rsc_pnp_last_samples(rsc_pnp* s, int32_t* out, int cap);
/* Parity hook: inlier counts and float poses (R row-major 9 + t 3) of every hypothesis of the last
 * launch for this solver (PnPsolver.cpp:139-146 mnInliersi / mRi, mti per hypothesis).  Valid until
 * the context's next launch.  The counts are always the full counts: when that launch ran with the
 * scan bound on (rsc_context_set_scan_bound), the first call that asks for counts runs the launch's
 * scan once more with the bound off, on the same tables, records and outputs, and waits for it; later
 * calls find the round already recounted.  Lifetime: the context's buffers that launch reads stay valid
 * until the context's next launch of any kind, but it also reads the correspondences of every solver
 * of the round, which go with the solver.  So the recount needs all PnP solvers of the context alive:
 * once one has been destroyed after a round that still awaits its recount, a call that asks for counts
 * launches nothing and returns RSC_ERR_UNSUPPORTED, for every solver of that round, until the context's
 * next launch (rsc_pnp_last_counts_raw still returns what the round left; poses alone, counts == NULL,
 * are still served). */
int rsc_pnp_last_hypotheses(rsc_pnp* s, int32_t* counts, float* poses, int cap);
/* The counts of the last launch for this solver as they stand in the count buffer: before a recount by
 * rsc_pnp_last_hypotheses, what the round itself left (a hypothesis cut short by the scan bound shows
 * its count over the first min(N, 128 PPT) correspondences).  Returns the number written. */
int rsc_pnp_last_counts_raw(rsc_pnp* s, int32_t* counts, int cap);

/* ---- Sim3Solver (include/Sim3Solver.hpp:16-103, src/Sim3Solver.cpp) --------------------------- */
/* Raw constructor inputs for one keyframe pair (Sim3Solver.cpp:6-85), per match slot i1 < n1. */
typedef struct {
    int32_t n1;              /* vpMatched12.size() */
    const uint8_t* valid;    /* slot usable: match, pMP1, not bad, both indices >= 0 (:28-43) */
    const float* Xw1;        /* [n1][3] pMP1->GetWorldPos() */
    const float* Xw2;        /* [n1][3] pMP2->GetWorldPos() */
    const float* sigma2_1;   /* [n1] pKF1->mvLevelSigma2[kp1.octave] */
    const float* sigma2_2;   /* [n1] pKF2->mvLevelSigma2[kp2.octave] */
    float R1[9], t1[3];      /* pKF1->GetRotation()/GetTranslation(), row-major */
    float R2[9], t2[3];
    float K1[4], K2[4];      /* fx, fy, cx, cy of KeyFrame::mK */
} rsc_sim3_input;

/* Sim3Solver::Sim3Solver (Sim3Solver.cpp:6-85, includes its SetRansacParameters() call). */
int rsc_sim3_create(rsc_context* ctx, const rsc_sim3_input* in, uint32_t seed, rsc_sim3** out);
void rsc_sim3_destroy(rsc_sim3* s);
/* Sim3Solver::SetRansacParameters (Sim3Solver.cpp:87-111; defaults 0.99, 6, 300). */
int rsc_sim3_set_ransac_parameters(rsc_sim3* s, double probability, int min_inliers, int max_iterations);
typedef struct {
    int32_t ok, no_more, n_inliers, iterations;
    float R[9], t[3];    /* GetEstimatedRotation()/GetEstimatedTranslation() after the call */
} rsc_sim3_result;
/* Sim3Solver::iterate (Sim3Solver.cpp:113-178); `inliers` receives n1 bytes (always sized). */
int rsc_sim3_iterate(rsc_sim3* s, int n_iterations, rsc_sim3_result* out, uint8_t* inliers);
int rsc_sim3_find(rsc_sim3* s, rsc_sim3_result* out, uint8_t* inliers);
int rsc_sim3_iterate_many(rsc_sim3* const* solvers, int count, const int32_t* n_iterations, rsc_sim3_result* out,
                          uint8_t* const* inliers);
int rsc_sim3_reset(rsc_sim3* s, uint32_t seed);
int rsc_sim3_reset_many(rsc_sim3* const* solvers, int count, const uint32_t* seeds);
int rsc_sim3_set_ransac_parameters_many(rsc_sim3* const* solvers, int count, double probability, int min_inliers,
                                        int max_iterations);
/* out: [0] mnIterations [1] mRansacMaxIts [2] mRansacMinInliers [3] mnBestInliers [4] N [5] mN1 */
int rsc_sim3_get_state(const rsc_sim3* s, int32_t out[6]);
/* Prepared per-correspondence arrays built by the constructor (for parity tests):
 * X1c/X2c [N][3], P1im1/P2im2 [N][2], max_err1/2 [N] (size_t thresholds), indices1 [N]. */
/* Parity hook: inlier counts and float (R12 9 + t12 3) of every hypothesis of the last launch
 * (Sim3Solver.cpp:150-153 mnInliersi / mR12i, mt12i). */
int rsc_sim3_last_hypotheses(rsc_sim3* s, int32_t* counts, float* poses, int cap);
int rsc_sim3_prepared(const rsc_sim3* s, float* X1c, float* X2c, float* P1im1, float* P2im2, uint64_t* max_err1,
                      uint64_t* max_err2, int32_t* indices1);

/* ---- MLPnPsolver (include/MLPnPsolver.hpp:10-199, src/MLPnPsolver.cpp) ----------------------------
 * Dormant in the reference (not compiled, call sites commented out, Tracking.cpp:1222,1227-1228);
 * exported for BASELINE config 4.  Same problem struct and result record as PnP.  Parity of this
 * solver against the reference is unpinned. */
/* MLPnPsolver::MLPnPsolver (MLPnPsolver.cpp:5-53, includes its SetRansacParameters() call). */
int rsc_mlpnp_create(rsc_context* ctx, const rsc_pnp_problem* problem, uint32_t seed, rsc_mlpnp** out);
void rsc_mlpnp_destroy(rsc_mlpnp* s);
/* computePose's covMats (MLPnPsolver.cpp:321, :375-388, :483-484, :694-695): cov = [n][9] row-major
 * 3x3 bearing-vector covariance per correspondence (the problem's compacted order), or NULL for the
 * reference's own configuration (it passes a single-element covMats, so use_cov is false).  With
 * covariances the hypotheses solve A^T P A and the Gauss-Newton runs on J^T Kll J, P = Kll the
 * block-diagonal (N^T Sigma N)^-1.  Not reachable from the reference's callers: parity unpinned
 * (SURVEY.md Q15); checked against the oracle's restatement. */
int rsc_mlpnp_set_covariances(rsc_mlpnp* s, const double* cov);
/* MLPnPsolver::SetRansacParameters (MLPnPsolver.cpp:185-220; defaults 0.99, 8, 300, 6, 0.4, 5.991).
 * min_set must be in [6, 8] (computePose asserts n > 5, :324) -> RSC_ERR_UNSUPPORTED otherwise. */
int rsc_mlpnp_set_ransac_parameters(rsc_mlpnp* s, double probability, int min_inliers, int max_iterations,
                                    int min_set, float epsilon, float th2);
int rsc_mlpnp_set_ransac_parameters_many(rsc_mlpnp* const* solvers, int count, double probability, int min_inliers,
                                         int max_iterations, int min_set, float epsilon, float th2);
/* MLPnPsolver::iterate (MLPnPsolver.cpp:56-183): T is identity unless ok (Tout.setIdentity(), :57). */
int rsc_mlpnp_iterate(rsc_mlpnp* s, int n_iterations, rsc_pnp_result* out, uint8_t* inliers);
int rsc_mlpnp_iterate_many(rsc_mlpnp* const* solvers, int count, const int32_t* n_iterations, rsc_pnp_result* out,
                           uint8_t* const* inliers);
int rsc_mlpnp_reset(rsc_mlpnp* s, uint32_t seed);
int rsc_mlpnp_reset_many(rsc_mlpnp* const* solvers, int count, const uint32_t* seeds);
/* out: [0] mnIterations [1] mRansacMaxIts [2] mRansacMinInliers [3] mnBestInliers [4] N [5] mRansacMinSet */
int rsc_mlpnp_get_state(const rsc_mlpnp* s, int32_t out[6]);
/* Parity hooks: double poses (R 9 + t 3) and sample indices (8 per hypothesis) of the last launch. */
int rsc_mlpnp_last_poses(rsc_mlpnp* s, double* out, int cap);
int rsc_mlpnp_last_samples(rsc_mlpnp* s, int32_t* out, int cap);
int rsc_mlpnp_last_counts(rsc_mlpnp* s, int32_t* counts, int cap);

/* ---- The reference's shared rand() stream (Q3) ---------------------------------------------------
 * DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp:47-50) draws from glibc's process-
 * global rand(), which the reference never seeds (= srand(1)); every candidate's iterate() of a
 * relocalization (Tracking.cpp:1239-1262) or loop closure (LoopClosing.cpp:271-286) continues that one
 * stream where the previous call stopped.  An rsc_stream is that stream: srand(seed) and a position. */
int rsc_stream_create(rsc_context* ctx, uint32_t seed, rsc_stream** out);
void rsc_stream_destroy(rsc_stream* s);
/* Consume n draws (rand() calls made elsewhere in the process between two solver calls). */
int rsc_stream_skip(rsc_stream* s, int64_t n);
/* Draws consumed since srand(seed). */
int rsc_stream_position(const rsc_stream* s, int64_t* out);
/* The next n rand() outputs, without consuming them (parity hook; computed on the device). */
int rsc_stream_peek(rsc_stream* s, int n, int32_t* out);
/* Bind a solver to a shared stream (NULL: back to its own stream, which resumes where it stopped).
 * Every later iterate()/find() of a bound solver draws its samples from the stream's current position
 * and advances it by the draws it made (mRansacMinSet per PnP / MLPnP hypothesis, 3 per Sim3
 * hypothesis), exactly as the reference's call does.  *_iterate_many over bound solvers runs the
 * calls one after the other in list order (the reference's call order). */
int rsc_pnp_bind_stream(rsc_pnp* s, rsc_stream* stream);
int rsc_sim3_bind_stream(rsc_sim3* s, rsc_stream* stream);
int rsc_mlpnp_bind_stream(rsc_mlpnp* s, rsc_stream* stream);

/* ---- Event drivers (BASELINE config 5) -----------------------------------------------------------
 * One relocalization or loop-closure event = the candidate solvers one Tracking::Relocalization() /
 * LoopClosing::ComputeSim3() call builds (Tracking.cpp:1207-1232, LoopClosing.cpp:238-265), stored
 * contiguously: event e owns solvers[event_begin[e] .. event_begin[e+1]).  Every candidate of every
 * event runs in the same launches. */
typedef struct {
    int32_t winner;      /* first candidate (in the reference's round-robin order) whose iterate()
                            returns a pose, -1 if none: the pose the reference hands to
                            PoseOptimization / SearchBySim3 first */
    int32_t round;       /* round of iterate(5) calls in which it returns */
    int32_t hypothesis;  /* index of the returning hypothesis in that candidate's stream */
    int32_t n_inliers;
} rsc_event_result;
/* Relocalization (Tracking.cpp:1239-1262): rounds of iterate(5) over the non-discarded candidates
 * (bNoMore discards) until a candidate returns a pose; per_candidate receives each candidate's last
 * iterate() result (candidates after the winner in the winning round are iterated as well — the
 * reference reaches them only if the downstream check rejects the winner, with identical results). */
int rsc_reloc_events(rsc_pnp* const* solvers, const int32_t* event_begin, int n_events, rsc_pnp_result* per_candidate,
                     rsc_event_result* per_event);
/* Loop closure (LoopClosing.cpp:271-286): each candidate's stream is run to its first success or
 * to mRansacMaxIts in one call; the winner is the lexicographically smallest (round, candidate) with
 * round = hypothesis / 5 — identical to the reference's round-robin of iterate(5) calls. */
int rsc_loop_events(rsc_sim3* const* solvers, const int32_t* event_begin, int n_events,
                    rsc_sim3_result* per_candidate, rsc_event_result* per_event);
/* The same events on the reference's shared rand() stream: event e's calls draw from streams[e]
 * (one distinct stream per event; its position at the Relocalization / ComputeSim3 call) in the
 * round-robin's call order — round by round, candidate by candidate, iterate(5) each — and advance it.
 * All events' rounds still run in the same launches: each call is positioned assuming every earlier
 * call of its round ran its whole loop, which holds up to the first success (the only early return),
 * and that success ends the event.  Candidates after the winner in the winning round are calls the
 * reference never makes: their per_candidate records are left as they were and their solver state
 * is unspecified.  Solvers must not be bound to a stream (RSC_ERR_ARG). */
int rsc_reloc_events_shared(rsc_pnp* const* solvers, const int32_t* event_begin, int n_events,
                            rsc_stream* const* streams, rsc_pnp_result* per_candidate, rsc_event_result* per_event);
int rsc_loop_events_shared(rsc_sim3* const* solvers, const int32_t* event_begin, int n_events,
                           rsc_stream* const* streams, rsc_sim3_result* per_candidate, rsc_event_result* per_event);

/* ---- Gated events (round 6): the reference's post-RANSAC acceptance test inside the event loop ----
 * The drivers above end an event at the first candidate whose iterate() returns a pose.  The
 * reference then checks that pose with the next stages and, on rejection, continues the round-robin
 * (the next candidate of the same round, then later rounds, the rejected candidate included).  The
 * gated drivers run those stages on the device (PoseOptimization / SearchBySim3 + OptimizeSim3, the
 * kernels of rsc_pose_optimization_many / rsc_search_by_sim3_many / rsc_optimize_sim3_many) for every
 * success in the reference's order, batched across events, until a success passes.  Solvers draw
 * from their own streams (bound solvers: RSC_ERR_UNSUPPORTED).  per_candidate: each candidate's last
 * iterate() record. */
#define RSC_GATE_NONE 0    /* every candidate discarded without an accepted pose (bMatch false) */
#define RSC_GATE_MATCH 1   /* a success passed the gate (bMatch = true) */
#define RSC_GATE_HANDOFF 2 /* rsc_reloc_events_gated only: 10 <= nGood < 50 after PoseOptimization, where the
                              reference runs its SearchByProjection refinement (Tracking.cpp:1294-1323).  This
                              driver stops the event there; rsc_reloc_events_refined (below) runs that chain on
                              the device and carries the round-robin on, so it never returns this status */
/* Tracking::Relocalization (Tracking.cpp:1239-1335).  The current Frame's data PoseOptimization reads
 * beyond what the solvers hold (their compacted p2d / p3dw / sigma2 are Frame::mvKeysUn, the MapPoint
 * positions and mvLevelSigma2; mvInvLevelSigma2 = 1.0f / mvLevelSigma2 as ORBextractor sets it). */
typedef struct {
    const float* u_right;  /* [n_points] Frame::mvuRight (>= 0: stereo edge), NULL for a monocular Frame */
    float bf;              /* Frame::mbf */
} rsc_reloc_frame;
typedef struct {
    int32_t status;       /* RSC_GATE_* */
    int32_t winner;       /* candidate of the accepted (MATCH) or handed-off success, -1 for NONE */
    int32_t round;        /* its round of iterate(5) calls */
    int32_t hypothesis;   /* index of the returning hypothesis in that candidate's stream */
    int32_t n_inliers;    /* RANSAC nInliers of that success */
    int32_t n_good;       /* PoseOptimization's return value on it (Tracking.cpp:1284) */
    int32_t rejected;     /* successes rejected before it (nGood < 10, Tracking.cpp:1286-1287) */
    int32_t gates;        /* PoseOptimization runs of the event */
    float Tcw[16];        /* row-major pose after PoseOptimization (mCurrentFrame.mTcw) */
} rsc_reloc_gate_result;
/* frames[e]: event e's current Frame (its solvers' n_points = Frame::N).  outlier[e] (may be NULL, or
 * NULL entries): [n_points] mvbOutlier of the winner's PoseOptimization for the slots with a map point
 * (others 0); inliers[e] (may be NULL / NULL entries): [n_points] the winner's vbInliers. */
int rsc_reloc_events_gated(rsc_pnp* const* solvers, const int32_t* event_begin, int n_events,
                           const rsc_reloc_frame* frames, rsc_pnp_result* per_candidate,
                           rsc_reloc_gate_result* per_event, uint8_t* const* outlier, uint8_t* const* inliers);

/* LoopClosing::ComputeSim3 (LoopClosing.cpp:268-329).  A candidate's Sim3 solver was built from
 * (kf1 = mpCurrentKF, kf2 = the candidate KeyFrame, vvpMapPointMatches[i]); the gate needs those
 * views and matches: SearchBySim3(kf1, kf2, vpMapPointMatches = the RANSAC inliers of matches12, R,
 * t, 7.5) then OptimizeSim3(kf1, kf2, vpMapPointMatches, gScm = Sim3(R, t, 1), 10) with
 * mvInvLevelSigma2 = 1 / (scale_factors[l]^2) (float, as ORBextractor); accepted when nInliers >= 20. */
struct rsc_kfview;
typedef struct {
    struct rsc_kfview* kf1;    /* mpCurrentKF's view (rsc_kfview_create) */
    struct rsc_kfview* kf2;    /* the candidate KeyFrame's view */
    const int32_t* matches12;  /* [kf1 n] vvpMapPointMatches[i]: KF2 keypoint index of the matched
                                  MapPoint, -1 NULL, -2 a MapPoint not in KF2 (the solver's input) */
} rsc_loop_candidate;
typedef struct {
    int32_t status;         /* RSC_GATE_NONE or RSC_GATE_MATCH */
    int32_t winner, round, hypothesis, n_inliers;  /* the accepted success (as rsc_event_result) */
    int32_t n_found;        /* SearchBySim3's return value on it */
    int32_t n_opt_inliers;  /* OptimizeSim3's return value (>= 20 on MATCH) */
    int32_t rejected;       /* successes rejected before it (nInliers < 20) */
    double S[8];            /* gScm after OptimizeSim3: q (x, y, z, w), t, s */
} rsc_loop_gate_result;
/* matches_out[e] (may be NULL / NULL entries): [kf1 n] mvpCurrentMatchedPoints of the accepted
 * candidate as KF2 keypoint indices (-1 NULL, -2 a MapPoint not in KF2). */
int rsc_loop_events_gated(rsc_sim3* const* solvers, const rsc_loop_candidate* candidates,
                          const int32_t* event_begin, int n_events, rsc_sim3_result* per_candidate,
                          rsc_loop_gate_result* per_event, int32_t* const* matches_out);

/* ---- Optimizer::PoseOptimization (src/Optimizer.cpp:205-424) ------------------------------------
 * The pose-only g2o optimisation every tracking step and Tracking::Relocalization()
 * (Tracking.cpp:1284,1300,1315) run on the RANSAC pose: Levenberg-Marquardt of one VertexSE3Expmap
 * over EdgeSE3ProjectXYZOnlyPose (mvuRight < 0) and EdgeStereoSE3ProjectXYZOnlyPose (mvuRight >= 0,
 * Optimizer.cpp:252-323) edges with Huber kernels (delta sqrt(5.991) / sqrt(7.815)), 4 rounds of 10
 * iterations, each restarted from the entry pose, with chi2 > 5.991 / 7.815 outlier re-classification.
 * Parity against the reference is unpinned (g2o/Eigen cannot be built here). */
typedef struct {
    int32_t n;                /* pFrame->N keypoint slots */
    const uint8_t* has_mp;    /* [n] mvpMapPoints[i] != NULL (an edge is built); NULL = every slot */
    const float* uv;          /* [n][2] mvKeysUn[i].pt */
    const float* Xw;          /* [n][3] MapPoint::GetWorldPos() */
    const float* inv_sigma2;  /* [n] mvInvLevelSigma2[kpUn.octave] (information = I * invSigma2) */
    const float* u_right;     /* [n] mvuRight (>= 0: stereo observation), or NULL for a monocular Frame */
    float fx, fy, cx, cy;     /* Frame::fx,fy,cx,cy */
    float Tcw[16];            /* row-major pFrame->mTcw on entry */
    float bf;                 /* Frame::mbf (stereo baseline * fx; unused without stereo slots) */
} rsc_poseopt_problem;

typedef struct {
    int32_t n_good;        /* return value: nInitialCorrespondences - nBad (0 if < 3 edges) */
    int32_t n_initial;     /* nInitialCorrespondences */
    int32_t rounds;        /* outer rounds run (breaks after one when fewer than 10 edges) */
    int32_t lm_iterations; /* OptimizationAlgorithmLevenberg::solve calls */
    int32_t lm_trials;     /* linear solves (Levenberg trials) */
    float Tcw[16];         /* row-major pose after the call (pFrame->SetPose, Optimizer.cpp:420-421);
                              the entry pose when fewer than 3 edges (the reference returns early) */
} rsc_poseopt_result;

/* Optimizer::PoseOptimization on `count` Frames in one launch (one workgroup per Frame).
 * outlier[c] receives mvbOutlier for the slots with a map point (others untouched); may be NULL.
 *
 * Limits and degenerate inputs.  A Frame may have any number of slots but at most 8192 edges (slots
 * with a map point): more returns RSC_ERR_UNSUPPORTED before anything runs, and the context stays
 * usable.  The values are taken as given and treated as the reference's g2o code treats them; nothing
 * is validated or clamped.  A NaN or infinite Xw, uv or Tcw entry, or a point with z == 0 in the camera
 * frame, makes activeRobustChi2 non-finite: rho is NaN, no trial is accepted, every round runs its 10
 * iterations of one trial, the pose returned is the (normalised) entry pose — NaN where Tcw was NaN —
 * and such an edge is never an outlier (NaN > 5.991 is false).  inv_sigma2 == 0, or fx == fy == 0 on a
 * monocular Frame, gives H == 0 and rho == 0: every optimize() call ends after one trial.  A negative inv_sigma2 (ORB-SLAM2
 * never produces one) makes the LDLT of H + lambda I non-positive: the previous update _x is applied
 * again and tempChi becomes DBL_MAX, as LinearSolverDense and solve() do.  No input makes the call
 * loop: every loop of the kernel is bounded by the edge count and the 4 x 10 x 10 LM schedule.
 * tests/test_gpu_lm_edges.py holds these cases against the oracle. */
int rsc_pose_optimization_many(rsc_context* ctx, const rsc_poseopt_problem* problems, int count,
                               rsc_poseopt_result* out, uint8_t* const* outlier);

/* ---- Optimizer::OptimizeSim3 (src/Optimizer.cpp:1054-1250) ----------------------------------------
 * The loop-closure refinement LoopClosing::ComputeSim3 runs on every candidate whose Sim3 RANSAC
 * succeeded, right after SearchBySim3 (LoopClosing.cpp:309-311): g2o Levenberg-Marquardt of one
 * VertexSim3Expmap (_fix_scale) over EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ pairs (numeric
 * Jacobians) with Huber kernels (delta = sqrt(th2)), optimize(5), outlier removal (chi2 > th2),
 * optimize(5 or 10).  Parity against the reference is unpinned (g2o/Eigen cannot be built here). */
typedef struct {
    int32_t n;               /* vpMatches1.size() = pKF1->N (KeyFrame 1 keypoint slots) */
    const uint8_t* valid;    /* [n] slot i is a correspondence: vpMatches1[i] and vpMapPoints1[i] set, neither
                                isBad(), vpMatches1[i]->GetIndexInKeyFrame(pKF2) >= 0 (Optimizer.cpp:1112-1143) */
    const float* X1w;        /* [n][3] vpMapPoints1[i]->GetWorldPos() */
    const float* X2w;        /* [n][3] vpMatches1[i]->GetWorldPos() */
    const float* uv1;        /* [n][2] pKF1->mvKeysUn[i].pt */
    const float* uv2;        /* [n][2] pKF2->mvKeysUn[i2].pt, i2 = GetIndexInKeyFrame(pKF2) */
    const float* inv1;       /* [n] pKF1->mvInvLevelSigma2[octave of i] */
    const float* inv2;       /* [n] pKF2->mvInvLevelSigma2[octave of i2] */
    float R1w[9], t1w[3];    /* pKF1->GetRotation(), GetTranslation() (row-major) */
    float R2w[9], t2w[3];    /* pKF2 */
    float K1[4], K2[4];      /* mK: fx, fy, cx, cy */
    double S[8];             /* g2oS12 on entry: quaternion (x, y, z, w), t, s */
    float th2;               /* 10 in LoopClosing.cpp:311 */
} rsc_sim3opt_problem;

typedef struct {
    int32_t n_inliers;          /* return value nIn (0 when nCorrespondences - nBad < 10) */
    int32_t n_correspondences;
    int32_t n_bad;              /* correspondences removed after the first optimize(5) */
    int32_t lm_iterations;      /* OptimizationAlgorithmLevenberg::solve calls */
    int32_t lm_trials;
    double S[8];                /* g2oS12 after the call (the entry value when n_inliers == 0) */
} rsc_sim3opt_result;

/* OptimizeSim3 on `count` KeyFrame pairs in one launch (one workgroup per pair).  keep[c] (may be
 * NULL) receives per slot 0 where vpMatches1[i] is set to NULL (an outlier), 1 elsewhere.
 *
 * Limits and degenerate inputs.  A pair may have any number of slots but at most 8192 valid
 * correspondences: more returns RSC_ERR_UNSUPPORTED before anything runs, and the context stays
 * usable; a pair without a valid correspondence returns 0 with S untouched.  The values are taken as
 * given, as the reference's g2o code treats them.  A NaN or infinite point, observation or S entry, or
 * s == 0, makes activeRobustChi2 non-finite: rho is NaN, no trial is accepted, both optimize() calls
 * run all their iterations with one trial each, S is returned as it came and no correspondence is
 * removed (NaN > th2 is false).  inv1 == inv2 == 0 gives H == 0 and rho == 0: one trial per optimize().
 * Negative inv1 / inv2 (ORB-SLAM2 never produces them) make the LDLT non-positive: the previous update
 * is applied again and tempChi becomes DBL_MAX.  Every loop and every hand-off wait of the kernel (both
 * forms) is bounded independently of the data.  tests/test_gpu_lm_edges.py holds these cases against
 * the oracle. */
int rsc_optimize_sim3_many(rsc_context* ctx, const rsc_sim3opt_problem* problems, int count,
                           rsc_sim3opt_result* out, uint8_t* const* keep);

/* ---- Optimizer::LocalBundleAdjustment (src/Optimizer.cpp:426-787) ----------------------------------
 * The local mapping thread's bundle adjustment, called after SearchInNeighbors (LocalMapping.cpp): g2o
 * Levenberg-Marquardt over the local KeyFrames (VertexSE3Expmap; the fixed cameras and KeyFrame 0 fixed) and the
 * local MapPoints (VertexSBAPointXYZ, marginalised) with EdgeSE3ProjectXYZ (u_right < 0) and
 * EdgeStereoSE3ProjectXYZ edges, BlockSolver_6_3's Schur complement, Huber kernels (delta sqrt(5.991) /
 * sqrt(7.815) as float): optimize(5), classification (chi2 > 5.991 / 7.815 or depth <= 0 -> level 1, kernels
 * removed), initializeOptimization(0), optimize(10), final classification into vToErase, recovery.
 * The caller builds lLocalKeyFrames / lFixedCameras / lLocalMapPoints (:430-483) and passes plain arrays.
 * The reduced pose system is solved by an LDL^T without pivoting in Hessian-index order over the dense
 * matrix (DESIGN.md §2.17 states the arithmetic); the reference's LinearSolverEigen orders it by AMD first, so
 * the two differ at rounding level, and parity with a g2o / Eigen build is unpinned. */
#define RSC_LOCALBA_MAX_FREE_KFS 64   /* a 384 x 384 reduced system */
#define RSC_LOCALBA_MAX_KFS 4160      /* free and fixed together */
#define RSC_LOCALBA_MAX_POINTS 16384
#define RSC_LOCALBA_MAX_EDGES 131072
typedef struct {
    int32_t n_kfs;             /* lLocalKeyFrames and lFixedCameras, in any order */
    const int64_t* kf_id;      /* [n_kfs] mnId, unique; the Hessian index of a free KeyFrame is its rank by kf_id */
    const uint8_t* fixed;      /* [n_kfs] mnId == 0 or one of lFixedCameras */
    const float* Tcw;          /* [n_kfs][16] row-major GetPose() */
    const float* cam;          /* [n_kfs][5] fx, fy, cx, cy, mbf */
    int32_t n_points;          /* lLocalMapPoints, in list order */
    const int64_t* mp_id;      /* [n_points] mnId, unique; the landmark index is the rank by mp_id */
    const float* pos;          /* [n_points][3] GetWorldPos() */
    const uint8_t* bad;        /* [n_points] isBad() as the classification loops read it (:670,688,717,733) */
    const int32_t* obs_begin;  /* [n_points + 1] CSR over the points, obs_begin[0] == 0: the edges in the caller's
                                  iteration order of GetObservations(), bad KeyFrames left out (:574) */
    const int32_t* obs_kf;     /* [n_edges] index into the KeyFrames; a point names a KeyFrame at most once */
    const float* uv;           /* [n_edges][2] mvKeysUn[idx].pt */
    const float* u_right;      /* [n_edges] mvuRight[idx]; < 0: a monocular edge */
    const float* inv_sigma2;   /* [n_edges] mvInvLevelSigma2[octave] */
} rsc_localba_problem;

typedef struct {               /* any member may be NULL */
    float* Tcw;                /* [n_kfs][16] Converter::toIso(estimate) as float; fixed KeyFrames: the input bytes */
    float* pos;                /* [n_points][3] estimate.cast<float>() */
    uint8_t* edge_flags;       /* [n_edges] bit 0: level 1 after the first optimize(); bit 1: in vToErase */
    int32_t* erase;            /* [n_edges] the first n_erase entries: vToErase as edge indices, mono edges first,
                                  then stereo, each in edge order */
} rsc_localba_out;

typedef struct {
    int32_t n_vertices, n_points, n_edges; /* active vertices (fixed KeyFrames included), points among them, edges */
    int32_t lm_iterations, lm_trials;
    double chi2_first, chi2_last;          /* activeRobustChi2 at the first solve() and of the estimates left */
} rsc_localba_phase;

#define RSC_LOCALBA_NO_EDGE_1 1  /* status bits: the first optimize() had no active edge (no edge at all) */
#define RSC_LOCALBA_NO_EDGE_2 2  /* every edge was level 1: initializeOptimization(0) fails, optimize(10) returns */
#define RSC_LOCALBA_NO_FREE_KF 4 /* no free KeyFrame among the active vertices of the first optimize() */
typedef struct {
    int32_t n_erase, n_level1, status;
    rsc_localba_phase phase[2];
    int32_t branches[12];      /* LM branch counters over both phases: iterations, trials, zero pivot, tempChi
                                  non-finite, rho NaN, rejected, qmax == 10, rho == 0, nBad >= 3, phase without
                                  an active edge, vertices dropped from the active set, level-1 edges not erased */
} rsc_localba_result;

/* LocalBundleAdjustment on `count` problems, one after another; out (may be NULL) and result (may be NULL) are
 * arrays of `count`.  Each stage of a Levenberg trial is a launch spread over the device; the host reads one
 * small record per trial.  With timing on, rsc_context_last_kernel_timing's [2] is the device time of the call.
 *
 * Quirks reproduced: a level-1 edge's chi2() is never recomputed in the second optimize(), so the final loop reads
 * its first-phase value while isDepthPositive() reads the final estimates (an edge set aside for depth alone can
 * leave vToErase); the edges of a `bad` point are skipped by both classification loops and keep level 0 and
 * their kernel; a vertex without a level-0 edge leaves the active set and the indices are rebuilt; the edges'
 * _error after optimize() is that of the last trial, accepted or not.  The stop flag is not an input: the caller
 * reads *pbStopFlag before the call.
 *
 * Limits (checked before any launch; outputs untouched, the context stays usable): RSC_ERR_ARG for a NULL array,
 * a kf_id or mp_id that is not unique, obs_begin not ascending from 0, obs_kf out of range, or a point naming a
 * KeyFrame twice; RSC_ERR_UNSUPPORTED above RSC_LOCALBA_MAX_FREE_KFS free KeyFrames, RSC_LOCALBA_MAX_KFS
 * KeyFrames, RSC_LOCALBA_MAX_POINTS points or RSC_LOCALBA_MAX_EDGES edges.  count == 0 is RSC_OK.
 *
 * Degenerate problems.  No edge: initializeOptimization() fails and both optimize() calls return at once; free
 * KeyFrames come back as the quaternion round trip of their entry pose, points as given.  No free KeyFrame
 * with edges: the points alone are optimised (an empty reduced system solves trivially).  Every edge level 1
 * after the first phase: the second optimize() returns at once and the final loop reads the first phase's
 * chi2.  A vertex that was never active is recovered all the same (pose: quaternion round trip).  The update
 * vector starts at zero in each optimize() (the reference allocates it without clearing it; it matters only when
 * the first reduced solve of a phase meets a zero pivot).  NaN / Inf / z == 0 inputs are taken as given: a
 * non-finite chi2 makes rho NaN, no trial is accepted and every iteration runs one trial.  No input makes the
 * call loop: every loop is bounded by the counts and the (5 + 10) iterations x 10 trials schedule. */
int rsc_local_bundle_adjustment_many(rsc_context* ctx, const rsc_localba_problem* problems, int count,
                                     const rsc_localba_out* out, rsc_localba_result* result);

/* ---- ORBmatcher::SearchByBoW (src/ORBmatcher.cpp:110-240, :354-488) -----------------------------
 * The producer of every RANSAC correspondence set: Hamming-256 matching of ORB descriptors that
 * share a DBoW2 FeatureVector node, with the nearest-neighbour ratio test and the rotation-histogram
 * consistency check.  Views (KeyFrames, the current Frame) are uploaded once and stay resident in
 * HBM; searches name them by handle.  Integer work: results are bit-exact with the reference. */
typedef struct {
    int32_t n;                 /* keypoints (KeyFrame::N / Frame::N), <= 8192 */
    const uint8_t* desc;       /* [n][32] mDescriptors rows (CV_8U, 32 columns) */
    const float* angle;        /* [n] keypoint angle: mvKeysUn[i].angle for a KeyFrame, mvKeys[i].angle for
                                  the Frame (the angles the two overloads read, ORBmatcher.cpp:185,435) */
    const uint8_t* valid;      /* [n] GetMapPointMatches()[i] != NULL && !isBad(); NULL = all.
                                  Unused for the Frame side of the Frame overload. */
    int32_t n_nodes;           /* mFeatVec.size() */
    const uint32_t* node_id;   /* [n_nodes] mFeatVec keys, strictly ascending (std::map order) */
    const int32_t* node_begin; /* [n_nodes + 1] CSR offsets into feat */
    const uint32_t* feat;      /* [node_begin[n_nodes]] each node's vector<unsigned int>, in order; every
                                  feature index < n and at most once overall (DBoW2 transform) */
} rsc_bow_features;

typedef struct rsc_bow rsc_bow;

/* Upload a view's descriptors, angles, map-point validity and FeatureVector (KeyFrame::mFeatVec /
 * Frame::mFeatVec after ComputeBoW) to HBM. */
int rsc_bow_create(rsc_context* ctx, const rsc_bow_features* features, rsc_bow** out);
void rsc_bow_destroy(rsc_bow* view);
/* Refresh the map-point validity of a resident view (map points culled or replaced since upload). */
int rsc_bow_set_valid(rsc_bow* view, const uint8_t* valid);

/* SearchByBoW(pKF = kfs[c], F = frame, vpMapPointMatches) for c < count in one launch (the
 * relocalization candidate loop, Tracking.cpp:1207-1232).  matches[c][i] (i < frame->n) = the
 * KeyFrame feature whose map point matched Frame feature i (vpMapPointMatches[i] =
 * kf.GetMapPointMatches()[matches[c][i]]), or -1; nmatches[c] = the return value. */
int rsc_search_by_bow_frame_many(rsc_context* ctx, rsc_bow* const* kfs, int count, const rsc_bow* frame,
                                 float nnratio, int check_orientation, int32_t* const* matches, int32_t* nmatches);
/* SearchByBoW(pKF1 = kf1, pKF2 = kf2s[c], vpMatches12) for c < count in one launch (the loop
 * candidate loop, LoopClosing.cpp:238-265).  matches12[c][i] (i < kf1->n) = the KF2 feature whose
 * map point vpMatches12[i] is, or -1; nmatches[c] = the return value. */
int rsc_search_by_bow_kf_many(rsc_context* ctx, const rsc_bow* kf1, rsc_bow* const* kf2s, int count,
                              float nnratio, int check_orientation, int32_t* const* matches12, int32_t* nmatches);

/* ---- ORBmatcher::SearchBySim3 (src/ORBmatcher.cpp:948-1170) ---------------------------------
 * The loop-closure matcher run after a Sim3 RANSAC success (LoopClosing.cpp:296-309): unmatched
 * MapPoints of each KeyFrame are projected into the other with (R12, t12), matched to the best
 * descriptor among the keypoints of the predicted pyramid levels inside th * scale of the projection
 * (KeyFrame::GetFeaturesInArea), and kept when both directions agree. */
typedef struct {
    int32_t n;                  /* KeyFrame::N */
    const float* kp;            /* [n][2] mvKeysUn[i].pt */
    const int32_t* octave;      /* [n] mvKeysUn[i].octave */
    const uint8_t* desc;        /* [n][32] mDescriptors */
    const int32_t* cell_begin;  /* [64*48 + 1] CSR over mGrid[ix][iy] (cell = ix * 48 + iy) */
    const int32_t* cell_feat;   /* mGrid contents, each cell's vector<size_t> in order */
    float min_x, max_x, min_y, max_y;  /* mnMinX, mnMaxX, mnMinY, mnMaxY */
    float grid_w_inv, grid_h_inv;      /* mfGridElementWidthInv, mfGridElementHeightInv */
    float fx, fy, cx, cy;
    const float* scale_factors; /* [n_levels] mvScaleFactors */
    int32_t n_levels;           /* mnScaleLevels */
    float log_scale_factor;     /* mfLogScaleFactor */
    float Rcw[9], tcw[3];       /* GetRotation(), GetTranslation(), row-major */
    const uint8_t* mp_state;    /* [n] GetMapPointMatches()[i]: 0 = NULL, 1 = good, 2 = isBad() */
    const float* mp_pos;        /* [n][3] GetWorldPos() */
    const float* mp_dmax;       /* [n] mfMaxDistance */
    const float* mp_dmin;       /* [n] mfMinDistance */
    const uint8_t* mp_desc;     /* [n][32] MapPoint::GetDescriptor() */
} rsc_sim3_kf;

typedef struct rsc_kfview rsc_kfview;
/* Upload a KeyFrame's SearchBySim3 inputs (keypoints, grid, descriptors, pose, MapPoints) to HBM.
 * RSC_ERR_ARG when a slot with mp_state == 1 has a non-finite mp_dmax or mp_dmin: PredictScale's
 * (int)ceil(log(mfMaxDistance / dist) / mfLogScaleFactor) would leave int's range, which is undefined
 * in the reference (one platform yields INT_MIN, another saturates), so it is refused, not mirrored. */
int rsc_kfview_create(rsc_context* ctx, const rsc_sim3_kf* kf, rsc_kfview** out);
void rsc_kfview_destroy(rsc_kfview* view);

/* SearchBySim3(pKF1 = kf1[c], pKF2 = kf2[c], vpMatches12, R12[c], t12[c], th) for c < count in one
 * launch over resident views.  matched12[c][i1] (in, kf1[c] n entries): the KF2 keypoint index of
 * the MapPoint already in vpMatches12[i1] (GetIndexInKeyFrame(pKF2)), -1 for NULL, -2 for a
 * MapPoint not in KF2.  out12[c][i1]: the KF2 keypoint index of each new match
 * (vpMatches12[i1] = vpMapPoints2[idx2]), else -1; nfound[c] = the return value.
 * R12 [count][9] row-major, t12 [count][3].
 * RSC_ERR_ARG, before any launch, when th is not finite or when, for either KeyFrame of a pair,
 * th * scale_factors[n_levels - 1] * max(grid_w_inv, grid_h_inv) >= 2^30: GetFeaturesInArea's
 * (int)ceil((u - mnMinX + r) * mfGridElementWidthInv) must stay inside int (the u term is below 64
 * cells); outside it the reference's conversion is undefined and is refused, not mirrored. */
int rsc_search_by_sim3_many(rsc_context* ctx, rsc_kfview* const* kf1, rsc_kfview* const* kf2, int count,
                            const float* R12, const float* t12, float th, const int32_t* const* matched12,
                            int32_t* const* out12, int32_t* nfound);
/* Diagnostic: the two directions of pair `pair` of the most recent rsc_search_by_sim3_many on the
 * context, before the agreement step: m1[n1] = vnMatch1 (the KF2 keypoint of each KF1 slot or -1),
 * m2[n2] = vnMatch2.  n1 / n2 must equal that pair's kf1 / kf2 n.  RSC_ERR_ARG when the context's last
 * call did not succeed (or there was none), or the index or sizes do not fit. */
int rsc_diag_sim3match_directions(rsc_context* ctx, int pair, int32_t* m1, int n1, int32_t* m2, int n2);

/* ---- ORBmatcher::SearchByProjection(Frame&, KeyFrame, sAlreadyFound, th, ORBdist) ------------------
 * (src/ORBmatcher.cpp:1317-1444 with Frame::GetFeaturesInArea, src/Frame.cpp:394-447): the matcher of
 * Tracking::Relocalization's refinement (Tracking.cpp:1296, :1310).  Every MapPoint of the candidate
 * KeyFrame that is not in sAlreadyFound is projected with the Frame's pose and takes the free Frame
 * feature of the predicted levels [L-1, L+1] with the smallest descriptor distance (<= ORBdist) inside
 * th * scale[L] of the projection; features claimed by earlier MapPoints of the same call are not
 * free (the reference's sequential order is reproduced exactly), then the rotation histogram removes
 * the matches outside its three best bins.  Quirks kept: no z > 0 test, inclusive image bounds.
 * Precondition: no eligible MapPoint has camera-frame z == 0 (undefined in the reference). */
typedef struct {
    int32_t n;                  /* Frame::N, <= 8192 */
    const float* kp;            /* [n][2] mvKeysUn[i].pt */
    const int32_t* octave;      /* [n] mvKeysUn[i].octave */
    const float* angle;         /* [n] mvKeysUn[i].angle */
    const uint8_t* desc;        /* [n][32] mDescriptors */
    const int32_t* cell_begin;  /* [64*48 + 1] CSR over mGrid[ix][iy] (cell = ix * 48 + iy) */
    const int32_t* cell_feat;   /* mGrid contents, each cell's vector<size_t> in order */
    float min_x, max_x, min_y, max_y;  /* mnMinX, mnMaxX, mnMinY, mnMaxY */
    float grid_w_inv, grid_h_inv;      /* mfGridElementWidthInv, mfGridElementHeightInv */
    float fx, fy, cx, cy;
    const float* scale_factors; /* [n_levels] mvScaleFactors */
    int32_t n_levels;           /* mnScaleLevels, <= 64 */
    float log_scale_factor;     /* mfLogScaleFactor */
} rsc_frame_features;

typedef struct rsc_frameview rsc_frameview;
/* Upload the current Frame as the matcher reads it to HBM (host copies of the keypoints, octaves and
 * 1 / sigma^2 per level are kept for the PoseOptimization problems of rsc_reloc_refine_many). */
int rsc_frameview_create(rsc_context* ctx, const rsc_frame_features* frame, rsc_frameview** out);
void rsc_frameview_destroy(rsc_frameview* view);
/* The KeyFrame's keypoint angles, angle[i] = mvKeysUn[i].angle (view n entries): the rotation check of
 * SearchByProjection reads them and rsc_sim3_kf carries none. */
int rsc_kfview_set_angles(rsc_kfview* view, const float* angle);

/* SearchByProjection(CurrentFrame = frames[c], pKF = kfs[c], sAlreadyFound, th, ORBdist) for c < count in
 * one launch (one workgroup per problem).  Tcw [count][16]: CurrentFrame.mTcw, row-major.
 * already[c][i] (kfs[c] n entries): sAlreadyFound.count(vpMPs[i]).  frame_mp[c][f] (frames[c] n
 * entries) >= 0: CurrentFrame.mvpMapPoints[f] is set before the call (not modified).  out[c][f]: the
 * KeyFrame slot whose MapPoint the call writes to mvpMapPoints[f] and the rotation check keeps, else
 * -1; nmatches[c] = the return value; rounds (may be NULL): fixed-point rounds run (diagnostic).
 * check_orientation = mbCheckOrientation: needs rsc_kfview_set_angles on every kfs[c] (RSC_ERR_ARG
 * otherwise).  orb_dist outside [0, 255] is RSC_ERR_ARG. */
int rsc_search_by_projection_many(rsc_context* ctx, rsc_frameview* const* frames, rsc_kfview* const* kfs, int count,
                                  const float* Tcw, const uint8_t* const* already, const int32_t* const* frame_mp,
                                  float th, int orb_dist, int check_orientation, int32_t* const* out,
                                  int32_t* nmatches, int32_t* rounds);

/* Tracking::Relocalization's refinement chain (Tracking.cpp:1294-1323) for `count` candidates:
 * SearchByProjection(10, 100) -> PoseOptimization when nadditional + nGood >= 50 -> for 30 < nGood < 50
 * SearchByProjection(3, 64) with sFound = every occupied slot -> PoseOptimization and removal of its
 * outliers when nGood + nadditional >= 50.  Each stage is one launch over the candidates still in the
 * chain; each search reads the pose the optimisation before it wrote. */
typedef struct {
    int32_t n_good;           /* nGood after the chain (n_good_in when no optimisation ran) */
    int32_t n_additional[2];  /* SearchByProjection's return values, -1 when the stage did not run */
    int32_t pose_opts;        /* PoseOptimization runs, 0..2 */
    float Tcw[16];            /* mCurrentFrame.mTcw after the chain */
} rsc_reloc_refine_result;
/* frame_mp[c][f] (in/out, frames[c] n entries): the KeyFrame slot of mCurrentFrame.mvpMapPoints[f] or
 * -1, on entry after the outliers of the first PoseOptimization were removed (:1289-1291).  found[c]
 * (kfs[c] n entries): sFound as built at :1278, from ALL RANSAC inliers.  n_good_in / Tcw_in
 * [count][16]: nGood and mTcw of that first PoseOptimization.  fr[c]: the Frame's mvuRight / mbf.  The
 * optimisations read uv = the Frame keypoint, Xw = the KeyFrame view's mp_pos[slot], inv_sigma2 =
 * 1.0f / (s * s) with s = the scale factor of the Frame keypoint's octave. */
int rsc_reloc_refine_many(rsc_context* ctx, rsc_frameview* const* frames, rsc_kfview* const* kfs, int count,
                          const rsc_reloc_frame* fr, int32_t* const* frame_mp, const uint8_t* const* found,
                          const int32_t* n_good_in, const float* Tcw_in, rsc_reloc_refine_result* out);

/* Tracking::Relocalization (Tracking.cpp:1239-1335) from the candidate solvers to bMatch: the loop of
 * rsc_reloc_events_gated with the refinement chain inside.  A success with 10 <= nGood < 50 goes
 * through rsc_reloc_refine_many (batched over the events of the pass); nGood >= 50 afterwards is
 * RSC_GATE_MATCH, otherwise the walk continues with the next success of the round (:1327-1333).
 * status is RSC_GATE_MATCH or RSC_GATE_NONE.  Own-stream solvers only (RSC_ERR_UNSUPPORTED). */
typedef struct {
    rsc_kfview* kf;          /* vpCandidateKFs[i] (with angles) */
    const int32_t* matches;  /* [Frame n] vvpMapPointMatches[i] as KeyFrame slots, -1 NULL: the output of
                                rsc_search_by_bow_frame_many the candidate's solver was built from */
} rsc_reloc_candidate;
typedef struct {
    int32_t status, winner, round, hypothesis, n_inliers;  /* as rsc_reloc_gate_result */
    int32_t n_good;           /* nGood of the accepted success at :1327 (after its chain, if one ran) */
    int32_t rejected;         /* successes rejected before it (nGood < 10, or < 50 after the chain) */
    int32_t gates;            /* first PoseOptimization runs of the event */
    int32_t n_good_first;     /* the winner's nGood at :1284 */
    int32_t n_additional[2];  /* the winner's chain (-1: stage not run) */
    int32_t chains;           /* refinement chains run in the event */
    float Tcw[16];            /* mCurrentFrame.mTcw of the accepted success */
} rsc_reloc_refined_result;
/* views[e]: event e's current Frame; candidates[i]: per solver.  frame_mp_out[e] (may be NULL / NULL
 * entries): [Frame n] mCurrentFrame.mvpMapPoints of the accepted success as KeyFrame slots of the
 * winner (-1 NULL); untouched for RSC_GATE_NONE. */
int rsc_reloc_events_refined(rsc_pnp* const* solvers, const rsc_reloc_candidate* candidates,
                             const int32_t* event_begin, int n_events, rsc_frameview* const* views,
                             const rsc_reloc_frame* frames, rsc_pnp_result* per_candidate,
                             rsc_reloc_refined_result* per_event, int32_t* const* frame_mp_out);

/* ---- The loop-closing projection matchers over a flat MapPoint list ------------------------------
 * ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cpp:241-352) and
 * ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:823-946): the two matcher calls of
 * LoopClosing::ComputeSim3 (LoopClosing.cpp:360) and LoopClosing::SearchAndFuse (:578-600) over
 * mvpLoopMapPoints.  Every point that passes the gates (depth z >= 0, KeyFrame::IsInImage with the
 * maximum excluded, 0.8 dmin <= dist <= 1.2 dmax, PO.Pn >= 0.5 dist) takes the keypoint of the predicted
 * levels [L-1, L] with the smallest descriptor distance (<= TH_LOW = 50) inside th * scale[L] of its
 * projection.  SearchByProjection skips keypoints whose vpMatched slot is set, by the caller or by an
 * earlier point of the call (the reference's sequential order is reproduced exactly); Fuse skips none. */
typedef struct {
    int32_t n;             /* vpPoints.size() */
    const uint8_t* state;  /* [n] 1 = good, 2 = isBad() */
    const float* pos;      /* [n][3] GetWorldPos() */
    const float* normal;   /* [n][3] GetNormal() */
    const float* dmax;     /* [n] mfMaxDistance */
    const float* dmin;     /* [n] mfMinDistance */
    const uint8_t* desc;   /* [n][32] GetDescriptor() */
} rsc_mappoints;
typedef struct rsc_mpview rsc_mpview;
/* Upload a MapPoint list to HBM once; the view is shared by the projection call and by every Fuse call of
 * a loop correction.  Precondition: the points are distinct MapPoints (the reference builds
 * mvpLoopMapPoints through mnLoopPointForKF, LoopClosing.cpp:350-353, which guarantees it). */
int rsc_mpview_create(rsc_context* ctx, const rsc_mappoints* points, rsc_mpview** out);
void rsc_mpview_destroy(rsc_mpview* view);

/* SearchByProjection(pKF = kfs[c], Scw[c], vpPoints = points[c], vpMatched, th) for c < count in one launch
 * (one workgroup per problem).  Scw [count][16] row-major: the Isometry3f as the reference passes it; with
 * mScw = Converter::toIso(g2o::Sim3) that is the unit rotation and the translation NOT divided by the
 * scale, and the matcher uses both as they are (Ow = -R^T t), which this call keeps.
 * already[c][i] (points[c] n entries): spAlreadyFound.count(vpPoints[i]), the point is in vpMatched on
 * entry.  occupied[c][idx] (kfs[c] n entries): vpMatched[idx] != NULL on entry.  out[c][idx]: index into
 * points[c] of the MapPoint the call writes to vpMatched[idx], else -1; nmatches[c] = the return value;
 * rounds (may be NULL): fixed-point rounds run (diagnostic).  A KeyFrame with n > 8192 is RSC_ERR_ARG.
 * Camera z == 0 is defined: the projection is inf / NaN, IsInImage is false, the point is skipped. */
int rsc_search_by_projection_kf_many(rsc_context* ctx, rsc_kfview* const* kfs, rsc_mpview* const* points, int count,
                                     const float* Scw, const uint8_t* const* already,
                                     const uint8_t* const* occupied, int th, int32_t* const* out,
                                     int32_t* nmatches, int32_t* rounds);

/* Fuse(pKF = kfs[c], Scw[c], vpPoints = points, th, vpReplacePoint) for c < count in one launch, one lane
 * per (point, KeyFrame) pair.  Scw [count][16] row-major with linear() = s * R; the call divides by
 * scw = sqrt(row0 . row0) as the reference does.  in_kf[c][i] (points n entries):
 * pKF->GetMapPoints().count(vpPoints[i]).  best_idx[c][i]: bestIdx when bestDist <= 50, else -1; the
 * caller does the bookkeeping of :930-940 from the KeyFrame's own slot (replace, or AddObservation /
 * AddMapPoint).  nfused[c] = the return value (the number of best_idx[c][i] >= 0). */
int rsc_fuse_sim3_many(rsc_context* ctx, rsc_kfview* const* kfs, int count, rsc_mpview* points, const float* Scw,
                       const uint8_t* const* in_kf, float th, int32_t* const* best_idx, int32_t* nfused);

/* The closing stage of LoopClosing::ComputeSim3 (LoopClosing.cpp:318-320, :360-370) on the result of
 * rsc_loop_events_gated, for `count` accepted events in one launch: gSmw from kf_matched's pose,
 * mg2oScw = gScm * gSmw, mScw = toIso(mg2oScw), SearchByProjection(mpCurrentKF, mScw, mvpLoopMapPoints,
 * mvpCurrentMatchedPoints, 10), nTotalMatches >= 40.  The composition is host arithmetic in double
 * (csrc/rsc_sim3compose.h; its parity with the reference binary is unpinned). */
typedef struct {
    int32_t accepted;    /* nTotalMatches >= 40 */
    int32_t n_projected; /* SearchByProjection's return value */
    int32_t n_total;     /* nTotalMatches */
    double Scw_sim3[8];  /* mg2oScw: q (x, y, z, w), t, s */
    float Scw[16];       /* mScw, row-major */
} rsc_loop_verify_result;
/* S [count][8]: rsc_loop_gate_result.S.  matches[c] (kf_cur[c] n entries): matches_out of the gate; a slot
 * is occupied when matches[c][idx] != -1 (-2, a MapPoint not in the matched KeyFrame, is a non-null
 * pointer).  already[c][i] (loop_points[c] n entries): the point is in mvpCurrentMatchedPoints.
 * projected (may be NULL / NULL entries): [kf_cur n] as `out` of rsc_search_by_projection_kf_many. */
int rsc_loop_verify_many(rsc_context* ctx, rsc_kfview* const* kf_cur, rsc_kfview* const* kf_matched,
                         rsc_mpview* const* loop_points, int count, const double* S,
                         const int32_t* const* matches, const uint8_t* const* already,
                         rsc_loop_verify_result* out, int32_t* const* projected);

/* ---- Tracking::SearchLocalPoints: the frustum test and the local-map projection matcher -------------
 * Tracking::SearchLocalPoints (src/Tracking.cpp:1003-1028) = Frame::isInFrustum(pMP, 0.5)
 * (src/Frame.cpp:336-392) over mvpLocalMapPoints, then ORBmatcher::SearchByProjection(Frame&,
 * vector<MapPoint>&, th) (src/ORBmatcher.cpp:16-100), over a resident Frame (rsc_frameview with
 * rsc_frameview_set_stereo) and a flat MapPoint list (rsc_mpview).  Every point in view takes, among the
 * Frame features of levels [L-1, L] inside r * th * scale[L] of its projection (r = 2.5 when viewCos >
 * 0.998, else 4.0) that pass the stereo gate and hold no MapPoint with observations, the one with the
 * smallest descriptor distance, if that is <= TH_HIGH = 100 and not vetoed by the runner-up (same level,
 * bestDist > nn_ratio * bestDist2).  A feature taken by an earlier point of the call is skipped only when
 * that point has observations; otherwise a later point may take it again and overwrite it (both count).
 * The reference's sequential order is reproduced exactly.  Precondition: no eligible point projects to a
 * NaN pixel (camera z == 0 with x == 0 or y == 0, undefined in the reference); such a point is skipped. */
typedef struct {
    int32_t in_view;  /* mbTrackInView */
    float proj_x;     /* mTrackProjX */
    float proj_y;     /* mTrackProjY */
    float proj_xr;    /* mTrackProjXR */
    int32_t level;    /* mnTrackScaleLevel */
    float view_cos;   /* mTrackViewCos */
} rsc_track_record;

/* The Frame's mvuRight (view n entries, negative for a monocular feature) and mbf: isInFrustum writes
 * mTrackProjXR = u - mbf / z and the matcher's stereo gate reads both; rsc_frame_features carries none. */
int rsc_frameview_set_stereo(rsc_frameview* view, const float* u_right, float mbf);

/* Tracking.cpp:1003-1028 for c < count in one launch (one workgroup per problem).  Tcw [count][16]:
 * mCurrentFrame.mTcw, row-major.  skip[c][i] (points[c] n entries): mnLastFrameSeen == mCurrentFrame.mnId
 * (:1006); isBad() is the view's state.  has_obs[c][i]: Observations() > 0 of point i.  frame_occ[c][f]
 * (frames[c] n entries): 0 = F.mvpMapPoints[f] is NULL on entry, 1 = set with Observations() == 0, 2 = set
 * with Observations() > 0.  cos_limit = viewingCosLimit (0.5), th and nn_ratio as the reference's call
 * (nn_ratio >= 0).  out[c][f]: index into points[c] of the MapPoint the call leaves in F.mvpMapPoints[f],
 * else -1 (an entry occupant that nobody overwrote is not reported).  track[c][i] (out): what isInFrustum
 * leaves in point i, for the caller's mbTrackInView... write-back and IncreaseVisible (in_view = 0 and
 * zeros for a point that is skipped, bad or outside).  n_to_match[c] = nToMatch; nmatches[c] = the
 * matcher's return value (the reference skips the matcher when nToMatch == 0, which returns 0 here too);
 * rounds (may be NULL): fixed-point rounds run (diagnostic).  A Frame with n > 8192 or without
 * rsc_frameview_set_stereo is RSC_ERR_ARG; count == 0 and empty point lists are RSC_OK.  With timing
 * enabled, rsc_context_last_kernel_timing gives [0] the setup kernel, [1] the rounds kernel, [2] both (ms). */
int rsc_search_local_points_many(rsc_context* ctx, rsc_frameview* const* frames, rsc_mpview* const* points,
                                 int count, const float* Tcw, const uint8_t* const* skip,
                                 const uint8_t* const* has_obs, const uint8_t* const* frame_occ, float cos_limit,
                                 float th, float nn_ratio, int32_t* const* out, rsc_track_record* const* track,
                                 int32_t* nmatches, int32_t* n_to_match, int32_t* rounds);

/* The bare ORBmatcher::SearchByProjection(F, vpMapPoints, th) (ORBmatcher.cpp:16-100): as above with
 * track[c][i] as an INPUT holding the host's mbTrackInView, mTrackProjX / Y / XR, mnTrackScaleLevel and
 * mTrackViewCos (a level outside [0, n_levels) on a point in view is RSC_ERR_ARG).  A point with skip[c][i]
 * set is left out like one with mbTrackInView false.  n_to_match[c] = the points that reach the window. */
int rsc_search_by_projection_points_many(rsc_context* ctx, rsc_frameview* const* frames,
                                         rsc_mpview* const* points, int count, const uint8_t* const* skip,
                                         const uint8_t* const* has_obs, const uint8_t* const* frame_occ, float th,
                                         float nn_ratio, int32_t* const* out,
                                         const rsc_track_record* const* track, int32_t* nmatches,
                                         int32_t* n_to_match, int32_t* rounds);

/* ---- Tracking::TrackWithMotionModel: the last-frame matcher and its driver ---------------------------
 * ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th)
 * (src/ORBmatcher.cpp:1173-1315) over a resident current Frame (rsc_frameview with rsc_frameview_set_stereo)
 * and the last Frame's slots (rsc_lastframe).  Every LastFrame slot with a MapPoint that is not an outlier
 * projects its MapPoint with CurrentFrame.mTcw and takes, among the current features inside th *
 * scale[LastFrame octave] of the projection (strictly), at the levels of the call's mode, that pass the
 * stereo gate and hold no MapPoint with observations, the first one of the smallest descriptor distance, if
 * that is <= TH_HIGH = 100.  The mode is one per call (:1186-1194): 1 forward (tlc.z > mb, octaves >= o), 2
 * backward (-tlc.z > mb, octaves [0, o]), 0 otherwise (octaves [o-1, o+1]).  A slot whose MapPoint has no
 * observations takes a feature and blocks nobody: a later slot may take it again, and both count.  The
 * rotation histogram holds one entry per claim and the removal runs per entry (:1301-1311), so a feature is
 * left nullptr when ANY of its claimers fell into a removed bin, and the return value is (claims) - (claims in
 * removed bins).  The reference's sequential order is reproduced exactly.  Precondition: no eligible point
 * projects to a NaN pixel (camera z == 0 with x == 0 or y == 0, or a non-finite position; undefined in the
 * reference); such a point is skipped. */
typedef struct {
    int32_t n;                 /* LastFrame.N, at most 8192 */
    const int32_t* octave;     /* [n] mvKeys[i].octave */
    const float* angle;        /* [n] mvKeysUn[i].angle */
    const uint8_t* mp_state;   /* [n] 0 = mvpMapPoints[i] is NULL, 1 = set, 2 = set and mvbOutlier[i] */
    const float* mp_pos;       /* [n][3] GetWorldPos() (read where mp_state != 0) */
    const uint8_t* mp_desc;    /* [n][32] MapPoint::GetDescriptor(), not the Frame's descriptor row */
    const uint8_t* mp_has_obs; /* [n] Observations() > 0 */
} rsc_last_frame_slots;

typedef struct rsc_lastframe rsc_lastframe;

/* Uploads the last Frame as it stands after Tracking::UpdateLastFrame() (src/Tracking.cpp:648-712, which
 * stays with the caller), once per frame.  n > 8192 is RSC_ERR_ARG. */
int rsc_lastframe_create(rsc_context* ctx, const rsc_last_frame_slots* slots, rsc_lastframe** out);
void rsc_lastframe_destroy(rsc_lastframe* view);

/* ORBmatcher.cpp:1173-1315 for c < count in one launch (one workgroup per problem).  Tcw_cur / Tcw_last
 * [count][16]: CurrentFrame.mTcw / LastFrame.mTcw, row-major; mb[count]: CurrentFrame.mb.  frame_occ[c][f] as
 * in rsc_search_local_points_many (0, 1 or 2); frame_occ or frame_occ[c] NULL = every slot NULL on entry.
 * out[c][f] (frames[c] n entries): >= 0 the LastFrame slot whose MapPoint the call leaves in
 * CurrentFrame.mvpMapPoints[f]; -1 the slot is left as on entry; -2 the rotation check set it to nullptr.
 * nmatches[c] = the return value; mode[c] (may be NULL) = 0 window, 1 forward, 2 backward; rounds (may be
 * NULL): fixed-point rounds run (diagnostic, 1 without an eligible slot).  RSC_ERR_ARG, before any launch:
 * more than 8192 features or slots; a Frame view without rsc_frameview_set_stereo; an octave outside
 * [0, n_levels) on a slot that has a MapPoint; a non-finite th, or |th| * scale[n_levels-1] * max(grid_w_inv,
 * grid_h_inv) >= 2^30 (GetFeaturesInArea converts the cell coordinate to int, Frame.cpp:399-411).  count == 0
 * and a LastFrame without eligible slots are RSC_OK.  With timing enabled, rsc_context_last_kernel_timing
 * gives [0] the setup kernel, [1] the rounds kernel, [2] both (ms). */
int rsc_search_by_projection_last_many(rsc_context* ctx, rsc_frameview* const* frames, rsc_lastframe* const* lasts,
                                       int count, const float* Tcw_cur, const float* Tcw_last, const float* mb,
                                       const uint8_t* const* frame_occ, float th, int check_orientation,
                                       int32_t* const* out, int32_t* nmatches, int32_t* mode, int32_t* rounds);

typedef struct {
    int32_t ok;                 /* the return value of TrackWithMotionModel */
    int32_t searches;           /* 1 or 2 */
    int32_t nmatches_search[2]; /* the matcher's return value at th and at 2 * th (-1: did not run) */
    int32_t mode;               /* as rsc_search_by_projection_last_many */
    int32_t nmatches;           /* after the outlier discard (Tracking.cpp:761) */
    int32_t nmatches_map;       /* nmatchesMap (:763-764) */
    int32_t vo;                 /* mbVO = nmatchesMap < 10, set with only_tracking (:770); else 0 */
    int32_t n_good;             /* PoseOptimization's return value (0 when it did not run) */
    float Tcw[16];              /* mCurrentFrame.mTcw afterwards (Tcw_cur when PoseOptimization did not run) */
} rsc_track_motion_result;

/* Tracking::TrackWithMotionModel (src/Tracking.cpp:724-774) for `count` frames: one search launch at th from
 * an empty mvpMapPoints (:724-732), one at 2 * th, again from empty, over the frames with nmatches < 20
 * (:735-739), one rsc_pose_optimization_many launch over the frames that reached 20 (:745), and the discard
 * loop (:749-766) on the host.  Tcw_cur = mVelocity * mLastFrame.mTcw as the caller computed it (:722).  th =
 * 15 or 7 (:728-731); only_tracking[count] = mbOnlyTracking of each frame's Tracking object.  A frame that
 * stays below 20 has ok = 0 and its second search's matches in out[c], as the reference leaves them
 * (slots the rotation check nulled read -1).  out[c][f]: the LastFrame slot in
 * mvpMapPoints[f] after the discard, else -1; discarded[c][f]: the LastFrame slot whose MapPoint was removed
 * as an outlier (the caller sets its mbTrackInView = false and mnLastFrameSeen), else -1.  nmatches starts
 * from the matcher's return value, double counts included, as in the reference.  Arguments are checked as in
 * rsc_search_by_projection_last_many, for th and 2 * th. */
int rsc_track_motion_model_many(rsc_context* ctx, rsc_frameview* const* frames, rsc_lastframe* const* lasts,
                                int count, const float* Tcw_cur, const float* Tcw_last, const float* mb, float th,
                                const int32_t* only_tracking, rsc_track_motion_result* result,
                                int32_t* const* out, int32_t* const* discarded);

/* ---- KeyFrameDatabase: BoW candidate scoring (src/KeyFrameDatabase.cpp) ---------------------- */
/* A device-resident keyframe database: each KeyFrame is a slot in [0, capacity) holding its
 * BowVector (word ids ascending, TF-IDF values, DBoW2 L1_NORM scoring), its
 * GetBestCovisibilityKeyFrames(10) list and the per-KeyFrame query state of the reference
 * (mnLoopQuery/mnLoopWords/mLoopScore, mnRelocQuery/mnRelocWords/mRelocScore, KeyFrame.hpp:129-134),
 * which persists across queries exactly as the KeyFrame members do.  Replaces
 * KeyFrameDatabase (include/KeyFrameDatabase.hpp). */
typedef struct rsc_kfdb rsc_kfdb;
/* KeyFrameDatabase(voc) (KeyFrameDatabase.cpp:8-13): vocab_words = voc->size() (word ids are below
 * it; 10^6 for ORBvoc.txt), capacity slots, max_words (<= 4096) bounds one BowVector. */
int rsc_kfdb_create(rsc_context* ctx, uint32_t vocab_words, int capacity, int max_words, rsc_kfdb** out);
void rsc_kfdb_destroy(rsc_kfdb* db);
/* add(pKF) (:15-21): ids strictly ascending (a std::map BowVector) and below vocab_words; a slot
 * already present ->
 * RSC_ERR_UNSUPPORTED (the reference would list it twice per word). */
int rsc_kfdb_add(rsc_kfdb* db, int kf, int n_words, const uint32_t* word_id, const double* word_value);
/* erase(pKF) (:23-43); erasing an absent slot is a no-op as in the reference. */
int rsc_kfdb_erase(rsc_kfdb* db, int kf);
/* Frees slot kf for reuse by another KeyFrame (not a reference operation): erase + the slot's
 * query state and covisibility row reset to the fresh-KeyFrame values (KeyFrame.cpp:15).  The
 * facade calls it when a KeyFrame leaves the database. */
int rsc_kfdb_release(rsc_kfdb* db, int kf);
/* clear() (:45-49): empties the inverted file; the per-KeyFrame query state is kept. */
int rsc_kfdb_clear(rsc_kfdb* db);
/* pKF->GetBestCovisibilityKeyFrames(10) of slot kf (n <= 10 slots, in order). */
int rsc_kfdb_set_covisibility(rsc_kfdb* db, int kf, int n, const int32_t* best);
/* The same for count slots at once (kf[c], n[c] <= 10, best[c][10] row-major); only the span of
 * rows whose content changed is uploaded. */
int rsc_kfdb_set_covisibility_many(rsc_kfdb* db, int count, const int32_t* kf, const int32_t* n,
                                   const int32_t* best);
/* DetectRelocalizationCandidates(F) (:174-283): frame_id = F->mnId, (word_id, word_value) =
 * F->mBowVec.  candidates (room for 1 + the highest slot added or referenced so far; capacity
 * always suffices): the returned vector's slots in order.  Queries sweep only the slots in use. */
int rsc_kfdb_detect_relocalization(rsc_kfdb* db, uint64_t frame_id, int n_words, const uint32_t* word_id,
                                   const double* word_value, int32_t* candidates, int32_t* n_candidates);
/* DetectLoopCandidates(pKF, minScore) (:52-172): kf_id = pKF->mnId, connected =
 * pKF->GetConnectedKeyFrames() (slots). */
int rsc_kfdb_detect_loop(rsc_kfdb* db, uint64_t kf_id, int n_words, const uint32_t* word_id,
                         const double* word_value, int n_connected, const int32_t* connected, float min_score,
                         int32_t* candidates, int32_t* n_candidates);
/* Per-slot query state (parity hook): q[2] = {mnLoopQuery, mnRelocQuery}, w[2] = {mnLoopWords,
 * mnRelocWords}, s[2] = {mLoopScore, mRelocScore}. */
int rsc_kfdb_state(rsc_kfdb* db, int kf, uint64_t* q, int32_t* w, float* s);

/* ---- ORBVocabulary::transform (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1194) -------
 * Frame::ComputeBoW / KeyFrame::ComputeBoW (src/Frame.cpp:462-469, src/KeyFrame.cpp:46-55): the
 * descriptors of a view descend the vocabulary tree; the leaves give the BowVector (TF-IDF weights,
 * L1-normalised), the nodes `levelsup` levels above the leaves give the FeatureVector.  The tree is
 * uploaded once and stays resident.  Integer descent + the reference's order of FP64 adds: results
 * are bit-exact with the reference. */
#define RSC_VOC_TF_IDF 0   /* DBoW2::WeightingType */
#define RSC_VOC_L1_NORM 0  /* DBoW2::ScoringType */
typedef struct {
    int32_t k, L;              /* m_k, m_L of the header line (k is informative: child counts come from parent[]) */
    int32_t scoring;           /* only RSC_VOC_L1_NORM, */
    int32_t weighting;         /* with RSC_VOC_TF_IDF (what ORBvoc.txt declares): else RSC_ERR_UNSUPPORTED */
    int32_t n_nodes;           /* m_nodes.size(), root (node 0) included; >= 2 */
    const int32_t* parent;     /* [n_nodes] parent[0] ignored; 0 <= parent[i] < i (RSC_ERR_ARG otherwise); the
                                  children of a node are its children vector in ascending node id; more
                                  than 32 under one node is RSC_ERR_UNSUPPORTED */
    const uint8_t* is_leaf;    /* [n_nodes] nIsLeaf > 0: the node is a word (word id = its rank among these) */
    const uint8_t* desc;       /* [n_nodes][32] node descriptors (the root's is unused) */
    const double* weight;      /* [n_nodes] node weights (a leaf's weight <= 0: a stopped word) */
    int32_t lds_budget_bytes;  /* 0 = default.  TEST HOOK: the byte budget (<= 48 KiB) of the tree levels
                                  staged in LDS by the descent (40 B per node, whole levels) */
} rsc_vocabulary_nodes;

typedef struct rsc_voc rsc_voc;

int rsc_voc_create(rsc_context* ctx, const rsc_vocabulary_nodes* nodes, rsc_voc** out);
void rsc_voc_destroy(rsc_voc* voc);
/* voc->size(): the number of words (rsc_kfdb_create's vocab_words). */
int rsc_voc_size(const rsc_voc* voc, uint32_t* n_words);
/* Layout facts (diagnostic): info[0] nodes staged in LDS, [1] the tree levels they make, [2] the
 * shallowest and [3] the deepest leaf depth, [4] the most children of one node. */
int rsc_voc_info(const rsc_voc* voc, int32_t* info);

/* One view's transform outputs; every array has room for the view's n entries (node_begin: n + 1)
 * and may be NULL when not wanted. */
typedef struct {
    int32_t n_words;            /* BowVector: size, */
    uint32_t* word_id;          /*   keys ascending, */
    double* word_value;         /*   values */
    int32_t n_nodes;            /* FeatureVector: size, keys ascending, CSR as in rsc_bow_features */
    uint32_t* node_id;
    int32_t* node_begin;
    uint32_t* feat;
    uint32_t* feature_word;     /* parity hook, per feature: word id, */
    uint32_t* feature_node;     /*   node id at nid_level, */
    uint8_t* feature_stopped;   /*   1 when the leaf weight is not > 0 */
} rsc_voc_output;

/* transform(desc[c], BowVector, FeatureVector, levelsup) for c < count in one call (a Frame and the
 * KeyFrames inserted since; a batch of relocalization events).  n[c] <= 8192 descriptors of 32
 * bytes; n[c] = 0 gives empty vectors.  L - levelsup above the vocabulary's shallowest leaf depth is
 * RSC_ERR_UNSUPPORTED (the reference reads an uninitialised NodeId there).  The work buffers belong to
 * the vocabulary: calls on one rsc_voc must not overlap (the facade serialises them). */
int rsc_voc_transform_many(rsc_voc* voc, int count, const int32_t* n, const uint8_t* const* desc, int levelsup,
                           rsc_voc_output* out);
/* Device time (ms) of the last transform's descent and build kernels (needs
 * rsc_context_enable_timing). */
int rsc_voc_last_kernel_timing(rsc_voc* voc, double* ms2);

/* rsc_bow_create with the FeatureVector computed by the vocabulary: features->n_nodes / node_id /
 * node_begin / feat are ignored; the view's node arrays are written on the device by the transform.
 * bow (may be NULL) receives the BowVector (and whatever else it asks for), for rsc_kfdb_add and
 * rsc_kfdb_detect_*. */
int rsc_bow_create_transformed(rsc_context* ctx, rsc_voc* voc, const rsc_bow_features* features, int levelsup,
                               rsc_bow** out, rsc_voc_output* bow);

/* ---- LocalMapping::CreateNewMapPoints: SearchForTriangulation and the triangulation ------------
 * What triangulation reads and a rsc_kfview lacks (in the style of rsc_kfview_set_angles). */
typedef struct {
    const float* u_right;              /* [n] mvuRight (negative: monocular; `>= 0` is stereo, ORBmatcher.cpp:537) */
    const float* depth;                /* [n] mvDepth */
    const float* kp_raw;               /* [n][2] mvKeys[i].pt: UnprojectStereo reads mvKeys, not mvKeysUn
                                          (KeyFrame.cpp:611-612) */
    const float* cos_parallax_stereo;  /* [n] cos(2*atan2(mb/2, mvDepth[i])), the expression of
                                          LocalMapping.cpp:286,288 evaluated by the caller's libm; read only
                                          where u_right[i] >= 0 */
    float mb, mbf, invfx, invfy;
    float scale_factor;                /* mfScaleFactor */
    float Rwc[9], Ow[3];               /* Twc as KeyFrame::SetPose stored it (KeyFrame.cpp:64-66), row-major */
    float Kinv[9];                     /* KeyFrame::mKinv, row-major (ComputeF12, LocalMapping.cpp:527-528) */
} rsc_kf_triangulation;
int rsc_kfview_set_triangulation(rsc_kfview* view, const rsc_kf_triangulation* t);

/* ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) (ORBmatcher.cpp:489-669)
 * for c < count in one launch.  bow1[c] / kf1[c] are the two resident views of KeyFrame 1 (same n), bow2[c] /
 * kf2[c] of KeyFrame 2; both kfviews carry rsc_kfview_set_triangulation.  F12: [count][9] row-major.
 * has_mp1 / has_mp2 (the arrays or single entries may be NULL): uint8 [n], GetMapPoint(idx) != nullptr, bad
 * points included; NULL takes the view's mp_state != 0.  only_stereo: [count] bOnlyStereo of each call (NULL: all
 * false).  check_orientation: mbCheckOrientation (a member of the matcher object in the reference, so one value
 * per launch), read from the rsc_bow views' angles.  Outputs: matches12[c][i1] = KeyFrame-2 index or -1 (vMatchedPairs = its non-negative
 * entries in ascending i1), nmatches[c], den_zero[c] = 1 when an eligible slot's epipolar line had den == 0
 * (`return false`, :552-553: nmatches 0, all -1, the reference leaves vMatchedPairs untouched), den_zero_slot
 * [c][i1] = 1 on those slots (either may be NULL).  vbMatched2 is never set in the reference, so two slots may
 * share a KeyFrame-2 feature; reproduced.  RSC_ERR_ARG before any launch: n > 8192, bow / kfview sizes that
 * differ, a view without rsc_kfview_set_triangulation, a KeyFrame-2 octave outside [0, n_levels), a
 * non-finite F12. */
int rsc_search_for_triangulation_many(rsc_context* ctx, const rsc_bow* const* bow1, rsc_kfview* const* kf1,
                                      const rsc_bow* const* bow2, rsc_kfview* const* kf2, int count,
                                      const float* F12, const uint8_t* const* has_mp1,
                                      const uint8_t* const* has_mp2, const int32_t* only_stereo,
                                      int check_orientation,
                                      int32_t* const* matches12, int32_t* nmatches, int32_t* den_zero,
                                      uint8_t* const* den_zero_slot);

/* The body of CreateNewMapPoints' match loop (LocalMapping.cpp:262-407) for npairs[c] pairs (idx1 in kf1[c] =
 * the current KeyFrame, idx2 in kf2[c]), pairs[c]: int32 [npairs][2].  status[c][k] names the `continue` the
 * pair took: 0 success, 1 temp(3) == 0 (:309), 2 no stereo and low parallax (:326), 3 z1 <= 0, 4 z2 <= 0,
 * 5 / 6 reprojection error in KeyFrame 1 / 2, 7 a zero distance (:398), 8 scale consistency (:406); x3d[c][k]
 * [3] the point.  The float JacobiSVD<Matrix4f> is restated (two-sided Jacobi; parity with an Eigen build
 * unpinned).  Quirks kept: cosParallaxStereo2 is read only when KeyFrame 1's feature is not stereo (:287);
 * KeyFrame 2's right-image error uses the current KeyFrame's mbf (:382).  RSC_ERR_ARG: an index or octave
 * out of range, a view without rsc_kfview_set_triangulation. */
int rsc_triangulate_pairs_many(rsc_context* ctx, rsc_kfview* const* kf1, rsc_kfview* const* kf2, int count,
                               const int32_t* npairs, const int32_t* const* pairs, int32_t* const* status,
                               float* const* x3d);

/* LocalMapping::CreateNewMapPoints' neighbour loop (LocalMapping.cpp:224-428) for count current KeyFrames:
 * neighbours neigh_begin[c] .. neigh_begin[c + 1] of bow_neigh / kf_neigh are vpNeighKFs of c in order (pass
 * only as many as the caller is prepared to process: CheckNewKeyFrames, :226, cannot be polled inside the
 * call).  Per neighbour: the baseline gate (:232-236), ComputeF12 (:512-531) on the host,
 * SearchForTriangulation(.., false) with the orientation check off (ORBmatcher matcher(0.6, false), :202),
 * the triangulation; a success fills the KeyFrame-1 slot, which later neighbours skip.  One matcher launch
 * and one triangulation launch from the initial slot state (mp_state != 0), then the neighbour order is
 * replayed on the host.  Outputs per current KeyFrame, indexed by its slot i1 (a slot is filled at most
 * once): new_neighbour[c][i1] = index into c's neighbour list or -1, new_idx2[c][i1], new_pos[c][i1][3],
 * nnew[c].  The reference's creation order is (neighbour, i1) ascending.  MapPoint allocation and
 * AddObservation / AddMapPoint stay with the caller; ComputeDistinctiveDescriptors and UpdateNormalAndDepth of
 * the new points (:418-420) are one rsc_update_map_points_many call. */
int rsc_create_new_map_points_many(rsc_context* ctx, const rsc_bow* const* bow_cur, rsc_kfview* const* kf_cur,
                                   int count, const int32_t* neigh_begin, const rsc_bow* const* bow_neigh,
                                   rsc_kfview* const* kf_neigh, int32_t* const* new_neighbour,
                                   int32_t* const* new_idx2, float* const* new_pos, int32_t* nnew);

/* ---- LocalMapping::SearchInNeighbors: ORBmatcher::Fuse(pKF, vpMapPoints, th) -------------------------
 * Fuse(pKF = kfs[c], vpMapPoints = points[c], th) (src/ORBmatcher.cpp:671-821) for c < count in one launch
 * over every (point, KeyFrame) pair: the matcher of :698-795.  points[c] may be one view repeated (the forward
 * loop of LocalMapping.cpp:461-466) or a view per problem; the points need not be distinct, no pair depends on
 * another.  The pose is the view's Rcw / tcw, the camera centre its rsc_kf_triangulation.Ow (the stored
 * Twc.translation()), mvuRight / mbf come from there too, and mvInvLevelSigma2[l] is derived as
 * 1.0f / (scale_factors[l] * scale_factors[l]).  A keypoint with u_right >= 0 (zero included) is stereo: chi2
 * 7.8 over (ex, ey, er), else 5.99 over (ex, ey).  skip[c][i] (points[c] n entries): isBad() ||
 * IsInKeyFrame(pKF) at launch; a view state of 2 skips as well.  best_idx[c][i]: bestIdx when bestDist <= 50,
 * else -1; nfused[c] (may be NULL): the number of best_idx[c][i] >= 0.  The bookkeeping of :797-817 (Replace,
 * AddObservation, AddMapPoint) mutates the caller's map and stays with the caller, in list order
 * (facade/ORBmatcher.hpp replays it).  RSC_ERR_ARG before any launch: a kfview without
 * rsc_kfview_set_triangulation, n > 8192, a keypoint octave outside [0, n_levels), a non-finite th, th *
 * scale[n_levels - 1] * grid_inv >= 2^30 (the bound of rsc_search_by_sim3_many).  count == 0 and empty point
 * lists are RSC_OK. */
int rsc_fuse_kf_many(rsc_context* ctx, rsc_kfview* const* kfs, rsc_mpview* const* points, int count,
                     const uint8_t* const* skip, float th, int32_t* const* best_idx, int32_t* nfused);

/* ---- MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth in a batch ---------------
 * The pair of calls the reference runs on every MapPoint a mapping step touched (src/MapPoint.cpp:224-289,
 * :312-353; LocalMapping.cpp:147-148, :418-420, :493-506), for n_points points in one launch per size class.
 * Each point has an ordered observation list, the caller's iteration of mObservations; the KeyFrames are
 * rsc_kfview handles (descriptors, octaves and scale factors are resident there; the camera centre is the Ow
 * of rsc_kfview_set_triangulation).
 * what & 1, ComputeDistinctiveDescriptors: observations of a KeyFrame with kf_bad are dropped; of the N kept
 * descriptors the one whose row of Hamming distances (the zero of the diagonal included) has the smallest
 * lower median, the element of rank (int)(0.5 * (N - 1)), wins; ties go to the first in list order.  best_obs
 * is its position in the point's list, -1 when N == 0 (every KeyFrame bad: no descriptor is written).
 * what & 2, UpdateNormalAndDepth: every observation counts, bad KeyFrames included; normal = (sum over the list,
 * in order, of (pos - Ow_i) / |pos - Ow_i|) / n, dmax = |pos - Ow_ref| * scale_ref[octave_ref[ref_idx]], dmin =
 * dmax / scale_ref[n_levels - 1], every step rounded to float, IEEE divisions.  A point on a camera centre
 * yields NaN, as in the reference.  When the reference KeyFrame is not among the observations the reference
 * reads index 0 (std::map::operator[] on its copy): pass ref_idx = 0.
 * A point with skip set (mbBad) or an empty list is left untouched: its entries of `out` keep what the caller
 * put there, as does every entry of a field the call did not write for a point (desc when best_obs is -1;
 * desc and best_obs without what & 1; normal, dmax, dmin without what & 2).  updated is written for every point.
 * dst / dst_index (both may be NULL): dst_index[p] is the slot of point p in the resident view dst, or -1;
 * every field written for p is also stored into that slot on the device, other fields and slots keep their
 * bytes, so the matchers can read the view without a host round trip.
 * A limit the reference does not have: a list holds at most RSC_MPUPDATE_MAX_OBS observations.
 * RSC_ERR_ARG before any launch, outputs untouched: what outside 1..3, obs_begin not ascending, a list longer
 * than the limit, obs_kf / obs_idx / ref_kf / ref_idx / dst_index out of range, two points with one dst slot,
 * dst of another context, with what & 2 a referenced view without rsc_kfview_set_triangulation or
 * octave[ref_idx] outside [0, n_levels).  The lists of skipped points are not read.  n_points == 0 and
 * all-empty lists are RSC_OK.  Parity with an Eigen build of the reference is unpinned (as for the
 * triangulation); the arithmetic is the one stated above. */
#define RSC_MPUPDATE_MAX_OBS 1024
typedef struct {
    int32_t n_points;
    const uint8_t* skip;        /* [n_points] mbBad: the point is left untouched (NULL: none) */
    const float*   pos;         /* [n_points][3] mWorldPos */
    const int32_t* obs_begin;   /* [n_points + 1] CSR over the observations, in mObservations order */
    const int32_t* obs_kf;      /* [n_obs] index into kfs[] */
    const int32_t* obs_idx;     /* [n_obs] mit->second */
    const uint8_t* kf_bad;      /* [n_kfs] pKF->isBad() (NULL: none) */
    const int32_t* ref_kf;      /* [n_points] mpRefKF as an index into kfs[] */
    const int32_t* ref_idx;     /* [n_points] observations[pRefKF] */
} rsc_mappoint_updates;

typedef struct {
    uint8_t* desc;        /* [n_points][32] */
    int32_t* best_obs;    /* [n_points] position of BestIdx in the point's list, -1: descriptor not written */
    float*   normal;      /* [n_points][3] */
    float*   dmax, *dmin; /* [n_points] */
    uint8_t* updated;     /* [n_points] bit 0 descriptor written, bit 1 normal / depth written */
} rsc_mappoint_update_out;   /* any member may be NULL */

int rsc_update_map_points_many(rsc_context* ctx, rsc_kfview* const* kfs, int n_kfs,
                               const rsc_mappoint_updates* in, int what /* 1 descriptor | 2 normal+depth */,
                               const rsc_mappoint_update_out* out, rsc_mpview* dst, const int32_t* dst_index);
/* Diagnostic: a resident MapPoint view read back (after the work enqueued on its context); any array may be
 * NULL.  state [n], pos / normal [n][3], dmax / dmin [n], desc [n][32]. */
int rsc_mpview_download(rsc_mpview* view, uint8_t* state, float* pos, float* normal, float* dmax, float* dmin,
                        uint8_t* desc);

/* ---- Frame::ComputeStereoMatches: mvuRight and mvDepth of a resident Frame ----------------------------
 * Frame::ComputeStereoMatches() (src/Frame.cpp:538-673, the keypoint-only matcher: no image is read) for c <
 * count in one launch per phase.  The left side is the resident view frames[c] (kp = mvKeysUn, octave, desc,
 * scale_factors of rsc_frame_features); right[c] carries mvKeysRight as extracted and mDescriptorsRight.
 * With maxD = mbf / mb and r = 2 * scale[octaveL], left keypoint i (skipped when uL < 0) takes, among the right
 * keypoints with yL - r < yR <= yL + r, octaveR in [octaveL - 1, octaveL + 1] and uL - maxD <= uR <= uL, the
 * one with the smallest (descriptor distance, yR, index); -0.0f and +0.0f are one y.  It is accepted when the
 * distance is below 75 and disparity = uL - uR lies in [0, maxD): mvuRight = uR, mvDepth = mbf / disparity,
 * and for disparity == 0 mvuRight = (float)((double)uL - 0.01), mvDepth = mbf / (float)0.01.  The cut then
 * resets to -1 / -1 every accepted keypoint with (float)distance >= th_dist = 1.5f * 1.4f * median, median =
 * the element of rank size / 2 of the accepted distances (a median of 0 removes every match).  Every float
 * operation is the reference's, rounded once.
 * u_right[c] / depth[c] (frames[c] n entries): mvuRight / mvDepth.  best_right[c] / best_dist[c] (either may be
 * NULL or hold NULL entries): the matched right index and distance before the cut, -1 where nothing was
 * accepted (the reference does not keep them).  set_stereo != 0 leaves every view as
 * rsc_frameview_set_stereo(frames[c], u_right[c], mbf[c]) would, without an upload.
 * Pinned where the reference is undefined: without an accepted match nothing is removed, median = -1 and th_dist
 * = 1.5f * 1.4f * -1; mb is an argument (the reference reads Frame::mb before its constructor assigns it).
 * Limits the reference does not have: at most RSC_STEREO_MAX_RIGHT right keypoints; mbf and mb finite and > 0.
 * RSC_ERR_ARG before any launch, outputs untouched: right[c].n above the limit, such an mbf or mb, a non-finite
 * right keypoint coordinate (std::sort on NaN in the reference), a left octave outside [0, n_levels), the same
 * view twice in one call with set_stereo, a view of another context.  Right octaves may be any int32.  count ==
 * 0, a left frame with n == 0 and a right frame with n == 0 (every entry -1) are RSC_OK.  With timing enabled,
 * rsc_context_last_kernel_timing gives [0] the match kernel, [1] the cut kernel, [2] both (ms). */
#define RSC_STEREO_MAX_RIGHT 8192
typedef struct {
    int32_t n;              /* mvKeysRight.size(), <= RSC_STEREO_MAX_RIGHT */
    const float* kp;        /* [n][2] mvKeysRight[i].pt, as extracted */
    const int32_t* octave;  /* [n] */
    const uint8_t* desc;    /* [n][32] mDescriptorsRight */
} rsc_right_features;
typedef struct {
    int32_t n_candidates;   /* vDistIdx.size(): accepted before the cut */
    int32_t n_removed;      /* reset to -1 by the cut */
    int32_t median;         /* -1 when n_candidates == 0 */
    float   th_dist;
} rsc_stereo_result;
int rsc_compute_stereo_matches_many(rsc_context* ctx, rsc_frameview* const* frames,
                                    const rsc_right_features* right, int count, const float* mbf,
                                    const float* mb, int set_stereo, float* const* u_right, float* const* depth,
                                    int32_t* const* best_right, int32_t* const* best_dist,
                                    rsc_stereo_result* result);

/* Diagnostics below: `cap` = number of uint64 slots at `out`; RSC_ERR_ARG when it is smaller than
 * the layout (64*24, 64*8, 4096*4 and at most 64*96 words).
 * Diagnostic: wall-clock (100 MHz) phase stamps of the last PnP refine launch, [job < 64][24]:
 * entry, compaction, control points, MtM, eigen, betas, check, exit, then inside the eigen phase:
 * tridiagonal, Q accumulated, QR chase, eigenvectors, then [12 + 4w + j] inside the betas phase of
 * wave w: betas + Gauss-Newton, pc0 sum, M sum + Horn, error sum (zeros unless built with
 * RSC_REFINE_STAMPS=1). */
int rsc_diag_refine_phase_stamps(rsc_context* ctx, uint64_t* out, int cap);
/* Diagnostic: wall-clock (100 MHz) phase stamps of the last PnP hypothesis solve, [3][wg < 4096][8]:
 * [0] eigen stage per workgroup (entry, sample + MtM, tridiagonal, Q, chase + store), [1] betas stage
 * per wave (entry, L + rho, find_betas, Gauss-Newton, row loads, R and t, hand-off; [7] = the
 * approximation | 256 * group), [2] inside find_betas' Jacobi SVD per betas wave (QR preconditioner,
 * U formed, sweeps done, then k = the SVD's columns) (zeros unless built with RSC_SOLVE_STAMPS=1;
 * cap >= 98304). */
int rsc_diag_solve_phase_stamps(rsc_context* ctx, uint64_t* out, int cap);
/* Diagnostic wall-clock (100 MHz) stamps of mlpnp_quad_kernel's phases, [8192 workgroups][8]: entry,
 * sample, design + normal matrix, JacobiSVD, pose recovery, Gauss-Newton (zeros unless the library is
 * built with RSC_ML_STAMPS=1; tools/mlpnp_probe.py). cap >= 8192 * 8. */
int rsc_diag_mlpnp_phase_stamps(rsc_context* ctx, uint64_t* out, int cap);
/* Diagnostic: wall-clock (100 MHz) ticks of the last PoseOptimization launch (built with
 * RSC_POSE_PHASES=1), [frame < 64][8]: fused passes (ticks), number of passes + (their active edges
 * << 24), re-classification, whole kernel, the LM solves, wave 1's slab phases (to the errors, to the
 * terms) and its slab count.  cap >= 64 * 24 returns [frame][24]: columns 8..15 = the HW_ID register
 * of waves 0..7 (SIMD in bits 5:4, CU in 11:8), 16 / 17 = wave 0's folding ticks and fold count. */
int rsc_diag_poseopt_phases(rsc_context* ctx, uint64_t* out, int cap);
/* Diagnostic: wall-clock (100 MHz) ticks of the last OptimizeSim3 launch (built with RSC_SO_PHASES=1),
 * [pair < 64][8]: passes, pass count, perturbed-estimate builds, LM solves, wave 1's edge evaluation
 * and its slab count, wave 0's folds, whole kernel.  cap >= 64 * 8. */
int rsc_diag_sim3opt_phases(rsc_context* ctx, uint64_t* out, int cap);
/* Diagnostic: wall clock (100 MHz) of KeyFrameDatabase slots 0..4095 in the last count launch,
 * [slot][4] = entry, staged, counted, exit (zeros unless built with RSC_KFDB_STAMPS=1). */
int rsc_diag_kfdb_stamps(rsc_context* ctx, uint64_t* out, int cap);
/* Diagnostic: wall-clock (100 MHz) phase stamps of the last SearchByBoW launch, [pair < 64][96]. */
int rsc_diag_bow_phase_stamps(rsc_context* ctx, uint64_t* out, int cap);
/* Diagnostic (tests of history independence): waits for the context stream, then fills every staging
 * buffer of the batched calls with `byte` (0..255) over its whole capacity: the matcher arenas (the shared
 * projection / Fuse / triangulation / MapPoint-update / stereo arena, SearchBySim3's, SearchByBoW's, and the
 * work arena of every rsc_voc created on the context) and the PoseOptimization and OptimizeSim3 input and
 * result buffers, each with its pinned mirror.  Resident views, KeyFrame databases and solvers are not
 * touched.  Returns the number of bytes filled (device and pinned together), or a negative RSC_ERR_*. */
int64_t rsc_diag_fill_staging(rsc_context* ctx, int byte);

/* Device milliseconds per stage, summed over the launches of the last rsc_local_bundle_adjustment_many that ran
 * with timing on (HIP events around every launch): out[0..10] = linearise and build, vertex sums, iteration head,
 * point inverses, Schur complement, reduced solve, trial errors, back-substitution and update, trial tail, restore,
 * classification.  cap >= 11. */
int rsc_diag_localba_stages(rsc_context* ctx, double* out, int cap);

/* ---- glibc rand() helpers (Thirdparty/DBoW2/DUtils/Random.cpp:33-50) -------------------------- */
/* First n rand() outputs after srand(seed), produced with the device jump table (parity hook). */
int rsc_rand_stream(rsc_context* ctx, uint32_t seed, int n, int32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* RSC_H_ */
