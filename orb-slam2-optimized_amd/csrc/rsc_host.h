// rsc_host.h — librsc's private header: what the translation units of the C ABI share (rsc_api.cpp: context,
// backends and solvers; rsc_optim.cpp, rsc_views.cpp, rsc_matchers.cpp, rsc_voc.cpp, rsc_kfdb.cpp by
// subsystem; rsc_drivers.cpp: the entry points that only compose other ABI calls): the opaque handle
// structs, RSC_HIP, the buffers, and the staging helpers of the batched calls.  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <chrono>
#include <memory>
#include <string>
#include "../../include/rsc.h"
#include "rsc_kernels.h"
#include "rsc_engine.h"
#include "rsc_sim3match.h"
#include "rsc_frameproj.h"
#include "rsc_lastproj.h"
#include "rsc_triang.h"
#include "rsc_kfdb.h"
#include "rsc_bowvoc.h"
#include "rsc_arena.h"
#include "rsc_viewimage.h"

using namespace rsc;
#pragma GCC visibility push(hidden)  // what this block declares stays out of the library's exported symbols
// the text behind rsc_status_string for the statuses that carry one (per thread)
extern thread_local std::string g_last_error;
// iterate_many on the solvers' own streams, whatever stream they are bound to
extern "C" int pnp_iterate_many_impl(rsc_pnp* const* solvers, int count, const int32_t* n_its, rsc_pnp_result* out,
                                     uint8_t* const* inliers);
extern "C" int sim3_iterate_many_impl(rsc_sim3* const* solvers, int count, const int32_t* n_its, rsc_sim3_result* out,
                                      uint8_t* const* inliers);

#define RSC_HIP(call)                                                                         \
    do {                                                                                      \
        hipError_t _e = (call);                                                               \
        if (_e != hipSuccess) {                                                               \
            g_last_error = std::string(#call) + ": " + hipGetErrorString(_e);                  \
            return RSC_ERR_HIP;                                                               \
        }                                                                                     \
    } while (0)

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    int ensure(size_t n) {
        if (n <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max(n, (size_t)64);
        hipError_t e = hipMalloc(&p, want * sizeof(T));
        if (e != hipSuccess) {
            g_last_error = std::string("hipMalloc: ") + hipGetErrorString(e);
            return RSC_ERR_OOM;
        }
        cap = want;
        return 0;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

template <typename T>
struct PinBuf {
    T* p = nullptr;
    size_t cap = 0;
    int ensure(size_t n) {
        if (n <= cap) return 0;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max(n, (size_t)64);
        hipError_t e = hipHostMalloc(&p, want * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) {
            g_last_error = std::string("hipHostMalloc: ") + hipGetErrorString(e);
            return RSC_ERR_OOM;
        }
        cap = want;
        return 0;
    }
    ~PinBuf() {
        if (p) (void)hipHostFree(p);
    }
};
#pragma GCC visibility pop

struct rsc_context {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    RngTable table;
    DevBuf<uint32_t> d_table;
    // speculation work buffers
    DevBuf<float> d_poses;
    DevBuf<int32_t> d_counts;
    DevBuf<uint64_t> d_masks;
    DevBuf<int32_t> d_samples;
    DevBuf<double> d_stage;  // quad path: per-hypothesis stage records between the two solve kernels
    DevBuf<double> d_berr;   // pnp_betas_kernel results for the scan: error per (approximation, record)
    DevBuf<float> d_bpose;   //   float pose [12] per (approximation, record)
    DevBuf<float> d_gather;  // gathered pose records (+ their indices)
    DevBuf<double> d_mposes; // MLPnP hypothesis poses, double[12] per record
    DevBuf<char> d_desc;
    PinBuf<char> h_desc;
    PinBuf<int32_t> h_counts;
    PinBuf<int32_t> h_qual;  // PnP rounds: 1 when a problem has a hypothesis reaching min_inliers
    // PnP work tables (eigen / betas / scan workgroups) on the device, uploaded when the round's shape
    // (pnp_tab_key) changes instead of with every round's descriptors
    DevBuf<char> d_pnp_tab;
    std::vector<int> pnp_tab_key;
    size_t pnp_tab_quad[3] = {0, 0, 0}, pnp_tab_solve[3] = {0, 0, 0}, pnp_tab_scan = 0;
    // The PnP round's DevPnP table, resident next to the work tables (the argument path of speculate()):
    // `pnp_probs_host` mirrors what d_pnp_probs holds, and a round whose table equals it uploads nothing.
    DevBuf<DevPnP> d_pnp_probs;
    std::vector<DevPnP> pnp_probs_host;
    // Round records as kernel arguments and the resident table (default), or every round's
    // descriptors through the blob; env RSC_ROUND_ARGS=0/1, rsc_context_set_round_args
    bool round_args = true;
    // diagnostic counters (rsc_diag_round_paths): rounds on the argument path, rounds on the blob path,
    // uploads of the resident problem table
    int64_t n_rounds_args = 0, n_rounds_blob = 0, n_probs_uploads = 0;
    // resident pnp_scan_kernel<PPT> workgroups of the device, [log2 PPT] (occupancy query x CU count,
    // read at the first round that needs it; 0: not read yet)
    int pnp_scan_capacity[6] = {0, 0, 0, 0, 0, 0};
    PinBuf<float> h_small;
    PinBuf<float> h_pick;  // Sim3 pick records of the last round, [solver][16]
    DevBuf<char> d_refine;
    DevBuf<RefineSelOut> d_selout;  // pnp_select_refine_kernel results of the last fused round
    PinBuf<RefineSelOut> h_selout;
    // PoseOptimization: packed inputs (problems | xw | uv), edge error scratch, results (outliers | poses)
    DevBuf<char> d_po_in;
    // OptimizeSim3: packed inputs (problems | e12 | e21 | uv), edge errors, results (out | keep)
    DevBuf<char> d_so_in;
    PinBuf<char> h_so_in;
    DevBuf<char> d_so_res;
    PinBuf<char> h_so_res;
    DevBuf<char> d_po_res;
    PinBuf<char> h_po_in;
    PinBuf<char> h_po_res;
    // LocalBundleAdjustment: problem | plan | estimates and work | results (device, pinned mirror)
    DevBuf<char> d_lba;
    PinBuf<char> h_lba;
    // device milliseconds per stage of the last rsc_local_bundle_adjustment_many with timing on
    // (rsc_diag_localba_stages)
    double lba_stage_ms[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // SearchBySim3: packed KeyFrames + pair table + scratch + outputs (device, pinned mirror)
    DevBuf<char> d_s3m;
    PinBuf<char> h_s3m;
    // where the last rsc_search_by_sim3_many left each pair's vnMatch1 / vnMatch2 in d_s3m
    // (rsc_diag_sim3match_directions); empty before the first call and after a failed one
    struct S3mPair { size_t o_m1, o_m2; int n1, n2; };
    std::vector<S3mPair> s3m_last;
    // SearchByBoW: pair table + output vectors + match counts (device, pinned mirror)
    DevBuf<char> d_bow;
    PinBuf<char> h_bow;
    // the vocabularies created on this context (rsc_diag_fill_staging reaches their work arenas)
    std::vector<struct rsc_voc*> vocs;
    // SearchByProjection (Frame, KeyFrame): problem table + flags + per-MapPoint scratch + outputs
    DevBuf<char> d_fp;
    PinBuf<char> h_fp;
    int mask_words = 0;  // per hypothesis, last speculation
    bool keep_samples = true;
    // timing
    bool timing = false;
    hipEvent_t ev[12] = {};  // [0..5] phase marks, [6+2g], [7+2g] eigen-stage kernel of sample-size group g
    double last_ms[6] = {0, 0, 0, 0, 0, 0};
    // host-side phase clock of the last PnP iterate_many (diagnostic): microseconds from entry to
    // [0] speculation inputs built, [1] kernels enqueued, [2] counts back (sync), [3] return
    double host_us[4] = {0, 0, 0, 0};
    bool direct_counts = true;  // env RSC_DIRECT_COUNTS=0 restores the HBM buffer + D2H copy
    // PnP scan: a hypothesis that cannot reach mRansacMinInliers after the first half of the thread's
    // point slices is not counted further (rsc_scanbound.h); env RSC_SCAN_BOUND=0/1,
    // rsc_context_set_scan_bound.  Off: every stored count is exact.
    bool scan_bound = true;
    // The last PnP round's scan launch, kept so that the parity hook (rsc_pnp_last_hypotheses) can
    // count that round again with the bound off: `pending` is set by a round that ran with the bound
    // on and cleared by the recount and, first thing, by the context's next speculation of any kind.
    // The tables, the betas results and the outputs the launch names stay valid until that next
    // speculation; the blob path's records do not (a Refine reuses the descriptor buffer), so their
    // bytes are kept.  The problem table names every solver's point buffers, which live only as long
    // as the solver: the round notes how many of the context's PnP solvers had been destroyed
    // (`pnp_destroyed`, which ~rsc_pnp counts up), and once that number has moved the hook reports an
    // error for that round (`lost`) instead of launching over freed memory.
    struct PnpScanLaunch {
        bool pending = false, use_args = false;
        bool lost = false;        // a PnP solver of the context was destroyed before a recount
        uint64_t destroyed = 0;   // *pnp_destroyed when the round was launched
        int ppt = 0, nwg = 0, mask_words = 0, total = 0;
        int32_t* counts = nullptr;      // where the round's counts went (pinned memory or HBM)
        int32_t* counts_dev = nullptr;  // the fused round's HBM copy, or null
        RoundArgs args;                 // argument path: the round's records
        std::vector<DevPnP> probs;      // blob path: the problem table and the records
        std::vector<LaunchProb> lps;
        void forget() { pending = lost = false; }  // a new round: nothing left to recount
    } pnp_scan_last;
    // PnP solvers of this context destroyed so far.  Shared with the solvers, which may outlive the
    // context (a binding's objects are collected in any order), so a solver never follows `ctx` to it.
    std::shared_ptr<std::atomic<uint64_t>> pnp_destroyed = std::make_shared<std::atomic<uint64_t>>(0);
    bool fused_refine = true;   // env RSC_FUSED_REFINE=0: the replay's Refine always as its own launch
    bool dma_upload = false;    // env RSC_DMA_UPLOAD=1: descriptors by hipMemcpyAsync instead of the copy kernel
    // eigen stage in the rows form when it has <= W workgroups (small, latency-bound launches such as
    // one relocalization event: 125 -> 99 us, profiles/r05/bench_latency_forms_ab_r5b.json); env
    // RSC_EIG_ROWS=W or rsc_context_set_eig_rows overrides (0: lane pairs always)
    int eig_rows_max_wgs = kEigRowsDefaultWgs;
    // hypotheses per betas wave for launches small enough for the rows-form eigen stage (a wave runs
    // the union of its hypotheses' data-dependent chains; env RSC_BETAS_HB)
    int betas_small_hb = kBetasHyps;
    // eigen stages beyond the rows form's range: split form (chase and Q rotations on two waves,
    // pnp_eig_split_kernel; config-2 eigen stage 119 -> 114 us, profiles/r05/split_ab_r5q.jsonl) or
    // the pair form (env RSC_EIG_SPLIT=0)
    bool eig_split = true;
    // host wait for a speculation round's results: spin on a completion flag in pinned host memory
    // (written by signal_kernel after the round) instead of hipStreamSynchronize's wake-up; env
    // RSC_SPIN_WAIT=0/1 (stream_wait)
    bool spin_wait = false;
    // OptimizeSim3's helper workgroups per pair (the cooperative form; -1: as many as fit one per CU,
    // at most 7; 0: one workgroup per pair)
    int so_helpers = -1;
    DevBuf<char> d_so_coop;  // the cooperative form's hand-off: polled words | publications | lists | chunks
    uint32_t* h_flag = nullptr;  // [0] stream_wait's sequence flag, [kFaultWord] the eigen stage's fault word
    uint32_t flag_seq = 0;
    std::chrono::steady_clock::time_point t_entry;
};

// The process-global glibc rand() stream the reference draws every sample from (Random.cpp:47-50,
// Q3): one position shared by all solvers bound to it, advanced by each iterate() call in call order.
struct rsc_stream {
    rsc_context* ctx = nullptr;
    RngStream st;
    int64_t position = 0;  // draws consumed since srand(seed)
};

struct rsc_pnp {
    rsc_context* ctx = nullptr;
    PnPState st;
    float4* d_pts = nullptr;
    float2* d_uv = nullptr;
    double* d_pws = nullptr;
    double* d_us = nullptr;
    double* d_als = nullptr;
    uint64_t* d_best = nullptr;
    uint64_t* d_refined = nullptr;
    int words = 0;
    int last_kind = 0;  // vbInliers of the last iterate(): 0 empty, 1 refined mask, 2 best mask
    // position in the last speculation of its context
    int spec_out0 = -1, spec_H = 0;
    rsc_stream* stream = nullptr;  // shared rand() stream (rsc_pnp_bind_stream) or null: own stream
    RngStream own_rng;             // the own stream, parked while bound (st.rng follows the shared one)
    std::vector<float> h_p2d, h_p3d;  // host copies (the gated events' PoseOptimization problems)
    std::shared_ptr<std::atomic<uint64_t>> ctx_destroyed;  // the context's pnp_destroyed
    ~rsc_pnp() {
        // the context's last round may name the buffers freed below: it cannot be counted again
        if (ctx_destroyed) ctx_destroyed->fetch_add(1, std::memory_order_relaxed);
        for (void* p : {(void*)d_pts, (void*)d_uv, (void*)d_pws, (void*)d_us, (void*)d_als, (void*)d_best,
                        (void*)d_refined})
            if (p) (void)hipFree(p);
    }
};

struct rsc_sim3 {
    rsc_context* ctx = nullptr;
    Sim3State st;
    // prepared arrays (host copies for rsc_sim3_prepared)
    std::vector<float> X1c, X2c, P1, P2;
    std::vector<uint64_t> e1, e2;
    float K1[4], K2[4];
    float4* d_x1 = nullptr;
    float4* d_x2 = nullptr;
    float4* d_pim = nullptr;
    int spec_out0 = -1, spec_H = 0;
    rsc_stream* stream = nullptr;
    RngStream own_rng;
    ~rsc_sim3() {
        for (void* p : {(void*)d_x1, (void*)d_x2, (void*)d_pim})
            if (p) (void)hipFree(p);
    }
};

struct rsc_kfview {
    rsc_context* ctx = nullptr;
    int n = 0;
    DevBuf<char> mem;  // DevSim3KF header | kp | octave | desc | grid | scales | MapPoints
    const DevSim3KF* hdr = nullptr;
    // host copies of what OptimizeSim3 reads (the gated loop events build its problem from them)
    std::vector<float> kp, mp_pos, inv_level_sigma2;
    std::vector<int32_t> octave;
    std::vector<uint8_t> mp_state;
    float R[9], t[3], K[4];
    float top_scale = 1.0f;  // mvScaleFactors[n_levels - 1] (the largest search radius is th times it)
    DevSim3KF dev;           // the header as uploaded (device pointers), for SearchByProjection's problem table
    // what the problem tables copy of an immutable view, built once: the KeyFrame of the loop-closing and Fuse
    // matchers (no rotation check: angle null) and of the Frame matcher (angle: rsc_kfview_set_angles)
    DevKfpKF kfp;
    DevProjKF proj;
    bool octaves_ok = false;  // every keypoint octave is in [0, dev.n_levels)
    DevBuf<float> d_angle;   // mvKeysUn[i].angle (rsc_kfview_set_angles)
    bool has_angles = false;
    // rsc_kfview_set_triangulation: kp_raw | u_right | depth | cos_stereo on the device, the view as the pair
    // geometry reads it (device pointers), and the host copies the drivers and the argument checks read
    DevBuf<char> tri_mem;
    TriView tri;
    std::vector<float> h_uright;
    float Kinv[9];
    bool has_triang = false;
};

struct rsc_frameview {
    rsc_context* ctx = nullptr;
    int n = 0;
    DevBuf<char> mem;  // DevProjFrame header | kp | octave | angle | desc | grid | scales
    const DevProjFrame* hdr = nullptr;
    // host copies of what the refinement chain's PoseOptimization problems read
    std::vector<float> kp, inv_level_sigma2;
    std::vector<int32_t> octave;
    float K[4];
    DevBuf<float> d_uright;  // mvuRight (rsc_frameview_set_stereo)
    std::vector<float> h_uright;  // its host copy (the motion-model driver's PoseOptimization problems)
    float mbf = 0.0f;
    bool has_stereo = false;
    float top_scale = 1.0f, gw_inv = 0.0f, gh_inv = 0.0f;  // the radius guard of the last-frame matcher
};

struct rsc_lastframe {
    rsc_context* ctx = nullptr;
    int n = 0;
    DevBuf<char> mem;  // octave | angle | mp_state | mp_pos | mp_desc | mp_has_obs
    DevLastFrame dev;  // device pointers
    // host copies: the argument check and the motion-model driver read them
    std::vector<int32_t> octave;
    std::vector<uint8_t> mp_state, mp_has_obs;
    std::vector<float> mp_pos;
};

struct rsc_mlpnp {
    rsc_context* ctx = nullptr;
    MLState st;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    float4* d_pts = nullptr;
    float2* d_uv = nullptr;
    float2* d_brg = nullptr;
    double* d_cov = nullptr;  // [N][9] when covariances were set
    bool use_cov = false;
    uint64_t* d_best = nullptr;
    int words = 0;
    int spec_out0 = -1, spec_H = 0;
    rsc_stream* stream = nullptr;
    RngStream own_rng;
    ~rsc_mlpnp() {
        for (void* p : {(void*)d_pts, (void*)d_uv, (void*)d_brg, (void*)d_cov, (void*)d_best})
            if (p) (void)hipFree(p);
    }
};

struct rsc_mpview {
    rsc_context* ctx = nullptr;
    int n = 0;
    DevBuf<char> mem;  // state | pos | normal | dmax | dmin | desc
    DevKfpPoints dev;  // device pointers
};

struct rsc_bow {
    rsc_context* ctx = nullptr;
    int n = 0;
    int n_nodes = 0;
    int n_feat = 0;
    DevBuf<char> mem;            // desc | desc_fv | angle | node_id | node_begin | feat
    size_t off_feat = 0;
    std::vector<uint32_t> feat;  // host copy of the FeatureVector entries (validity flags re-applied)
    DevBow hdr;                  // device pointers of this view (copied into every BowPair)
};

struct rsc_voc {
    rsc_context* ctx = nullptr;
    DevBuf<char> mem;        // desc | rec | orig | word | weight, all in breadth-first order
    DevVoc dev{};
    uint32_t n_words = 0;
    int L = 0;
    int lds_levels = 0;      // whole tree levels staged in LDS
    int min_leaf_depth = 0;  // the shallowest childless node
    int max_children = 0;
    DevBuf<char> d_work;     // job table | descriptors | per-view outputs
    PinBuf<char> h_work;
    hipEvent_t ev[3] = {};
    double last_ms[2] = {0, 0};
    ~rsc_voc() {
        for (auto e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

struct rsc_kfdb {
    rsc_context* ctx = nullptr;
    int cap = 0, max_words = 0;
    int hw = 0;  // slots in use: 1 + the highest slot ever added or referenced (queries sweep [0, hw))
    uint32_t vocab = 0;
    uint32_t next_seq = 1;
    std::vector<uint8_t> present;
    PinBuf<int32_t> covis_h, covis_n_h;  // host mirror of the covisibility table (pinned: the copy kernel reads it)
    DevBuf<uint32_t> ids, seq;
    DevBuf<double> vals;
    DevBuf<char> qbuf;  // the query BowVector: ids | vals (8-aligned), one upload per query
    DevBuf<int32_t> len, covis, covis_n, words, list, scored, best, tmp, counters, out;
    DevBuf<unsigned long long> query, key;
    DevBuf<float> score, sc, acc, tscore;
    DevBuf<uint8_t> conn;
    PinBuf<char> stage;  // query upload | candidates download
    void touch(int s) { hw = std::max(hw, s + 1); }
    DevKFDB dev() const {
        DevKFDB d;
        d.cap = hw;  // the kernels' sweep bound; the arrays are sized (and strided) by cap
        d.max_words = max_words;
        d.vocab = vocab;
        d.ids = ids.p;
        d.vals = vals.p;
        d.len = len.p;
        d.seq = seq.p;
        d.covis = covis.p;
        d.covis_n = covis_n.p;
        for (int t = 0; t < 2; ++t) {
            d.query[t] = query.p + (size_t)t * cap;
            d.words[t] = words.p + (size_t)t * cap;
            d.score[t] = score.p + (size_t)t * cap;
        }
        d.tscore = tscore.p;
        d.list = list.p;
        d.key = key.p;
        d.scored = scored.p;
        d.sc = sc.p;
        d.acc = acc.p;
        d.best = best.p;
        d.tmp = tmp.p;
        d.counters = counters.p;
        d.out = out.p;
        d.qids = reinterpret_cast<const uint32_t*>(qbuf.p);
        d.qvals = reinterpret_cast<const double*>(qbuf.p);  // set per query (after the ids)
        d.conn = conn.p;
        return d;
    }
};

// the validity flags of a FeatureVector's host copy (rsc_bow::feat), re-applied (rsc_views.cpp; exported like the next)
extern "C" void flag_invalid(std::vector<uint32_t>& feat, const uint8_t* valid);
// what rsc_search_by_projection_last_many refuses before any launch (an exported name since it exists)
extern "C" int last_check_args(rsc_context* C, rsc_frameview* const* frames, rsc_lastframe* const* lasts, int count,
                               float th);

#pragma GCC visibility push(hidden)
// rsc_search_for_triangulation_many with the driver's switch (not an exported symbol): speculative = 1 leaves the
// matches of a problem with den_zero in place (rsc_create_new_map_points_many's replay reads them when every
// den == 0 slot has been filled by an earlier neighbour)
extern "C" int tri_search_impl(rsc_context* C, const rsc_bow* const* bow1, rsc_kfview* const* kf1, const rsc_bow* const* bow2,
                    rsc_kfview* const* kf2, int count, const float* F12, const uint8_t* const* has_mp1,
                    const uint8_t* const* has_mp2, const int32_t* only_stereo, int check_orientation, int speculative,
                    int32_t* const* matches12, int32_t* nmatches, int32_t* den_zero, uint8_t* const* den_zero_slot);

constexpr int kFaultWord = 4;  // rsc_context::h_flag[4]: the split eigen stage's fault word

// The eigen stage's fault word (h_flag[kFaultWord], set by split_wait when a hand-off gives up):
// read after the round's wait, cleared, and returned as an error instead of the round's results.
inline int take_fault(rsc_context* C) {
    if (__atomic_load_n(C->h_flag + kFaultWord, __ATOMIC_ACQUIRE) == 0) return 0;
    __atomic_store_n(C->h_flag + kFaultWord, 0u, __ATOMIC_RELEASE);
    g_last_error = "a device hand-off wait timed out (split_wait: eigen stage chase / row wave, or a streamed "
                   "PoseOptimization pass, or an OptimizeSim3 chunk of the cooperative form); results discarded";
    return RSC_ERR_INTERNAL;
}

inline void timing_begin(rsc_context* C, int slot) {
    if (C->timing) (void)hipEventRecord(C->ev[slot], C->stream);
}

// The timed launch of the batched entry points: ev[3] and ev[4] around it, read by timing_read after
// the call's synchronise.
template <class Launch>
inline hipError_t timed_launch(rsc_context* C, Launch&& launch) {
    timing_begin(C, 3);
    const hipError_t e = launch();
    if (e == hipSuccess) timing_begin(C, 4);
    return e;
}

// rsc_context_last_kernel_timing: [2] the launch; with `mid` (the launch recorded ev[5] between its two
// kernels) also [0] setup kernel, [1] rounds kernel
inline void timing_read(rsc_context* C, bool mid = false) {
    if (!C->timing) return;
    float ms[3] = {0, 0, 0};
    (void)hipEventElapsedTime(&ms[2], C->ev[3], C->ev[4]);
    if (mid) {
        (void)hipEventElapsedTime(&ms[0], C->ev[3], C->ev[5]);
        (void)hipEventElapsedTime(&ms[1], C->ev[5], C->ev[4]);
    }
    for (int i = mid ? 0 : 2; i < 3; ++i) C->last_ms[i] = ms[i];
}

// One batched call over a staging arena (rsc_arena.h): fill(h, d) writes the problem table and the
// inputs into the pinned mirror h (d: the device addresses the table points at) and may refuse the call
// with a status; launch(d) enqueues the kernels.  `download` false: nothing comes back; `mid`: see
// timing_read.  Returns with the outputs in the mirror, [A.back, A.bytes).
template <class Fill, class Launch>
inline int arena_run(rsc_context* C, DevBuf<char>& dev, PinBuf<char>& pin, const Arena& A, Fill&& fill, Launch&& launch,
              bool download = true, bool mid = false) {
    RSC_HIP(hipSetDevice(C->device));
    if (int e = dev.ensure(A.bytes)) return e;
    if (int e = pin.ensure(A.bytes)) return e;
    // the previous call's copies into and out of the pinned mirror must be complete before it is rewritten
    RSC_HIP(hipStreamSynchronize(C->stream));
    char* h = pin.p;
    char* d = dev.p;
    if (int e = fill(h, d)) return e;
    RSC_HIP(hipMemcpyAsync(d, h, A.up, hipMemcpyHostToDevice, C->stream));
    RSC_HIP(timed_launch(C, [&] { return launch(d); }));
    if (download) RSC_HIP(hipMemcpyAsync(h + A.back, d + A.back, A.bytes - A.back, hipMemcpyDeviceToHost, C->stream));
    RSC_HIP(hipStreamSynchronize(C->stream));
    timing_read(C, mid);
    return 0;
}

// A view image (rsc_viewimage.h) into `mem` with one blocking copy; the pointer fields the builder named are
// bound to the allocation first (they must still be alive: members of the view, or locals of the builder).
// `wait`: work enqueued on the context stream may read what `mem` held before.  `hdr`: the view's header
// struct, copied into its piece `hdr_at` of the image once its pointers are bound.
template <class H = char>
inline int upload_image(rsc_context* C, DevBuf<char>& mem, ViewImage& img, bool wait = false,
                        Piece<H> hdr_at = {0}, const H* hdr = nullptr) {
    RSC_HIP(hipSetDevice(C->device));
    if (int e = mem.ensure(img.finish())) return e;
    img.bind(mem.p);
    if (hdr) std::memcpy(at(img.h.data(), hdr_at), hdr, sizeof(H));
    if (wait) RSC_HIP(hipStreamSynchronize(C->stream));
    RSC_HIP(hipMemcpy(mem.p, img.h.data(), img.h.size(), hipMemcpyHostToDevice));
    return 0;
}

// rsc_*_destroy of everything that lives on a context: work already enqueued on its stream may still read it
template <class V>
inline void destroy_on_stream(V* v) {
    if (!v) return;
    (void)hipStreamSynchronize(v->ctx->stream);
    delete v;
}

#pragma GCC visibility pop
