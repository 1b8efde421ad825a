// rsc_host.h — librsc's private header: what rsc_api.cpp (backends, matchers, staging) and
// rsc_drivers.cpp (the entry points that only compose other ABI calls) share.  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <chrono>
#include <string>
#include "../../include/rsc.h"
#include "rsc_kernels.h"
#include "rsc_engine.h"
#include "rsc_sim3match.h"
#include "rsc_frameproj.h"
#include "rsc_lastproj.h"
#include "rsc_triang.h"

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
    ~rsc_pnp() {
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
    DevBuf<float> d_angle;   // mvKeysUn[i].angle (rsc_kfview_set_angles)
    bool has_angles = false;
    // rsc_kfview_set_triangulation: kp_raw | u_right | depth | cos_stereo on the device, the view as the pair
    // geometry reads it (device pointers), and the host copies the drivers and the argument checks read
    DevBuf<char> tri_mem;
    TriView tri;
    std::vector<float> h_uright;
    float Kinv[9];
    int n_levels = 0;
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
#pragma GCC visibility pop
