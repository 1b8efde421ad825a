// rsc_api.cpp — the core of the C ABI (include/rsc.h): context, rand() streams, the HIP backends of the RANSAC
// engine and the PnP / Sim3 / MLPnP solvers.  The other subsystems: rsc_optim.cpp, rsc_views.cpp,
// rsc_matchers.cpp, rsc_voc.cpp, rsc_kfdb.cpp, rsc_drivers.cpp.
//
// Data layout in HBM (per solver, resident for the solver's lifetime):
//   PnP : pts float4[N] = (X, Y, Z, sigma^2), uv float2[N], EPnP grow-only buffers
//         pws/us/als double[N][3|2|4], best/refined inlier bitsets uint64[ceil(N/64)].
//   Sim3: x1 float4[N] = (X1c, maxErr1), x2 float4[N] = (X2c, maxErr2), pim float4[N].
// Per context (reused across calls, grown on demand): the rand() jump table (2.1 MB), pose
// records float[H][12|24], counts int32[H], inlier bitsets uint64[H][W], launch descriptors.
#include <cstdio>
#include <cstdlib>
#include <array>
#include <cmath>
#include <cstring>
#include <memory>
#include "rsc_host.h"
#include "rsc_rounds.h"
#include "rsc_poseopt.h"  // launch_selftest_ldlt
#include "rsc_sim3opt.h"

using namespace rsc;

thread_local std::string g_last_error;

namespace {

// XCD-aware order of a workgroup table.  The dispatcher deals blocks round-robin over the 8 XCDs
// (blocks b and b + 8 share one L2; MI355X_MICROARCH.md "Workgroup dispatch, XCD placement"), and
// every workgroup of a problem reads that problem's correspondences (scan: all of them; solve
// stages: random samples of them).  Dealt in problem order, each problem's workgroups spread over
// all 8 XCDs and every L2 fetches the problem's points from HBM again (8x the input bytes, measured
// with FETCH_SIZE); here the problems are binned onto the 8 residues of b (greedy by workgroup
// count) so a problem's workgroups share one L2.  Placement only: results do not depend on it.
template <class T, class Prob>
void xcd_order(std::vector<T>& wgs, Prob prob_of) {
    // O(n), no allocation once the scratch has grown (this runs inside every speculation round)
    constexpr int X = 8;
    const size_t n = wgs.size();
    if (n <= (size_t)X) return;
    // thread_local scratch, addressed once (each access to a thread_local of a shared library is a
    // __tls_get_addr call)
    thread_local std::vector<T> src_tl;
    thread_local std::vector<size_t> rb_tl;  // run r = entries [rb[r], rb[r + 1]) of one problem
    thread_local std::vector<int> runs_tl[X];
    std::vector<T>& src = src_tl;
    std::vector<size_t>& rb = rb_tl;
    std::vector<int>* runs = runs_tl;
    src.assign(wgs.begin(), wgs.end());
    rb.clear();
    for (size_t i = 0; i < n; ++i)
        if (i == 0 || prob_of(src[i]) != prob_of(src[i - 1])) rb.push_back(i);
    rb.push_back(n);
    size_t left[X] = {};
    for (int x = 0; x < X; ++x) runs[x].clear();
    for (size_t r = 0; r + 1 < rb.size(); ++r) {  // each problem to the least loaded residue
        int best = 0;
        for (int x = 1; x < X; ++x) if (left[x] < left[best]) best = x;
        runs[best].push_back((int)r);
        left[best] += rb[r + 1] - rb[r];
    }
    size_t cr[X] = {}, cp[X] = {};
    for (size_t b = 0; b < n; ++b) {
        int x = (int)(b % X);
        if (!left[x])  // this residue's problems are dealt: take from the one with most left
            for (int y = 0; y < X; ++y) if (left[y] > left[x]) x = y;
        const int r = runs[x][cr[x]];
        wgs[b] = src[rb[r] + cp[x]];
        if (++cp[x] == rb[r + 1] - rb[r]) { cp[x] = 0; ++cr[x]; }
        --left[x];
    }
}

// Hypotheses per scan workgroup: enough workgroups for ~8 waves per SIMD (256 CUs x 4 SIMDs,
// 4 waves per workgroup) without going below 8 hypotheses per point load.
// RSC_SCAN_WGS overrides the workgroup target (A/B of the chunk size).
int scan_chunk(int total_hyps) {
    static const int target = [] {
        const char* m = std::getenv("RSC_SCAN_WGS");
        return m ? std::max(1, std::atoi(m)) : 2048;
    }();
    int hc = 32;
    while (hc > 8 && (total_hyps + hc - 1) / hc < target) hc >>= 1;
    return hc;
}
// The PnP rounds size their scan from the device's capacity (pnp_scan_partition) unless the
// variable is set: then they too use scan_chunk's power-of-two chunks with a remainder chunk.
bool scan_wgs_overridden() {
    static const bool set = std::getenv("RSC_SCAN_WGS") != nullptr;
    return set;
}

// Scan workgroups of a PnP round: chunks[i] even chunks for problem i's H[i] hypotheses (sizes
// differ by at most one, even_chunk below).  `capacity` is what the device holds at once
// (pnp_scan_kernel<PPT>'s workgroups per CU x CUs) and `batch` the most hypotheses a workgroup takes
// (kScanMaxChunk: lane j of a wave stands for the chunk's hypothesis j).
//   * The round gets k x capacity workgroups, dealt to the problems in proportion to their
//     hypotheses, with the smallest k whose chunks stay within `batch`: whole rounds of residency, so
//     no CU idles through a part-filled last round, and each workgroup's head (table -> launch
//     record -> problem -> points) is paid for as many hypotheses as a full device allows
//     (config 2: 1,792 x 10 or 11 instead of 2,432 x 8 or 4).
//   * Never fewer than kScanMinChunk hypotheses per point load, so a round too small to fill the
//     device (the single event) keeps ceil(H / 8) workgroups per problem: it is latency-bound and
//     wants the width.
// Placement only: the counts, masks and poses do not depend on it.
constexpr int kScanMinChunk = 8;
constexpr int kScanMaxChunk = 64;
void pnp_scan_partition(const int* H, int count, int capacity, int batch, std::vector<int>& chunks) {
    chunks.assign((size_t)count, 1);
    int64_t total = 0;
    for (int i = 0; i < count; ++i) total += H[i];
    if (total <= 0) return;
    capacity = std::max(capacity, 1);
    batch = std::max(batch, kScanMinChunk);
    const int kmax = (int)(total / capacity) + 1;  // k x capacity > total: every share is at its upper bound
    for (int k = 1; k <= kmax; ++k) {
        bool fits = true;
        for (int i = 0; i < count; ++i) {
            const int h = std::max(H[i], 1);
            const int lo = (h + batch - 1) / batch, hi = (h + kScanMinChunk - 1) / kScanMinChunk;
            const int64_t share = (int64_t)k * capacity * h / total;  // floor: the sum stays <= k x capacity
            if (share < lo && k < kmax) { fits = false; break; }
            chunks[i] = (int)std::min<int64_t>(std::max<int64_t>(share, lo), hi);
        }
        if (fits) break;
    }
}
// Chunk c of n even chunks of H hypotheses: [h0, h0 + len), the first H % n chunks one longer.
inline void even_chunk(int H, int n, int c, int& h0, int& len) {
    const int q = H / n, r = H % n;
    h0 = c * q + std::min(c, r);
    len = q + (c < r ? 1 : 0);
}

int ppt_for(int n) {
    int need = (n + 255) / 256;
    int p = 1;
    while (p < need) p <<= 1;
    return p;
}

}  // namespace

namespace {

// ------------------------------------------------------------------------------------------------
// Launch-descriptor packing: one pinned blob -> one H2D copy per launch round.
// ------------------------------------------------------------------------------------------------
// Descriptor staging of one round.  The byte vector is a per-thread scratch that keeps its capacity
// across rounds (one Blob is alive at a time per thread), so a round allocates nothing here.
struct Blob {
    std::vector<char>& bytes;
    Blob() : bytes(scratch()) {
        // one Blob per thread at a time: a nested one would truncate the open one's descriptors
        if (in_use()) {
            std::fprintf(stderr, "rsc: nested launch-descriptor Blob on one thread\n");
            std::abort();
        }
        in_use() = true;
        bytes.clear();
    }
    ~Blob() { in_use() = false; }
    Blob(const Blob&) = delete;
    Blob& operator=(const Blob&) = delete;
    static std::vector<char>& scratch() {
        thread_local std::vector<char> v;
        return v;
    }
    static bool& in_use() {
        thread_local bool f = false;
        return f;
    }
    size_t add(const void* p, size_t n) {
        size_t off = (bytes.size() + 15) & ~(size_t)15;
        bytes.resize(off + n);
        std::memcpy(bytes.data() + off, p, n);
        return off;
    }
};

// n bytes through the pinned staging to dst (device memory with room for n rounded up to 16), in
// stream order with the launches that read them
int upload_bytes(rsc_context* C, const void* src, size_t n, void* dst) {
    const size_t n16 = (n + 15) / 16;
    if (int e = C->h_desc.ensure(n16 * 16)) return e;
    // the previous round's upload must be finished before the pinned staging is overwritten
    RSC_HIP(hipStreamSynchronize(C->stream));
    std::memcpy(C->h_desc.p, src, n);
    // a copy kernel on the context stream, not hipMemcpyAsync: the DMA engine's start-up and its
    // completion hand-off to the first kernel cost ~15 us per round (rocprofv3 copy + kernel trace)
    if (C->dma_upload)
        RSC_HIP(hipMemcpyAsync(dst, C->h_desc.p, n, hipMemcpyHostToDevice, C->stream));
    else
        RSC_HIP(launch_upload16(C->h_desc.p, dst, n16, C->stream));
    return 0;
}

int upload_blob(rsc_context* C, const Blob& b) {
    if (int e = C->d_desc.ensure((b.bytes.size() + 15) / 16 * 16)) return e;
    return upload_bytes(C, b.bytes.data(), b.bytes.size(), C->d_desc.p);
}

// Inlier counts of a speculation round: written by the scan kernel straight into pinned host
// memory (one fewer copy and no blit launch before the host replay), or into HBM + a D2H copy.
int counts_target(rsc_context* C, int total, int32_t** dst) {
    C->pnp_scan_last.forget();  // the count buffer gets a new round (the speculate()s did this on entry)
    if (int e = C->h_counts.ensure((size_t)total)) return e;
    if (C->direct_counts) {
        *dst = C->h_counts.p;
        return 0;
    }
    if (int e = C->d_counts.ensure((size_t)total)) return e;
    *dst = C->d_counts.p;
    return 0;
}

// Wait until everything enqueued on the context stream has finished.  With spin_wait a one-lane
// kernel stores a sequence number into pinned host memory behind the round and the host polls it
// (results written to pinned memory by the round's kernels are visible once the flag is: stream
// order + the flag's system-scope release); after 20 ms of polling it falls back to
// hipStreamSynchronize, which also reports a failed kernel.
int stream_wait(rsc_context* C) {
    if (!C->spin_wait || !C->h_flag || C->timing) {  // the timing pass reads events: a full sync
        RSC_HIP(hipStreamSynchronize(C->stream));
        return 0;
    }
    const uint32_t want = ++C->flag_seq;
    RSC_HIP(launch_signal(C->h_flag, want, C->stream));
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned it = 1;; ++it) {
        if (__atomic_load_n(C->h_flag, __ATOMIC_ACQUIRE) == want) return 0;
        __builtin_ia32_pause();
        if ((it & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
    }
    RSC_HIP(hipStreamSynchronize(C->stream));
    return 0;
}

void host_mark(rsc_context* C, int k) {
    C->host_us[k] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - C->t_entry).count();
}

// ------------------------------------------------------------------------------------------------
// PnP backend
// ------------------------------------------------------------------------------------------------
struct HipPnPBackend : PnPBackend {
    rsc_context* C;
    std::vector<rsc_pnp*> solvers;  // index = state slot in the current call
    int fused_count = 0;  // > 0: the last speculation ran pnp_select_refine_kernel over this many slots
    explicit HipPnPBackend(rsc_context* c) : C(c) {}
    rsc_pnp* of(PnPState* s) {
        for (auto* p : solvers)
            if (&p->st == s) return p;
        return nullptr;
    }
    DevPnP dev_of(rsc_pnp* p) {
        DevPnP d;
        std::memset(&d, 0, sizeof(d));  // padding too: the resident table is compared by its bytes
        d.pts = p->d_pts;
        d.uv = p->d_uv;
        d.n = p->st.N;
        d.fx = p->st.fx; d.fy = p->st.fy; d.cx = p->st.cx; d.cy = p->st.cy;
        d.th2 = p->st.th2;
        d.rows = p->st.max_rows;
        d.pws = p->d_pws; d.us = p->d_us; d.als = p->d_als;
        return d;
    }

    int speculate(PnPState* const* S, int count, const int* H, std::vector<std::vector<int32_t>>& counts) override {
        // before anything the last round's scan reads (tables, problem table, buffers) can change
        C->pnp_scan_last.forget();
        // group by min_set (template parameter of the solve kernel)
        int total = 0, maxN = 1;
        // per-thread scratch that keeps its capacity across rounds (no allocation per round)
        thread_local std::vector<DevPnP> probs_tl;
        thread_local std::vector<LaunchProb> lps_tl;
        std::vector<DevPnP>& probs = probs_tl;
        std::vector<LaunchProb>& lps = lps_tl;
        probs.resize(count);
        lps.resize(count);
        // The argument path: the round's records travel in the kernels' argument blocks and the windows
        // follow from the seeds on the device, which holds only while every solver still stands on its
        // seed window (a moved window or a shared stream's position exists as 31 words alone).
        bool use_args = C->round_args && count <= kRoundArgsCap;
        thread_local std::vector<rsc_pnp*> ps_tl;  // of(S[i]) is a search: once per solver and round
        std::vector<rsc_pnp*>& ps = ps_tl;
        ps.resize(count);
        for (int i = 0; i < count; ++i) {
            ps[i] = of(S[i]);
            if (!ps[i]) return RSC_ERR_ARG;
            if (S[i]->mRansacMinSet < 4 || S[i]->mRansacMinSet > 6) {
                g_last_error = "min_set outside the supported range [4,6]";
                return RSC_ERR_UNSUPPORTED;
            }
            S[i]->rng.ensure(C->table, H[i] * S[i]->mRansacMinSet);
            use_args = use_args && S[i]->rng.on_seed_window;
        }
        thread_local RoundArgs ra_tl;
        RoundArgs& ra = ra_tl;
        for (int i = 0; i < count; ++i) {
            rsc_pnp* p = ps[i];
            probs[i] = dev_of(p);
            LaunchProb& lp = lps[i];
            lp.prob = i;
            lp.H = H[i];
            lp.out0 = total;
            lp.g0 = S[i]->rng.g;
            lp.min_inliers = S[i]->mRansacMinInliers;  // only such hypotheses' masks are ever read
            if (use_args)
                ra.r[i] = RoundRec{i, H[i], total, lp.g0, lp.min_inliers, S[i]->rng.seed_value};
            else
                std::memcpy(lp.window, S[i]->rng.words(), sizeof(lp.window));  // works the words out if need be
            p->spec_out0 = total;
            p->spec_H = H[i];
            total += H[i];
            maxN = std::max(maxN, S[i]->N);
        }
        const int ppt = ppt_for(maxN);
        if (ppt > 32) {
            g_last_error = "more than 8192 correspondences per problem";
            return RSC_ERR_UNSUPPORTED;
        }
        const int mw = ppt * 4;
        C->mask_words = mw;
        // the replay's first Refine of every solver runs on the device with the round (small rounds)
        fused_count = 0;
        const bool fused = C->fused_refine && total <= kFusedRefineMaxHyps;
        thread_local std::vector<RefineSel> sels_tl;
        std::vector<RefineSel>& sels = sels_tl;
        sels.resize(fused ? count : 0);
        for (int i = 0; fused && i < count; ++i) {
            rsc_pnp* p = ps[i];
            RefineSel& r = sels[i];
            r.prob = i;
            r.out0 = lps[i].out0;
            r.H = H[i];
            r.min_inliers = S[i]->mRansacMinInliers;
            r.best0 = S[i]->mnBestInliers;
            r.rows0 = S[i]->max_rows;
            r.best = p->d_best;
            r.refined = p->d_refined;
            r.words = p->words;
        }
        // work tables
        thread_local std::vector<int2> solve_wgs_tl[3], quad_wgs_tl[3];
        thread_local std::vector<int4> scan_wgs_tl;
        std::vector<int2>* solve_wgs = solve_wgs_tl;
        std::vector<int2>* quad_wgs = quad_wgs_tl;
        std::vector<int4>& scan_wgs = scan_wgs_tl;
        // scan workgroups: even chunks sized from the device's capacity (pnp_scan_partition), or
        // RSC_SCAN_WGS's chunks of HC hypotheses with a remainder chunk
        const int HC = scan_wgs_overridden() ? scan_chunk(total) : 0;
        int scan_cap = 0;
        if (!HC) {
            int lg = 0;
            while ((1 << lg) < ppt) ++lg;
            if (!C->pnp_scan_capacity[lg]) {
                int per_cu = 0, cus = 0;
                RSC_HIP(pnp_scan_occupancy(ppt, &per_cu));
                RSC_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, C->device));
                if (per_cu <= 0 || cus <= 0) {
                    g_last_error = "pnp_scan_kernel: no resident workgroup (occupancy query)";
                    return RSC_ERR_INTERNAL;
                }
                C->pnp_scan_capacity[lg] = per_cu * cus;
            }
            scan_cap = C->pnp_scan_capacity[lg];
        }
        // The chunk limit is the kernel's, 64 for every PPT.  (Before the two-segment kernel the counts
        // were flushed in batches of 512 / PPT for PPT 16 and 32 and the chunks were capped there;
        // the partition differs only for rounds beyond 512 / PPT x capacity hypotheses.)
        const int scan_batch = kScanMaxChunk;
        const int hb = (total <= kEigHyps * C->eig_rows_max_wgs) ? C->betas_small_hb : kBetasHyps;

        // The tables depend only on the round's shape (count, sample size and H per problem, the scan's
        // chunking): a round with the shape of the previous one on this thread reuses them (building
        // and XCD-ordering ~2.5k entries costs ~10 us of host time per config-2 round).
        thread_local std::vector<int> shape_tl;
        std::vector<int>& shape = shape_tl;
        thread_local std::vector<int> key_tl;
        std::vector<int>& key = key_tl;
        key.clear();
        key.push_back(count);
        key.push_back(HC);
        key.push_back(scan_cap);
        key.push_back(hb);
        for (int i = 0; i < count; ++i) {
            key.push_back(S[i]->mRansacMinSet);
            key.push_back(H[i]);
        }
        if (key != shape) {
            for (int g = 0; g < 3; ++g) { solve_wgs[g].clear(); quad_wgs[g].clear(); }
            scan_wgs.clear();
            thread_local std::vector<int> chunks_tl;
            std::vector<int>& chunks = chunks_tl;
            if (!HC) pnp_scan_partition(H, count, scan_cap, scan_batch, chunks);
            for (int i = 0; i < count; ++i) {
                const int g = S[i]->mRansacMinSet - 4;
                for (int h0 = 0; h0 < H[i]; h0 += hb) solve_wgs[g].push_back(make_int2(i, h0));
                for (int h0 = 0; h0 < H[i]; h0 += kEigHyps) quad_wgs[g].push_back(make_int2(i, h0));
                if (HC) {
                    for (int h0 = 0; h0 < H[i]; h0 += HC)
                        scan_wgs.push_back(make_int4(i, h0, std::min(HC, H[i] - h0), 0));
                } else if (H[i] > 0) {
                    for (int c = 0; c < chunks[i]; ++c) {
                        int h0, len;
                        even_chunk(H[i], chunks[i], c, h0, len);
                        scan_wgs.push_back(make_int4(i, h0, len, 0));
                    }
                }
            }
            for (int g = 0; g < 3; ++g) {
                xcd_order(solve_wgs[g], [](const int2& w) { return w.x; });
                xcd_order(quad_wgs[g], [](const int2& w) { return w.x; });
            }
            xcd_order(scan_wgs, [](const int4& w) { return w.x; });
            shape.assign(key.begin(), key.end());
        }
        // The work tables (≈50 KB for config 2) live in the context's d_pnp_tab while the round's shape
        // repeats; only the per-round descriptors (problems, launch records, selections) travel in the
        // blob (the host copies and the upload kernel's PCIe reads shrink accordingly).
        if (C->pnp_tab_key != key || !C->d_pnp_tab.p) {
            std::vector<char> tab;
            auto put = [&](const void* p, size_t n) {
                const size_t o = tab.size();
                tab.resize(o + ((n + 15) & ~(size_t)15));
                if (n) std::memcpy(tab.data() + o, p, n);
                return o;
            };
            for (int g = 0; g < 3; ++g) C->pnp_tab_solve[g] = put(solve_wgs[g].data(), solve_wgs[g].size() * sizeof(int2));
            for (int g = 0; g < 3; ++g) C->pnp_tab_quad[g] = put(quad_wgs[g].data(), quad_wgs[g].size() * sizeof(int2));
            C->pnp_tab_scan = put(scan_wgs.data(), scan_wgs.size() * sizeof(int4));
            C->pnp_tab_key.clear();  // invalid until the copy below has landed
            if (int e = C->d_pnp_tab.ensure(std::max(tab.size(), (size_t)16))) return e;
            // the previous round (the tables' last reader) has finished: every round ends synchronized
            RSC_HIP(hipMemcpyAsync(C->d_pnp_tab.p, tab.data(), tab.size(), hipMemcpyHostToDevice, C->stream));
            RSC_HIP(hipStreamSynchronize(C->stream));
            C->pnp_tab_key = key;
        }
        const DevPnP* dprobs = nullptr;
        const LaunchProb* dlps = nullptr;
        const RefineSel* dsels = nullptr;
        thread_local SelArgs sa_tl;
        SelArgs& sa = sa_tl;
        if (use_args) {
            // The problem table changes only when SetRansacParameters, a Refine (rows, buffers) or the
            // solver set changes it: it stays on the device, and a round whose table equals the mirror
            // uploads nothing.  The previous round (the table's last reader) has finished.
            std::vector<DevPnP>& mirror = C->pnp_probs_host;
            const size_t pbytes = probs.size() * sizeof(DevPnP);
            if (mirror.size() != probs.size() || !C->d_pnp_probs.p ||
                std::memcmp(mirror.data(), probs.data(), pbytes) != 0) {
                mirror.clear();  // invalid until the upload below is enqueued
                if (int e = C->d_pnp_probs.ensure(probs.size() + 1)) return e;  // the copy moves whole 16-B words
                if (int e = upload_bytes(C, probs.data(), pbytes, C->d_pnp_probs.p)) return e;
                mirror.assign(probs.begin(), probs.end());
                ++C->n_probs_uploads;
            }
            dprobs = C->d_pnp_probs.p;
            for (int i = 0; fused && i < count; ++i) sa.s[i] = sels[i];
            ++C->n_rounds_args;
        } else {
            Blob b;
            const size_t o_probs = b.add(probs.data(), probs.size() * sizeof(DevPnP));
            const size_t o_lps = b.add(lps.data(), lps.size() * sizeof(LaunchProb));
            const size_t o_sel = fused ? b.add(sels.data(), sels.size() * sizeof(RefineSel)) : 0;
            if (int e = upload_blob(C, b)) return e;
            const char* base = C->d_desc.p;
            dprobs = reinterpret_cast<const DevPnP*>(base + o_probs);
            dlps = reinterpret_cast<const LaunchProb*>(base + o_lps);
            dsels = reinterpret_cast<const RefineSel*>(base + o_sel);
            ++C->n_rounds_blob;
        }
        const RoundArgs* dargs = use_args ? &ra : nullptr;
        const char* tab = C->d_pnp_tab.p;
        if (int e = C->d_poses.ensure((size_t)total * 12)) return e;
        int32_t* cnt_dst = nullptr;
        if (int e = counts_target(C, total, &cnt_dst)) return e;
        if (int e = C->h_qual.ensure((size_t)count)) return e;
        std::memset(C->h_qual.p, 0, (size_t)count * sizeof(int32_t));  // the previous round has finished
        int32_t* cnt_dev = nullptr;  // HBM copy of the counts for the device-side selection
        if (fused) {
            if (C->direct_counts) {
                if (int e = C->d_counts.ensure((size_t)total)) return e;
                cnt_dev = C->d_counts.p;
            }
            if (int e = C->d_selout.ensure((size_t)count)) return e;
            if (int e = C->h_selout.ensure((size_t)count)) return e;
        }
        // of a round's mask rows only the one of each scan chunk's first qualifying hypothesis is
        // written (pnp_scan_kernel's storing steps); every other row holds what earlier rounds left
        if (int e = C->d_masks.ensure((size_t)total * mw)) return e;
        if (int e = C->d_samples.ensure((size_t)total * 8)) return e;
        if (int e = C->d_stage.ensure((size_t)total * kStageDoubles)) return e;
        if (int e = C->d_berr.ensure((size_t)total * 3)) return e;
        if (int e = C->d_bpose.ensure((size_t)total * 36)) return e;
        const BetasScratch bs{C->d_berr.p, C->d_bpose.p, (size_t)total};
        host_mark(C, 0);
        timing_begin(C, 0);
        bool first_group = true;
        for (int g = 0; g < 3; ++g) {
            if (solve_wgs[g].empty()) continue;
            // the first group's eigen stage starts at ev[0]: no extra event in the queue
            hipEvent_t eb = (C->timing && !first_group) ? C->ev[6 + 2 * g] : nullptr;
            RSC_HIP(launch_pnp_solve_split(4 + g, (int)quad_wgs[g].size(),
                                          reinterpret_cast<const int2*>(tab + C->pnp_tab_quad[g]), (int)solve_wgs[g].size(),
                                          reinterpret_cast<const int2*>(tab + C->pnp_tab_solve[g]), dprobs, dlps,
                                          dargs, C->d_table.p, C->d_stage.p, C->d_samples.p, bs, C->stream,
                                          eb, C->timing ? C->ev[7 + 2 * g] : nullptr,
                                          (int)quad_wgs[g].size() <= C->eig_rows_max_wgs, C->eig_split,
                                          C->h_flag + kFaultWord, hb));
            first_group = false;
        }
        timing_begin(C, 1);
        RSC_HIP(launch_pnp_scan(ppt, (int)scan_wgs.size(), dprobs, dlps, dargs,
                                reinterpret_cast<const int4*>(tab + C->pnp_tab_scan),
                                bs, C->d_poses.p, cnt_dst, cnt_dev, C->d_masks.p, mw, C->h_qual.p, C->scan_bound,
                                C->stream));
        timing_begin(C, 2);
        if (C->scan_bound) {
            // what rsc_pnp_last_hypotheses needs to count this round again in full (pnp_recount)
            rsc_context::PnpScanLaunch& L = C->pnp_scan_last;
            L.use_args = use_args;
            L.ppt = ppt;
            L.nwg = (int)scan_wgs.size();
            L.mask_words = mw;
            L.total = total;
            L.counts = cnt_dst;
            L.counts_dev = cnt_dev;
            if (use_args) {
                std::memcpy(L.args.r, ra.r, sizeof(RoundRec) * (size_t)count);
            } else {
                L.probs.assign(probs.begin(), probs.end());
                L.lps.assign(lps.begin(), lps.end());
            }
            L.destroyed = C->pnp_destroyed->load(std::memory_order_relaxed);
            L.pending = true;
        }
        if (fused) {
            timing_begin(C, 3);
            RSC_HIP(launch_pnp_select_refine(count, dprobs, dsels, use_args ? &sa : nullptr,
                                             cnt_dev ? cnt_dev : cnt_dst, C->d_masks.p, mw, C->d_poses.p,
                                             C->d_selout.p, C->h_flag + kFaultWord, C->stream));
            timing_begin(C, 4);
            RSC_HIP(hipMemcpyAsync(C->h_selout.p, C->d_selout.p, sizeof(RefineSelOut) * count, hipMemcpyDeviceToHost,
                                   C->stream));
        }
        if (!C->direct_counts)
            RSC_HIP(hipMemcpyAsync(C->h_counts.p, C->d_counts.p, (size_t)total * 4, hipMemcpyDeviceToHost, C->stream));
        host_mark(C, 1);
        if (int e = stream_wait(C)) return e;
        host_mark(C, 2);
        if (int e = take_fault(C)) return e;
        if (C->timing) {
            float a = 0, s = 0;
            (void)hipEventElapsedTime(&a, C->ev[0], C->ev[1]);
            (void)hipEventElapsedTime(&s, C->ev[1], C->ev[2]);
            C->last_ms[0] += a;
            C->last_ms[1] += s;
            C->last_ms[3] += 1;
            C->last_ms[4] += total;
            bool first = true;
            for (int g = 0; g < 3; ++g) {
                if (solve_wgs[g].empty()) continue;
                float e = 0;
                (void)hipEventElapsedTime(&e, first ? C->ev[0] : C->ev[6 + 2 * g], C->ev[7 + 2 * g]);
                C->last_ms[5] += e;
                first = false;
            }
            if (fused) {
                float r = 0;
                (void)hipEventElapsedTime(&r, C->ev[3], C->ev[4]);
                C->last_ms[2] += r;
            }
        }
        // a problem none of whose hypotheses reaches min_inliers hands back no counts: the replay only
        // advances its counters (the GPU-written counts are not read back through the host caches)
        counts.resize(count);  // keeps the inner vectors' capacity
        for (int i = 0; i < count; ++i) {
            if (C->h_qual.p[i])
                counts[i].assign(C->h_counts.p + lps[i].out0, C->h_counts.p + lps[i].out0 + H[i]);
            else
                counts[i].clear();
        }
        if (fused) fused_count = count;
        return 0;
    }

    int refine(PnPState* const* S, int count, const int* spec_j, const int* pause_k, const int* adopt_k,
               const int* rows_after, int* rcount, float (*rpose)[12]) override {
        if (fused_count > 0) {
            // the device ran exactly these Refines with the round (pnp_select_refine_kernel applies the
            // replay's rules to the same counts); anything else is an engine bug, reported loudly
            const int nslots = fused_count;
            fused_count = 0;
            // every slot: the device refined exactly the listed slots (o.k >= 0) and no other one
            // (an unlisted device Refine would have overwritten that solver's best / refined masks)
            thread_local std::vector<int> listed_tl;
            std::vector<int>& listed = listed_tl;
            listed.assign((size_t)nslots, -1);
            for (int i = 0; i < count; ++i) {
                if (spec_j[i] < 0 || spec_j[i] >= nslots || listed[spec_j[i]] >= 0) {
                    g_last_error = "device-side Refine selection disagrees with the host replay";
                    return RSC_ERR_INTERNAL;
                }
                listed[spec_j[i]] = i;
            }
            for (int j = 0; j < nslots; ++j) {
                const RefineSelOut& o = C->h_selout.p[j];
                const int i = listed[j];
                const bool agree = i < 0 ? o.k < 0
                                         : o.k == pause_k[i] && (o.adopt != 0) == (adopt_k[i] >= 0) &&
                                               o.rows_after == rows_after[i];
                if (!agree) {
                    g_last_error = "device-side Refine selection disagrees with the host replay";
                    return RSC_ERR_INTERNAL;
                }
            }
            for (int i = 0; i < count; ++i) {
                const RefineSelOut& o = C->h_selout.p[spec_j[i]];
                rcount[i] = o.count;
                std::memcpy(rpose[i], o.pose, 48);
                if (adopt_k[i] >= 0) pose12_to_T(o.best_pose, S[i]->mBestTcw);
            }
            return 0;
        }
        if (count == 0) return 0;
        std::vector<DevPnP> probs(count);
        std::vector<RefineJob> jobs(count);
        // out: refined poses [count][12] | counts [count] | adopted best poses [count][12]
        if (int e = C->d_refine.ensure((size_t)count * 100)) return e;
        float* d_out_pose = reinterpret_cast<float*>(C->d_refine.p);
        int32_t* d_out_cnt = reinterpret_cast<int32_t*>(C->d_refine.p + (size_t)count * 48);
        float* d_out_best = reinterpret_cast<float*>(C->d_refine.p + (size_t)count * 52);
        for (int i = 0; i < count; ++i) {
            rsc_pnp* p = of(S[i]);
            probs[i] = dev_of(p);
            jobs[i].prob = i;
            jobs[i].rows_after = rows_after[i];
            (void)spec_j;
            if (adopt_k[i] >= 0) {
                const size_t rec = (size_t)(p->spec_out0 + adopt_k[i]);
                jobs[i].best_mask = C->d_masks.p + rec * C->mask_words;
                jobs[i].adopt_mask = p->d_best;
                jobs[i].adopt_pose = C->d_poses.p + rec * 12;
            } else {
                jobs[i].best_mask = p->d_best;
                jobs[i].adopt_mask = nullptr;
                jobs[i].adopt_pose = nullptr;
            }
            jobs[i].out_best_pose = d_out_best + 12 * i;
            jobs[i].out_pose = d_out_pose + 12 * i;
            jobs[i].out_count = d_out_cnt + i;
            jobs[i].out_mask = p->d_refined;
            jobs[i].out_words = p->words;
        }
        Blob b;
        const size_t o_probs = b.add(probs.data(), probs.size() * sizeof(DevPnP));
        const size_t o_jobs = b.add(jobs.data(), jobs.size() * sizeof(RefineJob));
        if (int e = upload_blob(C, b)) return e;
        timing_begin(C, 3);
        RSC_HIP(launch_pnp_refine(count, reinterpret_cast<const DevPnP*>(C->d_desc.p + o_probs),
                                  reinterpret_cast<const RefineJob*>(C->d_desc.p + o_jobs), C->h_flag + kFaultWord,
                                  C->stream));
        timing_begin(C, 4);
        if (int e = C->h_small.ensure((size_t)count * 25)) return e;
        RSC_HIP(hipMemcpyAsync(C->h_small.p, C->d_refine.p, (size_t)count * 100, hipMemcpyDeviceToHost, C->stream));
        RSC_HIP(hipStreamSynchronize(C->stream));
        if (int e = take_fault(C)) return e;
        if (C->timing) {
            float r = 0;
            (void)hipEventElapsedTime(&r, C->ev[3], C->ev[4]);
            C->last_ms[2] += r;
        }
        const int32_t* hc = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(C->h_small.p) + (size_t)count * 48);
        for (int i = 0; i < count; ++i) {
            rcount[i] = hc[i];
            std::memcpy(rpose[i], C->h_small.p + 12 * i, 48);
            if (adopt_k[i] >= 0) pose12_to_T(C->h_small.p + 13 * count + 12 * i, S[i]->mBestTcw);
        }
        return 0;
    }

    int fetch_mask(PnPState* const* S, int count, const int* kind, uint8_t* const* out) override {
        std::vector<std::vector<uint64_t>> words(count);
        for (int i = 0; i < count; ++i) {
            rsc_pnp* p = of(S[i]);
            words[i].resize(p->words);
            RSC_HIP(hipMemcpyAsync(words[i].data(), kind[i] == 1 ? p->d_refined : p->d_best, (size_t)p->words * 8,
                                   hipMemcpyDeviceToHost, C->stream));
        }
        RSC_HIP(hipStreamSynchronize(C->stream));
        for (int i = 0; i < count; ++i) {
            const PnPState& s = *S[i];
            std::memset(out[i], 0, s.N_points);
            for (int j = 0; j < s.N; ++j)
                if ((words[i][j >> 6] >> (j & 63)) & 1ull) out[i][s.kp_index[j]] = 1;
        }
        return 0;
    }
};

// ------------------------------------------------------------------------------------------------
// Sim3 backend
// ------------------------------------------------------------------------------------------------
struct HipSim3Backend : Sim3Backend {
    rsc_context* C;
    std::vector<rsc_sim3*> solvers;  // slot j of the last speculation
    bool pick_valid = false;  // C->h_pick holds this round's sim3_pick_kernel records
    explicit HipSim3Backend(rsc_context* c) : C(c) {}
    rsc_sim3* of(Sim3State* s, const std::vector<rsc_sim3*>& all) {
        for (auto* p : all)
            if (&p->st == s) return p;
        return nullptr;
    }
    std::vector<rsc_sim3*> all;

    int speculate(Sim3State* const* S, int count, const int* H, std::vector<std::vector<int32_t>>& counts) override {
        C->pnp_scan_last.forget();  // this round reuses the PnP round's pose, mask and count buffers
        pick_valid = false;  // set again only once this round's pick kernel is enqueued
        int total = 0, maxN = 1;
        // per-thread scratch that keeps its capacity across rounds (no allocation per round)
        thread_local std::vector<DevSim3> probs_tl;
        thread_local std::vector<LaunchProb> lps_tl;
        std::vector<DevSim3>& probs = probs_tl;
        std::vector<LaunchProb>& lps = lps_tl;
        probs.resize(count);
        lps.resize(count);
        solvers.assign(count, nullptr);
        for (int i = 0; i < count; ++i) {
            rsc_sim3* p = of(S[i], all);
            if (!p) return RSC_ERR_ARG;
            solvers[i] = p;
            S[i]->rng.ensure(C->table, H[i] * 3);
            DevSim3& d = probs[i];
            d.x1 = p->d_x1; d.x2 = p->d_x2; d.pim = p->d_pim; d.n = S[i]->N;
            std::memcpy(d.K1, p->K1, sizeof(d.K1));
            std::memcpy(d.K2, p->K2, sizeof(d.K2));
            LaunchProb& lp = lps[i];
            lp.prob = i; lp.H = H[i]; lp.out0 = total; lp.g0 = S[i]->rng.g;
            lp.min_inliers = S[i]->mRansacMinInliers;  // the pick kernel's return rule
            lp.best0 = S[i]->mnBestInliers;
            std::memcpy(lp.window, S[i]->rng.words(), sizeof(lp.window));
            p->spec_out0 = total;
            p->spec_H = H[i];
            total += H[i];
            maxN = std::max(maxN, S[i]->N);
        }
        const int ppt = ppt_for(maxN);
        if (ppt > 32) {
            g_last_error = "more than 8192 correspondences per problem";
            return RSC_ERR_UNSUPPORTED;
        }
        const int mw = ppt * 4;
        C->mask_words = mw;
        thread_local std::vector<int2> solve_wgs_tl;
        thread_local std::vector<int4> scan_wgs_tl;
        thread_local std::vector<int> shape_tl, key_tl;
        std::vector<int2>& solve_wgs = solve_wgs_tl;
        std::vector<int4>& scan_wgs = scan_wgs_tl;
        std::vector<int>& shape = shape_tl;
        std::vector<int>& key = key_tl;
        const int HC = 32;
        key.assign(H, H + count);  // the tables depend on the per-solver H only (as the PnP tables)
        if (key != shape) {
            solve_wgs.clear();
            scan_wgs.clear();
            for (int i = 0; i < count; ++i) {
                for (int h0 = 0; h0 < H[i]; h0 += 64) solve_wgs.push_back(make_int2(i, h0));
                for (int h0 = 0; h0 < H[i]; h0 += HC) scan_wgs.push_back(make_int4(i, h0, std::min(HC, H[i] - h0), 0));
            }
            xcd_order(solve_wgs, [](const int2& w) { return w.x; });
            xcd_order(scan_wgs, [](const int4& w) { return w.x; });
            shape.assign(key.begin(), key.end());
        }
        Blob b;
        const size_t o_probs = b.add(probs.data(), probs.size() * sizeof(DevSim3));
        const size_t o_lps = b.add(lps.data(), lps.size() * sizeof(LaunchProb));
        const size_t o_solve = b.add(solve_wgs.data(), solve_wgs.size() * sizeof(int2));
        const size_t o_scan = b.add(scan_wgs.data(), scan_wgs.size() * sizeof(int4));
        if (int e = upload_blob(C, b)) return e;
        if (int e = C->d_poses.ensure((size_t)total * 24)) return e;
        // the kept pose comes back with the counts (sim3_pick_kernel) when every solver's round
        // fits the pick kernel's LDS
        bool use_pick = true;
        for (int i = 0; i < count; ++i) use_pick = use_pick && H[i] <= kPickMaxH;
        int32_t* cnt_dst = nullptr;
        if (int e = counts_target(C, total, &cnt_dst)) return e;
        if (use_pick) {
            if (int e = C->d_counts.ensure((size_t)total)) return e;
            if (int e = C->h_pick.ensure((size_t)count * 16)) return e;
        }
        if (int e = C->d_masks.ensure((size_t)total * mw)) return e;
        if (C->keep_samples)
            if (int e = C->d_samples.ensure((size_t)total * 8)) return e;
        const char* base = C->d_desc.p;
        const DevSim3* dprobs = reinterpret_cast<const DevSim3*>(base + o_probs);
        const LaunchProb* dlps = reinterpret_cast<const LaunchProb*>(base + o_lps);
        timing_begin(C, 0);
        RSC_HIP(launch_sim3_solve((int)solve_wgs.size(), dprobs, dlps, reinterpret_cast<const int2*>(base + o_solve),
                                  C->d_table.p, C->d_poses.p, C->keep_samples ? C->d_samples.p : nullptr, C->stream));
        timing_begin(C, 1);
        int32_t* cnt_dev = (use_pick && C->direct_counts) ? C->d_counts.p : nullptr;  // else cnt_dst is HBM
        RSC_HIP(launch_sim3_scan(ppt, (int)scan_wgs.size(), dprobs, dlps, reinterpret_cast<const int4*>(base + o_scan),
                                 C->d_poses.p, cnt_dst, cnt_dev, C->d_masks.p, mw, C->stream));
        timing_begin(C, 2);
        if (use_pick) {
            RSC_HIP(launch_sim3_pick(count, dlps, C->d_counts.p, C->d_poses.p, C->h_pick.p, C->stream));
            pick_valid = true;
        }
        if (!C->direct_counts)
            RSC_HIP(hipMemcpyAsync(C->h_counts.p, C->d_counts.p, (size_t)total * 4, hipMemcpyDeviceToHost, C->stream));
        if (int e = stream_wait(C)) return e;
        if (C->timing) {
            float a = 0, s = 0;
            (void)hipEventElapsedTime(&a, C->ev[0], C->ev[1]);
            (void)hipEventElapsedTime(&s, C->ev[1], C->ev[2]);
            C->last_ms[0] += a;
            C->last_ms[1] += s;
            C->last_ms[3] += 1;
            C->last_ms[4] += total;
        }
        counts.resize(count);  // keeps the inner vectors' capacity
        for (int i = 0; i < count; ++i)
            counts[i].assign(C->h_counts.p + lps[i].out0, C->h_counts.p + lps[i].out0 + H[i]);
        return 0;
    }

    int fetch_poses(const int* j, const int* k, int n, float (*pose12)[12]) override {
        // the poses the pick kernel brought back with the counts, when the replay kept the same
        // hypotheses (it always does: both apply Sim3Solver.cpp:155-166 to the same counts)
        bool from_pick = pick_valid;
        for (int q = 0; q < n && from_pick; ++q)
            from_pick = reinterpret_cast<const int32_t*>(C->h_pick.p + (size_t)j[q] * 16)[0] == k[q];
        if (from_pick) {
            for (int q = 0; q < n; ++q) std::memcpy(pose12[q], C->h_pick.p + (size_t)j[q] * 16 + 1, 48);
            return 0;
        }
        // record indices -> one gather kernel -> one D2H copy
        if (int e = C->h_small.ensure((size_t)n * 13)) return e;
        int32_t* hidx = reinterpret_cast<int32_t*>(C->h_small.p + (size_t)n * 12);
        for (int q = 0; q < n; ++q) hidx[q] = solvers[j[q]]->spec_out0 + k[q];
        if (int e = C->d_gather.ensure((size_t)n * 13)) return e;
        int32_t* didx = reinterpret_cast<int32_t*>(C->d_gather.p + (size_t)n * 12);
        RSC_HIP(hipMemcpyAsync(didx, hidx, (size_t)n * 4, hipMemcpyHostToDevice, C->stream));
        RSC_HIP(launch_gather_records(C->d_poses.p, 24, 12, didx, n, C->d_gather.p, C->stream));
        RSC_HIP(hipMemcpyAsync(C->h_small.p, C->d_gather.p, (size_t)n * 48, hipMemcpyDeviceToHost, C->stream));
        RSC_HIP(hipStreamSynchronize(C->stream));
        std::memcpy(pose12, C->h_small.p, (size_t)n * 48);
        return 0;
    }

    int fetch_mask(const int* wj, const int* wk, Sim3State* const* S, int count, uint8_t* const* out) override {
        std::vector<std::vector<uint64_t>> words(count);
        for (int q = 0; q < count; ++q) {
            rsc_sim3* p = solvers[wj[q]];
            const int nw = (S[q]->N + 63) / 64;
            words[q].resize(nw);
            RSC_HIP(hipMemcpyAsync(words[q].data(), C->d_masks.p + (size_t)(p->spec_out0 + wk[q]) * C->mask_words,
                                   (size_t)nw * 8, hipMemcpyDeviceToHost, C->stream));
        }
        RSC_HIP(hipStreamSynchronize(C->stream));
        for (int q = 0; q < count; ++q) {
            const Sim3State& s = *S[q];
            std::memset(out[q], 0, s.mN1);
            for (int j = 0; j < s.N; ++j)
                if ((words[q][j >> 6] >> (j & 63)) & 1ull) out[q][s.indices1[j]] = 1;
        }
        return 0;
    }
};

// ------------------------------------------------------------------------------------------------
// MLPnP backend
// ------------------------------------------------------------------------------------------------
struct HipMLBackend : MLBackend {
    rsc_context* C;
    std::vector<rsc_mlpnp*> all;      // solvers of the call
    std::vector<rsc_mlpnp*> solvers;  // slot j of the last speculation
    explicit HipMLBackend(rsc_context* c) : C(c) {}
    rsc_mlpnp* of(MLState* s) {
        for (auto* p : all)
            if (&p->st == s) return p;
        return nullptr;
    }

    int speculate(MLState* const* S, int count, const int* H, std::vector<std::vector<int32_t>>& counts) override {
        C->pnp_scan_last.forget();  // this round reuses the PnP round's mask and count buffers
        int total = 0, maxN = 1;
        std::vector<DevML> probs(count);
        std::vector<LaunchProb> lps(count);
        solvers.assign(count, nullptr);
        for (int i = 0; i < count; ++i) {
            rsc_mlpnp* p = of(S[i]);
            if (!p) return RSC_ERR_ARG;
            solvers[i] = p;
            S[i]->rng.ensure(C->table, H[i] * S[i]->mRansacMinSet);
            DevML& d = probs[i];
            d.pts = p->d_pts; d.uv = p->d_uv; d.brg = p->d_brg; d.cov = p->use_cov ? p->d_cov : nullptr; d.n = S[i]->N;
            d.fx = p->fx; d.fy = p->fy; d.cx = p->cx; d.cy = p->cy; d.th2 = S[i]->th2;
            LaunchProb& lp = lps[i];
            lp.prob = i;
            lp.H = H[i];
            lp.out0 = total;
            lp.g0 = S[i]->rng.g;
            std::memcpy(lp.window, S[i]->rng.words(), sizeof(lp.window));
            lp.min_inliers = S[i]->mRansacMinInliers;  // only such hypotheses' masks are ever read
            p->spec_out0 = total;
            p->spec_H = H[i];
            total += H[i];
            maxN = std::max(maxN, S[i]->N);
        }
        const int ppt = ppt_for(maxN);
        if (ppt > 32) {
            g_last_error = "more than 8192 correspondences per problem";
            return RSC_ERR_UNSUPPORTED;
        }
        const int mw = ppt * 4;
        C->mask_words = mw;
        std::vector<std::vector<int2>> solve_wgs(6);  // by (min_set, covariances given)
        std::vector<int4> scan_wgs;
        const int HC = 32;
        for (int i = 0; i < count; ++i) {
            const int g = 2 * (S[i]->mRansacMinSet - 6) + (probs[i].cov ? 1 : 0);
            for (int h0 = 0; h0 < H[i]; h0 += kMlQuadHyps) solve_wgs[g].push_back(make_int2(i, h0));
            for (int h0 = 0; h0 < H[i]; h0 += HC) scan_wgs.push_back(make_int4(i, h0, std::min(HC, H[i] - h0), 0));
        }
        for (auto& t : solve_wgs) xcd_order(t, [](const int2& w) { return w.x; });
        xcd_order(scan_wgs, [](const int4& w) { return w.x; });
        Blob b;
        const size_t o_probs = b.add(probs.data(), probs.size() * sizeof(DevML));
        const size_t o_lps = b.add(lps.data(), lps.size() * sizeof(LaunchProb));
        size_t o_solve[6];
        for (int g = 0; g < 6; ++g) o_solve[g] = b.add(solve_wgs[g].data(), solve_wgs[g].size() * sizeof(int2));
        const size_t o_scan = b.add(scan_wgs.data(), scan_wgs.size() * sizeof(int4));
        if (int e = upload_blob(C, b)) return e;
        if (int e = C->d_mposes.ensure((size_t)total * 12)) return e;
        int32_t* cnt_dst = nullptr;
        if (int e = counts_target(C, total, &cnt_dst)) return e;
        if (int e = C->d_masks.ensure((size_t)total * mw)) return e;
        if (C->keep_samples)
            if (int e = C->d_samples.ensure((size_t)total * 8)) return e;
        const char* base = C->d_desc.p;
        const DevML* dprobs = reinterpret_cast<const DevML*>(base + o_probs);
        const LaunchProb* dlps = reinterpret_cast<const LaunchProb*>(base + o_lps);
        timing_begin(C, 0);
        for (int g = 0; g < 6; ++g) {
            if (solve_wgs[g].empty()) continue;
            RSC_HIP(launch_mlpnp_solve(6 + g / 2, (g & 1) != 0, (int)solve_wgs[g].size(), dprobs, dlps,
                                       reinterpret_cast<const int2*>(base + o_solve[g]), C->d_table.p, C->d_mposes.p,
                                       C->keep_samples ? C->d_samples.p : nullptr, C->stream));
        }
        timing_begin(C, 1);
        RSC_HIP(launch_mlpnp_scan(ppt, (int)scan_wgs.size(), dprobs, dlps, reinterpret_cast<const int4*>(base + o_scan),
                                  C->d_mposes.p, cnt_dst, C->d_masks.p, mw, C->stream));
        timing_begin(C, 2);
        if (!C->direct_counts)
            RSC_HIP(hipMemcpyAsync(C->h_counts.p, C->d_counts.p, (size_t)total * 4, hipMemcpyDeviceToHost, C->stream));
        if (int e = stream_wait(C)) return e;
        if (C->timing) {
            float a = 0, sc = 0;
            (void)hipEventElapsedTime(&a, C->ev[0], C->ev[1]);
            (void)hipEventElapsedTime(&sc, C->ev[1], C->ev[2]);
            C->last_ms[0] += a;
            C->last_ms[1] += sc;
            C->last_ms[3] += 1;
            C->last_ms[4] += total;
        }
        counts.resize(count);  // keeps the inner vectors' capacity
        for (int i = 0; i < count; ++i)
            counts[i].assign(C->h_counts.p + lps[i].out0, C->h_counts.p + lps[i].out0 + H[i]);
        return 0;
    }

    int pose_of(int j, int k, float* pose12) {
        // R, t double -> float (cv::Mat::convertTo(CV_32F), MLPnPsolver.cpp:152-153)
        double d[12];
        RSC_HIP(hipMemcpyAsync(d, C->d_mposes.p + (size_t)(solvers[j]->spec_out0 + k) * 12, 96, hipMemcpyDeviceToHost,
                               C->stream));
        RSC_HIP(hipStreamSynchronize(C->stream));
        for (int q = 0; q < 12; ++q) pose12[q] = (float)d[q];
        return 0;
    }

    int adopt_best(MLState* s, int j, int k) override {
        rsc_mlpnp* p = solvers[j];
        const size_t rec = (size_t)(p->spec_out0 + k);
        RSC_HIP(hipMemcpyAsync(p->d_best, C->d_masks.p + rec * C->mask_words, (size_t)p->words * 8,
                               hipMemcpyDeviceToDevice, C->stream));
        float pose[12];
        if (int e = pose_of(j, k, pose)) return e;
        pose12_to_T(pose, s->mBestTcw);
        return 0;
    }

    int fetch_poses(const int* j, const int* k, int n, float (*pose12)[12]) override {
        for (int q = 0; q < n; ++q)
            if (int e = pose_of(j[q], k[q], pose12[q])) return e;
        return 0;
    }

    int fetch_mask(MLState* const* S, int count, const int* kind, const int* j, const int* k,
                   uint8_t* const* out) override {
        std::vector<std::vector<uint64_t>> words(count);
        for (int q = 0; q < count; ++q) {
            rsc_mlpnp* p = of(S[q]);
            words[q].resize(p->words);
            const uint64_t* src = (kind[q] == 2) ? p->d_best
                                                 : C->d_masks.p + (size_t)(solvers[j[q]]->spec_out0 + k[q]) * C->mask_words;
            RSC_HIP(hipMemcpyAsync(words[q].data(), src, (size_t)p->words * 8, hipMemcpyDeviceToHost, C->stream));
        }
        RSC_HIP(hipStreamSynchronize(C->stream));
        for (int q = 0; q < count; ++q) {
            const MLState& s = *S[q];
            std::memset(out[q], 0, s.N_points);
            for (int i = 0; i < s.N; ++i)
                if ((words[q][i >> 6] >> (i & 63)) & 1ull) out[q][s.kp_index[i]] = 1;
        }
        return 0;
    }
};

void to_result(const PnPResult& r, rsc_pnp_result* o) {
    o->ok = r.ok;
    o->no_more = r.no_more;
    o->n_inliers = r.n_inliers;
    o->iterations = r.iterations;
    if (r.ok) std::memcpy(o->T, r.T, sizeof(o->T));
}

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================
// srand(seed) on a solver's own stream: while the solver is bound, that stream is the parked one
template <class Solver>
static void reset_solver(Solver* s, uint32_t seed) {
    s->st.reset(seed);
    if (s->stream) s->own_rng = s->st.rng;
}

// rsc_*_bind_stream: binding parks the own stream, unbinding resumes it where it stopped (a bound
// call overwrites st.rng with the shared stream's position); rebinding keeps the parked one
template <class Solver>
static int bind_stream(Solver* s, rsc_stream* stream) {
    if (!s || (stream && stream->ctx != s->ctx)) return RSC_ERR_ARG;
    if (!s->stream && stream) s->own_rng = s->st.rng;
    if (s->stream && !stream) s->st.rng = s->own_rng;
    s->stream = stream;
    return RSC_OK;
}

// iterate() calls of solvers bound to a shared stream draw in call order, so a bound solver's call
// starts where the previous call ended: the calls run one at a time in list order.
template <class Solver, class Impl, class Out>
static int bound_iterate_many(Solver* const* solvers, int count, const int32_t* n_its, Out* out,
                              uint8_t* const* inliers, Impl impl) {
    for (int i = 0; i < count; ++i) {
        Solver* s = solvers[i];
        if (!s) return RSC_ERR_ARG;
        const int it0 = s->st.mnIterations;
        if (s->stream) s->st.rng = s->stream->st;
        uint8_t* const m[1] = {inliers ? inliers[i] : nullptr};
        if (int st = impl(&solvers[i], 1, n_its + i, out + i, m)) return st;
        if (s->stream) {
            s->stream->st = s->st.rng;
            s->stream->position += (int64_t)(s->st.mnIterations - it0) * draws_per_hypothesis(s->st);
        }
    }
    return RSC_OK;
}

// The context's last PnP round counted again with the scan bound off, once: the same tables, records,
// betas results and outputs as the round's own scan launch (all valid until the context's next
// speculation), so the counts become exact and qual, the first qualifiers' masks and the poses are
// written again with the values the replay already used.
namespace {
int pnp_recount(rsc_context* C) {
    rsc_context::PnpScanLaunch& L = C->pnp_scan_last;
    // The problem table names every solver's point buffers: after a PnP solver of the context has been
    // destroyed the launch could read freed memory, so the round stays as it is.
    if (L.pending && L.destroyed != C->pnp_destroyed->load(std::memory_order_relaxed)) {
        L.pending = false;
        L.lost = true;
    }
    if (L.lost) {
        g_last_error = "a PnP solver of the context was destroyed after its last round: that round's full counts "
                       "are gone (rsc_pnp_last_counts_raw returns what the round left)";
        return RSC_ERR_UNSUPPORTED;
    }
    if (!L.pending) return 0;
    RSC_HIP(hipSetDevice(C->device));
    const DevPnP* dprobs = C->d_pnp_probs.p;
    const LaunchProb* dlps = nullptr;
    if (!L.use_args) {
        Blob b;
        const size_t o_probs = b.add(L.probs.data(), L.probs.size() * sizeof(DevPnP));
        const size_t o_lps = b.add(L.lps.data(), L.lps.size() * sizeof(LaunchProb));
        if (int e = upload_blob(C, b)) return e;
        dprobs = reinterpret_cast<const DevPnP*>(C->d_desc.p + o_probs);
        dlps = reinterpret_cast<const LaunchProb*>(C->d_desc.p + o_lps);
    }
    const BetasScratch bs{C->d_berr.p, C->d_bpose.p, (size_t)L.total};
    RSC_HIP(launch_pnp_scan(L.ppt, L.nwg, dprobs, dlps, L.use_args ? &L.args : nullptr,
                            reinterpret_cast<const int4*>(C->d_pnp_tab.p + C->pnp_tab_scan), bs, C->d_poses.p, L.counts,
                            L.counts_dev, C->d_masks.p, L.mask_words, C->h_qual.p, false, C->stream));
    if (L.counts != C->h_counts.p)
        RSC_HIP(hipMemcpyAsync(C->h_counts.p, L.counts, (size_t)L.total * 4, hipMemcpyDeviceToHost, C->stream));
    RSC_HIP(hipStreamSynchronize(C->stream));
    L.pending = false;
    return 0;
}
}  // namespace

extern "C" {

int rsc_version(void) { return 1; }

const char* rsc_status_string(int status) {
    switch (status) {
        case RSC_OK: return "ok";
        case RSC_ERR_ARG: return "invalid argument";
        case RSC_ERR_HIP: return g_last_error.empty() ? "HIP error" : g_last_error.c_str();
        case RSC_ERR_OOM: return g_last_error.empty() ? "out of device memory" : g_last_error.c_str();
        case RSC_ERR_UNSUPPORTED: return g_last_error.empty() ? "unsupported" : g_last_error.c_str();
        case RSC_ERR_NODEVICE: return "no HIP device";
        case RSC_ERR_INTERNAL: return g_last_error.empty() ? "internal error" : g_last_error.c_str();
        default: return "unknown status";
    }
}

int rsc_context_create(int device, rsc_context** out) {
    if (!out) return RSC_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RSC_ERR_NODEVICE;
    if (device < 0 || device >= ndev) return RSC_ERR_ARG;
    RSC_HIP(hipSetDevice(device));
    std::unique_ptr<rsc_context> C(new rsc_context());
    C->device = device;
    RSC_HIP(hipStreamCreateWithFlags(&C->stream, hipStreamNonBlocking));
    C->own_stream = true;
    if (const char* m = std::getenv("RSC_DIRECT_COUNTS")) C->direct_counts = std::strcmp(m, "0") != 0;
    if (const char* m = std::getenv("RSC_SCAN_BOUND")) C->scan_bound = std::strcmp(m, "0") != 0;
    if (const char* m = std::getenv("RSC_FUSED_REFINE")) C->fused_refine = std::strcmp(m, "0") != 0;
    if (const char* m = std::getenv("RSC_DMA_UPLOAD")) C->dma_upload = std::strcmp(m, "0") != 0;
    if (const char* m = std::getenv("RSC_EIG_ROWS")) C->eig_rows_max_wgs = std::max(0, std::atoi(m));
    if (const char* m = std::getenv("RSC_EIG_SPLIT")) C->eig_split = std::strcmp(m, "0") != 0;
    if (const char* m = std::getenv("RSC_BETAS_HB")) C->betas_small_hb = std::min(kBetasHyps, std::max(1, std::atoi(m)));
    if (const char* m = std::getenv("RSC_SPIN_WAIT")) C->spin_wait = std::strcmp(m, "0") != 0;
    if (const char* m = std::getenv("RSC_ROUND_ARGS")) C->round_args = std::strcmp(m, "0") != 0;
    if (const char* m = std::getenv("RSC_SO_HELPERS")) C->so_helpers = std::max(-1, std::atoi(m));
    {
        void* f = nullptr;
        RSC_HIP(hipHostMalloc(&f, 64, hipHostMallocCoherent));
        C->h_flag = static_cast<uint32_t*>(f);
        std::memset(C->h_flag, 0, 64);
    }
    C->table.build();
    if (int e = C->d_table.ensure(C->table.T.size())) return e;
    RSC_HIP(hipMemcpy(C->d_table.p, C->table.T.data(), C->table.T.size() * 4, hipMemcpyHostToDevice));
    for (auto& e : C->ev) RSC_HIP(hipEventCreate(&e));
    *out = C.release();
    return RSC_OK;
}

void rsc_context_destroy(rsc_context* C) {
    if (!C) return;
    (void)hipSetDevice(C->device);
    if (C->stream) (void)hipStreamSynchronize(C->stream);
    if (C->h_flag) (void)hipHostFree(C->h_flag);
    for (auto& e : C->ev)
        if (e) (void)hipEventDestroy(e);
    if (C->own_stream && C->stream) (void)hipStreamDestroy(C->stream);
    delete C;
}

int rsc_context_set_stream(rsc_context* C, void* s) {
    if (!C) return RSC_ERR_ARG;
    RSC_HIP(hipStreamSynchronize(C->stream));
    if (C->own_stream) (void)hipStreamDestroy(C->stream);
    C->stream = reinterpret_cast<hipStream_t>(s);
    C->own_stream = false;
    return RSC_OK;
}

int rsc_context_synchronize(rsc_context* C) {
    if (!C) return RSC_ERR_ARG;
    RSC_HIP(hipStreamSynchronize(C->stream));
    return RSC_OK;
}

int rsc_context_enable_timing(rsc_context* C, int enable) {
    if (!C) return RSC_ERR_ARG;
    C->timing = enable != 0;
    return RSC_OK;
}

int rsc_context_set_eig_rows(rsc_context* C, int max_workgroups) {
    if (!C || max_workgroups < 0) return RSC_ERR_ARG;
    C->eig_rows_max_wgs = max_workgroups;
    return RSC_OK;
}

int rsc_context_set_eig_split(rsc_context* C, int on) {
    if (!C) return RSC_ERR_ARG;
    C->eig_split = on != 0;
    return RSC_OK;
}

int rsc_context_set_round_args(rsc_context* C, int on) {
    if (!C) return RSC_ERR_ARG;
    C->round_args = on != 0;
    return RSC_OK;
}

int rsc_context_set_scan_bound(rsc_context* C, int on) {
    if (!C) return RSC_ERR_ARG;
    C->scan_bound = on != 0;
    return RSC_OK;
}

int rsc_diag_round_paths(rsc_context* C, int64_t out[3]) {
    if (!C || !out) return RSC_ERR_ARG;
    out[0] = C->n_rounds_args;
    out[1] = C->n_rounds_blob;
    out[2] = C->n_probs_uploads;
    return RSC_OK;
}

int64_t rsc_diag_fill_staging(rsc_context* C, int byte) {
    if (!C || byte < 0 || byte > 255) return RSC_ERR_ARG;
    RSC_HIP(hipSetDevice(C->device));
    RSC_HIP(hipStreamSynchronize(C->stream));
    int64_t total = 0;
    auto fill = [&](DevBuf<char>& d, PinBuf<char>& h) -> hipError_t {
        if (h.p) std::memset(h.p, byte, h.cap);
        total += (int64_t)h.cap + (int64_t)d.cap;
        return d.p ? hipMemsetAsync(d.p, byte, d.cap, C->stream) : hipSuccess;
    };
    RSC_HIP(fill(C->d_fp, C->h_fp));
    RSC_HIP(fill(C->d_s3m, C->h_s3m));
    RSC_HIP(fill(C->d_bow, C->h_bow));
    for (rsc_voc* V : C->vocs) RSC_HIP(fill(V->d_work, V->h_work));
    RSC_HIP(fill(C->d_po_in, C->h_po_in));
    RSC_HIP(fill(C->d_po_res, C->h_po_res));
    RSC_HIP(fill(C->d_so_in, C->h_so_in));
    RSC_HIP(fill(C->d_so_res, C->h_so_res));
    RSC_HIP(fill(C->d_lba, C->h_lba));
    RSC_HIP(hipStreamSynchronize(C->stream));
    return total;
}

int rsc_context_set_sim3opt_helpers(rsc_context* C, int helpers) {
    if (!C || helpers < -1) return RSC_ERR_ARG;
    C->so_helpers = helpers;
    return RSC_OK;
}

int rsc_selftest_math(rsc_context* C, int fn, const double* x, int n, double* out) {
    if (!C || fn < 0 || fn > 16 || fn == 14 || fn == 15 || n < 0 || (n > 0 && (!x || !out)) || (fn == 10 && n % 34) ||
        (fn == 16 && n % 42))
        return RSC_ERR_ARG;
    if (n == 0) return RSC_OK;
    RSC_HIP(hipSetDevice(C->device));
    double* d = nullptr;
    RSC_HIP(hipMalloc(&d, (size_t)n * 16));
    std::unique_ptr<double, void (*)(double*)> hold(d, [](double* p) { (void)hipFree(p); });
    RSC_HIP(hipMemcpyAsync(d, x, (size_t)n * 8, hipMemcpyHostToDevice, C->stream));
    if (fn == 16) RSC_HIP(launch_selftest_ldlt(d, n / 42, d + n, C->stream));
    else RSC_HIP(launch_selftest_math(fn, d, n, d + n, C->stream));
    RSC_HIP(hipMemcpyAsync(out, d + n, (size_t)n * 8, hipMemcpyDeviceToHost, C->stream));
    RSC_HIP(hipStreamSynchronize(C->stream));
    return RSC_OK;
}

int rsc_context_last_timing(rsc_context* C, double out[5]) {
    if (!C || !out) return RSC_ERR_ARG;
    for (int i = 0; i < 5; ++i) out[i] = C->last_ms[i];
    return RSC_OK;
}

int rsc_context_last_kernel_timing(rsc_context* C, double out[6]) {
    if (!C || !out) return RSC_ERR_ARG;
    for (int i = 0; i < 6; ++i) out[i] = C->last_ms[i];
    return RSC_OK;
}

// ---- PnP ----
int rsc_pnp_create(rsc_context* C, const rsc_pnp_problem* pb, uint32_t seed, rsc_pnp** out) {
    if (!C || !pb || !out || pb->n < 0 || pb->n_points < pb->n) return RSC_ERR_ARG;
    if (pb->n > 0 && (!pb->p2d || !pb->p3dw || !pb->sigma2)) return RSC_ERR_ARG;
    *out = nullptr;
    RSC_HIP(hipSetDevice(C->device));
    std::unique_ptr<rsc_pnp> S(new rsc_pnp());
    S->ctx = C;
    S->ctx_destroyed = C->pnp_destroyed;
    PnPState& s = S->st;
    s.N = pb->n;
    s.N_points = pb->n_points;
    s.fx = pb->fx; s.fy = pb->fy; s.cx = pb->cx; s.cy = pb->cy;
    s.kp_index.resize(pb->n);
    for (int i = 0; i < pb->n; ++i) s.kp_index[i] = pb->kp_index ? pb->kp_index[i] : i;
    s.sigma2.assign(pb->sigma2, pb->sigma2 + pb->n);
    s.reset(seed);
    S->h_p2d.assign(pb->p2d, pb->p2d + 2 * (size_t)pb->n);
    S->h_p3d.assign(pb->p3dw, pb->p3dw + 3 * (size_t)pb->n);
    const int n = std::max(pb->n, 1);
    S->words = (n + 63) / 64;
    std::vector<float4> pts(n);
    std::vector<float2> uv(n);
    for (int i = 0; i < pb->n; ++i) {
        pts[i] = make_float4(pb->p3dw[3 * i], pb->p3dw[3 * i + 1], pb->p3dw[3 * i + 2], pb->sigma2[i]);
        uv[i] = make_float2(pb->p2d[2 * i], pb->p2d[2 * i + 1]);
    }
    const size_t cap = (size_t)std::max(n, 8);
    RSC_HIP(hipMalloc(&S->d_pts, n * sizeof(float4)));
    RSC_HIP(hipMalloc(&S->d_uv, n * sizeof(float2)));
    RSC_HIP(hipMalloc(&S->d_pws, cap * 3 * sizeof(double)));
    RSC_HIP(hipMalloc(&S->d_us, cap * 2 * sizeof(double)));
    RSC_HIP(hipMalloc(&S->d_als, cap * 4 * sizeof(double)));
    RSC_HIP(hipMalloc(&S->d_best, S->words * 8));
    RSC_HIP(hipMalloc(&S->d_refined, S->words * 8));
    RSC_HIP(hipMemcpy(S->d_pts, pts.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    RSC_HIP(hipMemcpy(S->d_uv, uv.data(), n * sizeof(float2), hipMemcpyHostToDevice));
    RSC_HIP(hipMemset(S->d_pws, 0, cap * 3 * sizeof(double)));
    RSC_HIP(hipMemset(S->d_us, 0, cap * 2 * sizeof(double)));
    RSC_HIP(hipMemset(S->d_als, 0, cap * 4 * sizeof(double)));
    RSC_HIP(hipMemset(S->d_best, 0, S->words * 8));
    RSC_HIP(hipMemset(S->d_refined, 0, S->words * 8));
    // PnPsolver does not call SetRansacParameters in its constructor; iterate() before it is UB in
    // the reference.  Install the declared defaults so that the object is always usable.
    pnp_set_params(s, 0.99, 8, 300, 4, 0.4f, 5.991f);
    *out = S.release();
    return RSC_OK;
}

// ~rsc_pnp counts the context's pnp_destroyed up: a round that named this solver's buffers is not
// counted again (pnp_recount)
void rsc_pnp_destroy(rsc_pnp* s) { delete s; }

int rsc_pnp_set_ransac_parameters(rsc_pnp* s, double probability, int min_inliers, int max_iterations, int min_set,
                                  float epsilon, float th2) {
    if (!s) return RSC_ERR_ARG;
    pnp_set_params(s->st, probability, min_inliers, max_iterations, min_set, epsilon, th2);
    return RSC_OK;
}

int rsc_pnp_iterate_many(rsc_pnp* const* solvers, int count, const int32_t* n_its, rsc_pnp_result* out,
                         uint8_t* const* inliers) {
    if (count <= 0) return RSC_OK;
    if (!solvers || !n_its || !out) return RSC_ERR_ARG;
    for (int i = 0; i < count; ++i)
        if (solvers[i] && solvers[i]->stream)
            return bound_iterate_many(solvers, count, n_its, out, inliers, pnp_iterate_many_impl);
    return pnp_iterate_many_impl(solvers, count, n_its, out, inliers);
}

int pnp_iterate_many_impl(rsc_pnp* const* solvers, int count, const int32_t* n_its, rsc_pnp_result* out,
                                 uint8_t* const* inliers) {
    if (count <= 0) return RSC_OK;
    if (!solvers || !n_its || !out) return RSC_ERR_ARG;
    rsc_context* C = solvers[0]->ctx;
    for (int i = 0; i < count; ++i)
        if (!solvers[i] || solvers[i]->ctx != C) return RSC_ERR_ARG;
    // vbInliers of a call that fails is empty (rsc_pnp_last_inliers returns 0 after it)
    for (int i = 0; i < count; ++i) solvers[i]->last_kind = 0;
    C->t_entry = std::chrono::steady_clock::now();
    RSC_HIP(hipSetDevice(C->device));
    for (double& v : C->last_ms) v = 0;
    HipPnPBackend be(C);
    be.solvers.assign(solvers, solvers + count);
    std::vector<PnPState*> S(count);
    std::vector<int> its(count);
    for (int i = 0; i < count; ++i) { S[i] = &solvers[i]->st; its[i] = n_its[i]; }
    std::vector<PnPResult> res(count);
    int st = pnp_iterate_many(be, S.data(), count, its.data(), res.data(), inliers);
    if (st) return st;
    for (int i = 0; i < count; ++i) {
        to_result(res[i], &out[i]);
        solvers[i]->last_kind = res[i].mask_kind;
    }
    host_mark(C, 3);
    return RSC_OK;
}

int rsc_diag_host_timing(rsc_context* C, double out[4]) {
    if (!C || !out) return RSC_ERR_ARG;
    for (int i = 0; i < 4; ++i) out[i] = C->host_us[i];
    return RSC_OK;
}

int rsc_pnp_iterate(rsc_pnp* s, int n_its, rsc_pnp_result* out, uint8_t* inliers) {
    if (!s || !out) return RSC_ERR_ARG;
    int32_t n = n_its;
    uint8_t* const m[1] = {inliers};
    return rsc_pnp_iterate_many(&s, 1, &n, out, m);
}

int rsc_pnp_find(rsc_pnp* s, rsc_pnp_result* out, uint8_t* inliers) {
    if (!s) return RSC_ERR_ARG;
    return rsc_pnp_iterate(s, s->st.mRansacMaxIts, out, inliers);
}

int rsc_pnp_last_inliers(rsc_pnp* s, uint8_t* out) {
    if (!s || !out) return RSC_ERR_ARG;
    const PnPState& t = s->st;
    std::memset(out, 0, (size_t)t.N_points);
    if (s->last_kind == 0) return 0;
    std::vector<uint64_t> w((size_t)s->words);
    RSC_HIP(hipMemcpyAsync(w.data(), s->last_kind == 1 ? s->d_refined : s->d_best, (size_t)s->words * 8,
                           hipMemcpyDeviceToHost, s->ctx->stream));
    RSC_HIP(hipStreamSynchronize(s->ctx->stream));
    for (int j = 0; j < t.N; ++j)
        if ((w[j >> 6] >> (j & 63)) & 1ull) out[t.kp_index[j]] = 1;
    return 1;
}

int rsc_pnp_reset(rsc_pnp* s, uint32_t seed) {
    if (!s) return RSC_ERR_ARG;
    reset_solver(s, seed);
    s->last_kind = 0;
    return RSC_OK;
}

int rsc_pnp_get_state(const rsc_pnp* s, int32_t out[8]) {
    if (!s || !out) return RSC_ERR_ARG;
    const PnPState& t = s->st;
    out[0] = t.mnIterations; out[1] = t.mRansacMaxIts; out[2] = t.mRansacMinInliers; out[3] = t.mnBestInliers;
    out[4] = t.max_rows; out[5] = t.N; out[6] = t.N_points; out[7] = t.mRansacMinSet;
    return RSC_OK;
}

int rsc_pnp_last_samples(rsc_pnp* s, int32_t* out, int cap) {
    if (!s || !out) return RSC_ERR_ARG;
    rsc_context* C = s->ctx;
    if (s->spec_out0 < 0 || !C->d_samples.p) return 0;
    const int n = std::min(cap, s->spec_H);
    RSC_HIP(hipMemcpy(out, C->d_samples.p + (size_t)s->spec_out0 * 8, (size_t)n * 8 * 4, hipMemcpyDeviceToHost));
    return n;
}

// Parity hook: counts + float poses of the last speculation of this solver.  The counts live in the
// context's pinned count buffer (valid until the context's next speculation); poses stay in HBM.
namespace {
int last_hypotheses(rsc_context* C, int out0, int H, int stride, int32_t* counts, float* poses, int cap) {
    if (out0 < 0) return 0;
    const int n = std::min(cap, H);
    if (counts) std::memcpy(counts, C->h_counts.p + out0, (size_t)n * 4);
    if (poses) {
        if (!C->d_poses.p) return RSC_ERR_ARG;
        std::vector<float> all((size_t)n * stride);
        RSC_HIP(hipMemcpy(all.data(), C->d_poses.p + (size_t)out0 * stride, all.size() * 4, hipMemcpyDeviceToHost));
        for (int h = 0; h < n; ++h) std::memcpy(poses + (size_t)h * 12, all.data() + (size_t)h * stride, 48);
    }
    return n;
}
}  // namespace

int rsc_pnp_last_hypotheses(rsc_pnp* s, int32_t* counts, float* poses, int cap) {
    if (!s) return RSC_ERR_ARG;
    // a round that ran with the scan bound on left partial counts for the hypotheses it cut short
    if (counts && s->spec_out0 >= 0)
        if (int e = pnp_recount(s->ctx)) return e;
    return last_hypotheses(s->ctx, s->spec_out0, s->spec_H, 12, counts, poses, cap);
}

int rsc_pnp_last_counts_raw(rsc_pnp* s, int32_t* counts, int cap) {
    if (!s || !counts) return RSC_ERR_ARG;
    return last_hypotheses(s->ctx, s->spec_out0, s->spec_H, 12, counts, nullptr, cap);
}

// ---- Sim3 ----
int rsc_sim3_create(rsc_context* C, const rsc_sim3_input* in, uint32_t seed, rsc_sim3** out) {
    if (!C || !in || !out || in->n1 < 0) return RSC_ERR_ARG;
    *out = nullptr;
    RSC_HIP(hipSetDevice(C->device));
    std::unique_ptr<rsc_sim3> S(new rsc_sim3());
    S->ctx = C;
    Sim3State& s = S->st;
    s.mN1 = in->n1;
    // Sim3Solver::Sim3Solver (Sim3Solver.cpp:26-68): camera-frame points (float), size_t thresholds
    for (int i1 = 0; i1 < in->n1; ++i1) {
        if (!in->valid[i1]) continue;
        S->e1.push_back((uint64_t)(9.210 * in->sigma2_1[i1]));
        S->e2.push_back((uint64_t)(9.210 * in->sigma2_2[i1]));
        s.indices1.push_back(i1);
        const float* a = &in->Xw1[3 * i1];
        const float* b = &in->Xw2[3 * i1];
        // Rcw*X3Dw + tcw (Sim3Solver.cpp:58,62): Matrix3f * Vector3f, coefficient-path reductions
        for (int r = 0; r < 3; ++r)
            S->X1c.push_back(ered3(in->R1[3 * r] * a[0], in->R1[3 * r + 1] * a[1], in->R1[3 * r + 2] * a[2]) + in->t1[r]);
        for (int r = 0; r < 3; ++r)
            S->X2c.push_back(ered3(in->R2[3 * r] * b[0], in->R2[3 * r + 1] * b[1], in->R2[3 * r + 2] * b[2]) + in->t2[r]);
    }
    s.N = (int)s.indices1.size();
    std::memcpy(S->K1, in->K1, sizeof(S->K1));
    std::memcpy(S->K2, in->K2, sizeof(S->K2));
    // FromCameraToImage (Sim3Solver.cpp:329-347)
    auto to_image = [](const std::vector<float>& X, std::vector<float>& P, const float K[4]) {
        const size_t n = X.size() / 3;
        P.resize(2 * n);
        for (size_t i = 0; i < n; ++i) {
            const float invz = 1 / X[3 * i + 2];
            const float x = X[3 * i] * invz;
            const float y = X[3 * i + 1] * invz;
            P[2 * i] = K[0] * x + K[2];
            P[2 * i + 1] = K[1] * y + K[3];
        }
    };
    to_image(S->X1c, S->P1, S->K1);
    to_image(S->X2c, S->P2, S->K2);
    const int n = std::max(s.N, 1);
    std::vector<float4> x1(n), x2(n), pim(n);
    for (int i = 0; i < s.N; ++i) {
        x1[i] = make_float4(S->X1c[3 * i], S->X1c[3 * i + 1], S->X1c[3 * i + 2], (float)S->e1[i]);
        x2[i] = make_float4(S->X2c[3 * i], S->X2c[3 * i + 1], S->X2c[3 * i + 2], (float)S->e2[i]);
        pim[i] = make_float4(S->P1[2 * i], S->P1[2 * i + 1], S->P2[2 * i], S->P2[2 * i + 1]);
    }
    RSC_HIP(hipMalloc(&S->d_x1, n * sizeof(float4)));
    RSC_HIP(hipMalloc(&S->d_x2, n * sizeof(float4)));
    RSC_HIP(hipMalloc(&S->d_pim, n * sizeof(float4)));
    RSC_HIP(hipMemcpy(S->d_x1, x1.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    RSC_HIP(hipMemcpy(S->d_x2, x2.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    RSC_HIP(hipMemcpy(S->d_pim, pim.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    s.reset(seed);
    sim3_set_params(s, 0.99, 6, 300);  // the constructor's SetRansacParameters() (:84)
    *out = S.release();
    return RSC_OK;
}

void rsc_sim3_destroy(rsc_sim3* s) { delete s; }

int rsc_sim3_set_ransac_parameters(rsc_sim3* s, double probability, int min_inliers, int max_iterations) {
    if (!s) return RSC_ERR_ARG;
    sim3_set_params(s->st, probability, min_inliers, max_iterations);
    return RSC_OK;
}

int rsc_sim3_iterate_many(rsc_sim3* const* solvers, int count, const int32_t* n_its, rsc_sim3_result* out,
                          uint8_t* const* inliers) {
    if (count <= 0) return RSC_OK;
    if (!solvers || !n_its || !out) return RSC_ERR_ARG;
    for (int i = 0; i < count; ++i)
        if (solvers[i] && solvers[i]->stream)
            return bound_iterate_many(solvers, count, n_its, out, inliers, sim3_iterate_many_impl);
    return sim3_iterate_many_impl(solvers, count, n_its, out, inliers);
}

int sim3_iterate_many_impl(rsc_sim3* const* solvers, int count, const int32_t* n_its, rsc_sim3_result* out,
                                  uint8_t* const* inliers) {
    if (count <= 0) return RSC_OK;
    if (!solvers || !n_its || !out) return RSC_ERR_ARG;
    rsc_context* C = solvers[0]->ctx;
    for (int i = 0; i < count; ++i)
        if (!solvers[i] || solvers[i]->ctx != C) return RSC_ERR_ARG;
    RSC_HIP(hipSetDevice(C->device));
    for (double& v : C->last_ms) v = 0;
    HipSim3Backend be(C);
    be.all.assign(solvers, solvers + count);
    std::vector<Sim3State*> S(count);
    std::vector<int> its(count);
    for (int i = 0; i < count; ++i) { S[i] = &solvers[i]->st; its[i] = n_its[i]; }
    std::vector<Sim3Result> res(count);
    int st = sim3_iterate_many(be, S.data(), count, its.data(), res.data(), inliers);
    if (st) return st;
    for (int i = 0; i < count; ++i) {
        out[i].ok = res[i].ok;
        out[i].no_more = res[i].no_more;
        out[i].n_inliers = res[i].n_inliers;
        out[i].iterations = res[i].iterations;
        std::memcpy(out[i].R, res[i].R, sizeof(out[i].R));
        std::memcpy(out[i].t, res[i].t, sizeof(out[i].t));
    }
    return RSC_OK;
}

int rsc_sim3_iterate(rsc_sim3* s, int n_its, rsc_sim3_result* out, uint8_t* inliers) {
    if (!s || !out) return RSC_ERR_ARG;
    int32_t n = n_its;
    uint8_t* const m[1] = {inliers};
    return rsc_sim3_iterate_many(&s, 1, &n, out, m);
}

int rsc_sim3_find(rsc_sim3* s, rsc_sim3_result* out, uint8_t* inliers) {
    if (!s) return RSC_ERR_ARG;
    return rsc_sim3_iterate(s, s->st.mRansacMaxIts, out, inliers);
}

int rsc_sim3_reset(rsc_sim3* s, uint32_t seed) {
    if (!s) return RSC_ERR_ARG;
    const int mi = s->st.mRansacMinInliers, mx = s->st.mRansacMaxIts;
    (void)mi; (void)mx;
    reset_solver(s, seed);
    return RSC_OK;
}

int rsc_sim3_get_state(const rsc_sim3* s, int32_t out[6]) {
    if (!s || !out) return RSC_ERR_ARG;
    const Sim3State& t = s->st;
    out[0] = t.mnIterations; out[1] = t.mRansacMaxIts; out[2] = t.mRansacMinInliers; out[3] = t.mnBestInliers;
    out[4] = t.N; out[5] = t.mN1;
    return RSC_OK;
}

int rsc_sim3_last_hypotheses(rsc_sim3* s, int32_t* counts, float* poses, int cap) {
    if (!s) return RSC_ERR_ARG;
    return last_hypotheses(s->ctx, s->spec_out0, s->spec_H, 24, counts, poses, cap);
}

int rsc_sim3_prepared(const rsc_sim3* s, float* X1c, float* X2c, float* P1im1, float* P2im2, uint64_t* e1,
                      uint64_t* e2, int32_t* idx) {
    if (!s) return RSC_ERR_ARG;
    const int N = s->st.N;
    if (X1c) std::memcpy(X1c, s->X1c.data(), 12 * (size_t)N);
    if (X2c) std::memcpy(X2c, s->X2c.data(), 12 * (size_t)N);
    if (P1im1) std::memcpy(P1im1, s->P1.data(), 8 * (size_t)N);
    if (P2im2) std::memcpy(P2im2, s->P2.data(), 8 * (size_t)N);
    if (e1) std::memcpy(e1, s->e1.data(), 8 * (size_t)N);
    if (e2) std::memcpy(e2, s->e2.data(), 8 * (size_t)N);
    if (idx) std::memcpy(idx, s->st.indices1.data(), 4 * (size_t)N);
    return RSC_OK;
}

int rsc_diag_refine_phase_stamps(rsc_context* C, uint64_t* out, int cap) {
    if (!C || !out || cap < 64 * 24) return RSC_ERR_ARG;
    RSC_HIP(hipStreamSynchronize(C->stream));
    RSC_HIP(read_refine_stamps(out));
    return RSC_OK;
}

int rsc_diag_solve_phase_stamps(rsc_context* C, uint64_t* out, int cap) {
    if (!C || !out || cap < 3 * 4096 * 8) return RSC_ERR_ARG;
    RSC_HIP(hipStreamSynchronize(C->stream));
    RSC_HIP(read_solve_stamps(out));
    return RSC_OK;
}

int rsc_diag_mlpnp_phase_stamps(rsc_context* C, uint64_t* out, int cap) {
    if (!C || !out || cap < 8192 * 8) return RSC_ERR_ARG;
    RSC_HIP(hipStreamSynchronize(C->stream));
    RSC_HIP(read_ml_stamps(out));
    return RSC_OK;
}

int rsc_rand_stream(rsc_context* C, uint32_t seed, int n, int32_t* out) {
    if (!C || !out || n < 0) return RSC_ERR_ARG;
    if (n == 0) return RSC_OK;
    RSC_HIP(hipSetDevice(C->device));
    RngStream r;
    r.seed(seed);
    int done = 0;
    DevBuf<int32_t> d;
    if (int e = d.ensure(std::min(n, 8192))) return e;
    while (done < n) {
        const int chunk = std::min(8192, n - done);
        r.ensure(C->table, chunk);
        RSC_HIP(launch_rng_stream(C->d_table.p, r.words(), r.g, chunk, d.p, C->stream));
        RSC_HIP(hipMemcpyAsync(out + done, d.p, (size_t)chunk * 4, hipMemcpyDeviceToHost, C->stream));
        RSC_HIP(hipStreamSynchronize(C->stream));
        r.g += chunk;
        done += chunk;
    }
    return RSC_OK;
}

// ---- batched state helpers ----
// ---- Shared rand() stream (Q3) ----
int rsc_stream_create(rsc_context* C, uint32_t seed, rsc_stream** out) {
    if (!C || !out) return RSC_ERR_ARG;
    rsc_stream* s = new rsc_stream();
    s->ctx = C;
    s->st.seed(seed);
    s->st.drop_seed_mark();  // bound solvers copy this position: a shared stream is always its words
    *out = s;
    return RSC_OK;
}

void rsc_stream_destroy(rsc_stream* s) { delete s; }

int rsc_stream_skip(rsc_stream* s, int64_t n) {
    if (!s || n < 0) return RSC_ERR_ARG;
    s->st.advance(s->ctx->table, n);
    s->position += n;
    return RSC_OK;
}

int rsc_stream_position(const rsc_stream* s, int64_t* out) {
    if (!s || !out) return RSC_ERR_ARG;
    *out = s->position;
    return RSC_OK;
}

int rsc_stream_peek(rsc_stream* s, int n, int32_t* out) {
    if (!s || !out || n < 0) return RSC_ERR_ARG;
    if (n == 0) return RSC_OK;
    rsc_context* C = s->ctx;
    RSC_HIP(hipSetDevice(C->device));
    RngStream r = s->st;
    DevBuf<int32_t> d;
    if (int e = d.ensure(std::min(n, 8192))) return e;
    for (int done = 0; done < n;) {
        const int chunk = std::min(8192, n - done);
        r.ensure(C->table, chunk);
        RSC_HIP(launch_rng_stream(C->d_table.p, r.words(), r.g, chunk, d.p, C->stream));
        RSC_HIP(hipMemcpyAsync(out + done, d.p, (size_t)chunk * 4, hipMemcpyDeviceToHost, C->stream));
        RSC_HIP(hipStreamSynchronize(C->stream));
        r.g += chunk;
        done += chunk;
    }
    return RSC_OK;
}

int rsc_pnp_bind_stream(rsc_pnp* s, rsc_stream* stream) { return bind_stream(s, stream); }

int rsc_sim3_bind_stream(rsc_sim3* s, rsc_stream* stream) { return bind_stream(s, stream); }

int rsc_mlpnp_bind_stream(rsc_mlpnp* s, rsc_stream* stream) { return bind_stream(s, stream); }

int rsc_pnp_reset_many(rsc_pnp* const* s, int count, const uint32_t* seeds) {
    if (count < 0 || (count && (!s || !seeds))) return RSC_ERR_ARG;
    for (int i = 0; i < count; ++i) {
        if (!s[i]) return RSC_ERR_ARG;
        reset_solver(s[i], seeds[i]);
        s[i]->last_kind = 0;
    }
    return RSC_OK;
}

int rsc_pnp_set_ransac_parameters_many(rsc_pnp* const* s, int count, double probability, int min_inliers,
                                       int max_iterations, int min_set, float epsilon, float th2) {
    if (count < 0 || (count && !s)) return RSC_ERR_ARG;
    for (int i = 0; i < count; ++i) {
        if (!s[i]) return RSC_ERR_ARG;
        pnp_set_params(s[i]->st, probability, min_inliers, max_iterations, min_set, epsilon, th2);
    }
    return RSC_OK;
}

int rsc_sim3_reset_many(rsc_sim3* const* s, int count, const uint32_t* seeds) {
    if (count < 0 || (count && (!s || !seeds))) return RSC_ERR_ARG;
    for (int i = 0; i < count; ++i) {
        if (!s[i]) return RSC_ERR_ARG;
        reset_solver(s[i], seeds[i]);
    }
    return RSC_OK;
}

int rsc_sim3_set_ransac_parameters_many(rsc_sim3* const* s, int count, double probability, int min_inliers,
                                        int max_iterations) {
    if (count < 0 || (count && !s)) return RSC_ERR_ARG;
    for (int i = 0; i < count; ++i) {
        if (!s[i]) return RSC_ERR_ARG;
        sim3_set_params(s[i]->st, probability, min_inliers, max_iterations);
    }
    return RSC_OK;
}

// ---- MLPnP ----
int rsc_mlpnp_create(rsc_context* C, const rsc_pnp_problem* pb, uint32_t seed, rsc_mlpnp** out) {
    if (!C || !pb || !out || pb->n < 0 || pb->n_points < pb->n) return RSC_ERR_ARG;
    if (pb->n > 0 && (!pb->p2d || !pb->p3dw || !pb->sigma2)) return RSC_ERR_ARG;
    *out = nullptr;
    RSC_HIP(hipSetDevice(C->device));
    std::unique_ptr<rsc_mlpnp> S(new rsc_mlpnp());
    S->ctx = C;
    MLState& s = S->st;
    s.N = pb->n;
    s.N_points = pb->n_points;
    S->fx = pb->fx; S->fy = pb->fy; S->cx = pb->cx; S->cy = pb->cy;
    s.kp_index.resize(pb->n);
    for (int i = 0; i < pb->n; ++i) s.kp_index[i] = pb->kp_index ? pb->kp_index[i] : i;
    s.reset(seed);
    const int n = std::max(pb->n, 1);
    S->words = (n + 63) / 64;
    std::vector<float4> pts(n);
    std::vector<float2> uv(n), brg(n);
    for (int i = 0; i < pb->n; ++i) {
        pts[i] = make_float4(pb->p3dw[3 * i], pb->p3dw[3 * i + 1], pb->p3dw[3 * i + 2], pb->sigma2[i]);
        uv[i] = make_float2(pb->p2d[2 * i], pb->p2d[2 * i + 1]);
        // bearing (x, y, 1): float arithmetic as MLPnPsolver.cpp:32-33
        const float bx = (pb->p2d[2 * i] - pb->cx) / pb->fx;
        const float by = (pb->p2d[2 * i + 1] - pb->cy) / pb->fy;
        brg[i] = make_float2(bx, by);
    }
    RSC_HIP(hipMalloc(&S->d_pts, n * sizeof(float4)));
    RSC_HIP(hipMalloc(&S->d_uv, n * sizeof(float2)));
    RSC_HIP(hipMalloc(&S->d_brg, n * sizeof(float2)));
    RSC_HIP(hipMalloc(&S->d_best, S->words * 8));
    RSC_HIP(hipMemcpy(S->d_pts, pts.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    RSC_HIP(hipMemcpy(S->d_uv, uv.data(), n * sizeof(float2), hipMemcpyHostToDevice));
    RSC_HIP(hipMemcpy(S->d_brg, brg.data(), n * sizeof(float2), hipMemcpyHostToDevice));
    RSC_HIP(hipMemset(S->d_best, 0, S->words * 8));
    mlpnp_set_params(s, 0.99, 8, 300, 6, 0.4f, 5.991f);  // the ctor's SetRansacParameters() (:52)
    *out = S.release();
    return RSC_OK;
}

void rsc_mlpnp_destroy(rsc_mlpnp* s) { delete s; }

int rsc_mlpnp_set_covariances(rsc_mlpnp* s, const double* cov) {
    if (!s) return RSC_ERR_ARG;
    if (!cov) {
        s->use_cov = false;
        return RSC_OK;
    }
    const int n = s->st.N;
    for (size_t k = 0; k < 9 * (size_t)n; ++k)
        if (!std::isfinite(cov[k])) return RSC_ERR_ARG;
    RSC_HIP(hipSetDevice(s->ctx->device));
    if (!s->d_cov && n > 0) RSC_HIP(hipMalloc(&s->d_cov, 9 * sizeof(double) * (size_t)n));
    RSC_HIP(hipStreamSynchronize(s->ctx->stream));
    if (n > 0) RSC_HIP(hipMemcpy(s->d_cov, cov, 9 * sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    s->use_cov = n > 0;
    return RSC_OK;
}

int rsc_mlpnp_set_ransac_parameters(rsc_mlpnp* s, double probability, int min_inliers, int max_iterations,
                                    int min_set, float epsilon, float th2) {
    if (!s) return RSC_ERR_ARG;
    if (min_set < 6 || min_set > 8) {
        g_last_error = "MLPnP min_set outside [6,8] (computePose asserts n > 5, MLPnPsolver.cpp:324)";
        return RSC_ERR_UNSUPPORTED;
    }
    mlpnp_set_params(s->st, probability, min_inliers, max_iterations, min_set, epsilon, th2);
    return RSC_OK;
}

int rsc_mlpnp_set_ransac_parameters_many(rsc_mlpnp* const* s, int count, double probability, int min_inliers,
                                         int max_iterations, int min_set, float epsilon, float th2) {
    for (int i = 0; i < count; ++i)
        if (int e = rsc_mlpnp_set_ransac_parameters(s[i], probability, min_inliers, max_iterations, min_set, epsilon,
                                                    th2))
            return e;
    return RSC_OK;
}

static int mlpnp_iterate_many_impl(rsc_mlpnp* const* solvers, int count, const int32_t* n_its, rsc_pnp_result* out,
                                   uint8_t* const* inliers);

int rsc_mlpnp_iterate_many(rsc_mlpnp* const* solvers, int count, const int32_t* n_its, rsc_pnp_result* out,
                           uint8_t* const* inliers) {
    if (count <= 0) return RSC_OK;
    if (!solvers || !n_its || !out) return RSC_ERR_ARG;
    for (int i = 0; i < count; ++i)
        if (solvers[i] && solvers[i]->stream)
            return bound_iterate_many(solvers, count, n_its, out, inliers, mlpnp_iterate_many_impl);
    return mlpnp_iterate_many_impl(solvers, count, n_its, out, inliers);
}

static int mlpnp_iterate_many_impl(rsc_mlpnp* const* solvers, int count, const int32_t* n_its, rsc_pnp_result* out,
                                   uint8_t* const* inliers) {
    if (count <= 0) return RSC_OK;
    if (!solvers || !n_its || !out) return RSC_ERR_ARG;
    rsc_context* C = solvers[0]->ctx;
    for (int i = 0; i < count; ++i)
        if (!solvers[i] || solvers[i]->ctx != C) return RSC_ERR_ARG;
    RSC_HIP(hipSetDevice(C->device));
    for (double& v : C->last_ms) v = 0;
    HipMLBackend be(C);
    be.all.assign(solvers, solvers + count);
    std::vector<MLState*> S(count);
    for (int i = 0; i < count; ++i) S[i] = &solvers[i]->st;
    std::vector<MLResult> res(count);
    if (int st = mlpnp_iterate_many(be, S.data(), count, n_its, res.data(), inliers)) return st;
    for (int i = 0; i < count; ++i) {
        out[i].ok = res[i].ok;
        out[i].no_more = res[i].no_more;
        out[i].n_inliers = res[i].n_inliers;
        out[i].iterations = res[i].iterations;
        std::memcpy(out[i].T, res[i].T, sizeof(out[i].T));
    }
    return RSC_OK;
}

int rsc_mlpnp_iterate(rsc_mlpnp* s, int n_its, rsc_pnp_result* out, uint8_t* inliers) {
    if (!s || !out) return RSC_ERR_ARG;
    int32_t n = n_its;
    uint8_t* const m[1] = {inliers};
    return rsc_mlpnp_iterate_many(&s, 1, &n, out, m);
}

int rsc_mlpnp_reset(rsc_mlpnp* s, uint32_t seed) {
    if (!s) return RSC_ERR_ARG;
    reset_solver(s, seed);
    return RSC_OK;
}

int rsc_mlpnp_reset_many(rsc_mlpnp* const* s, int count, const uint32_t* seeds) {
    if (count > 0 && (!s || !seeds)) return RSC_ERR_ARG;
    for (int i = 0; i < count; ++i) {
        if (!s[i]) return RSC_ERR_ARG;
        reset_solver(s[i], seeds[i]);
    }
    return RSC_OK;
}

int rsc_mlpnp_get_state(const rsc_mlpnp* s, int32_t out[6]) {
    if (!s || !out) return RSC_ERR_ARG;
    const MLState& t = s->st;
    out[0] = t.mnIterations; out[1] = t.mRansacMaxIts; out[2] = t.mRansacMinInliers; out[3] = t.mnBestInliers;
    out[4] = t.N; out[5] = t.mRansacMinSet;
    return RSC_OK;
}

// Parity hook: double poses (R row-major 9 + t 3) of the last launch's hypotheses of this solver.
int rsc_mlpnp_last_poses(rsc_mlpnp* s, double* out, int cap) {
    if (!s || !out) return RSC_ERR_ARG;
    rsc_context* C = s->ctx;
    if (s->spec_out0 < 0 || !C->d_mposes.p) return 0;
    const int n = std::min(cap, s->spec_H);
    RSC_HIP(hipMemcpy(out, C->d_mposes.p + (size_t)s->spec_out0 * 12, (size_t)n * 96, hipMemcpyDeviceToHost));
    return n;
}

int rsc_mlpnp_last_counts(rsc_mlpnp* s, int32_t* counts, int cap) {
    if (!s || !counts) return RSC_ERR_ARG;
    return last_hypotheses(s->ctx, s->spec_out0, s->spec_H, 12, counts, nullptr, cap);
}

int rsc_mlpnp_last_samples(rsc_mlpnp* s, int32_t* out, int cap) {
    if (!s || !out) return RSC_ERR_ARG;
    rsc_context* C = s->ctx;
    if (s->spec_out0 < 0 || !C->d_samples.p) return 0;
    const int n = std::min(cap, s->spec_H);
    RSC_HIP(hipMemcpy(out, C->d_samples.p + (size_t)s->spec_out0 * 8, (size_t)n * 8 * 4, hipMemcpyDeviceToHost));
    return n;
}

}  // extern "C"
