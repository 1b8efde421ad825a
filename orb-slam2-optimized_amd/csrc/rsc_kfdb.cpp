// rsc_kfdb.cpp — the KeyFrame database of the C ABI (rsc_kfdb.h).
#include <array>
#include <cstring>
#include <memory>
#include "rsc_host.h"

extern "C" {

namespace {
int check_bow_vector(const rsc_kfdb* db, int n, const uint32_t* id, const double* val) {
    if (n < 0 || n > db->max_words || (n && (!id || !val))) return RSC_ERR_ARG;
    for (int i = 1; i < n; ++i)
        if (id[i] <= id[i - 1]) return RSC_ERR_ARG;  // a BowVector (std::map) is strictly ascending
    if (n && id[n - 1] >= db->vocab) return RSC_ERR_ARG;  // not a word of the vocabulary
    return RSC_OK;
}
}  // namespace

int rsc_kfdb_create(rsc_context* C, uint32_t vocab_words, int capacity, int max_words, rsc_kfdb** out) {
    if (!C || !out || vocab_words == 0 || vocab_words > (1u << 30) || capacity <= 0 || max_words <= 0 ||
        max_words > kKfdbMaxWords)
        return RSC_ERR_ARG;
    *out = nullptr;
    std::unique_ptr<rsc_kfdb> db(new rsc_kfdb);
    db->ctx = C;
    db->cap = capacity;
    db->max_words = max_words;
    db->vocab = vocab_words;
    db->present.assign(capacity, 0);
    RSC_HIP(hipSetDevice(C->device));
    const size_t K = (size_t)capacity;
    int e = 0;
    if ((e = db->covis_h.ensure(K * kKfdbCovis)) || (e = db->covis_n_h.ensure(K))) return e;
    std::memset(db->covis_h.p, 0, K * kKfdbCovis * sizeof(int32_t));
    std::memset(db->covis_n_h.p, 0, K * sizeof(int32_t));
    if ((e = db->ids.ensure(K * max_words)) || (e = db->vals.ensure(K * max_words)) || (e = db->len.ensure(K)) ||
        (e = db->seq.ensure(K)) || (e = db->covis.ensure(K * kKfdbCovis)) || (e = db->covis_n.ensure(K)) ||
        (e = db->query.ensure(2 * K)) || (e = db->words.ensure(2 * K)) || (e = db->score.ensure(2 * K)) ||
        (e = db->list.ensure(K)) || (e = db->key.ensure(K)) || (e = db->scored.ensure(K)) || (e = db->sc.ensure(K)) ||
        (e = db->acc.ensure(K)) || (e = db->tscore.ensure(K)) || (e = db->best.ensure(K)) || (e = db->tmp.ensure(K)) || (e = db->counters.ensure(4)) ||
        (e = db->out.ensure(K + 1)) || (e = db->qbuf.ensure(16 * (size_t)max_words + 16)) ||
        (e = db->conn.ensure(K)))
        return e;
    const size_t stage = std::max((size_t)max_words * 16 + 16 + K, (K + 1) * 4);
    if ((e = db->stage.ensure(stage))) return e;
    // KeyFrame.cpp:15: query ids and word counts start at 0; the scores (uninitialised in the
    // reference) are defined as 0
    RSC_HIP(hipMemsetAsync(db->counters.p, 0, 16, C->stream));  // the finish kernel re-zeroes n_list
    RSC_HIP(hipMemsetAsync(db->len.p, 0, 4 * K, C->stream));
    RSC_HIP(hipMemsetAsync(db->covis_n.p, 0, 4 * K, C->stream));
    RSC_HIP(hipMemsetAsync(db->covis.p, 0, 4 * K * kKfdbCovis, C->stream));  // padded rows read slot 0
    RSC_HIP(hipMemsetAsync(db->query.p, 0, 16 * K, C->stream));
    RSC_HIP(hipMemsetAsync(db->words.p, 0, 8 * K, C->stream));
    RSC_HIP(hipMemsetAsync(db->score.p, 0, 8 * K, C->stream));
    RSC_HIP(hipStreamSynchronize(C->stream));
    *out = db.release();
    return RSC_OK;
}

void rsc_kfdb_destroy(rsc_kfdb* db) { destroy_on_stream(db); }

int rsc_kfdb_add(rsc_kfdb* db, int kf, int n, const uint32_t* id, const double* val) {
    if (!db || kf < 0 || kf >= db->cap) return RSC_ERR_ARG;
    if (int e = check_bow_vector(db, n, id, val)) return e;
    if (db->present[kf]) return RSC_ERR_UNSUPPORTED;
    rsc_context* C = db->ctx;
    RSC_HIP(hipSetDevice(C->device));
    const size_t o = (size_t)kf * db->max_words;
    const uint32_t s = db->next_seq++;
    RSC_HIP(hipStreamSynchronize(C->stream));
    if (n) {
        RSC_HIP(hipMemcpy(db->ids.p + o, id, 4 * (size_t)n, hipMemcpyHostToDevice));
        RSC_HIP(hipMemcpy(db->vals.p + o, val, 8 * (size_t)n, hipMemcpyHostToDevice));
    }
    RSC_HIP(hipMemcpy(db->seq.p + kf, &s, 4, hipMemcpyHostToDevice));
    RSC_HIP(hipMemcpy(db->len.p + kf, &n, 4, hipMemcpyHostToDevice));
    db->present[kf] = 1;
    db->touch(kf);
    return RSC_OK;
}

int rsc_kfdb_erase(rsc_kfdb* db, int kf) {
    if (!db || kf < 0 || kf >= db->cap) return RSC_ERR_ARG;
    if (!db->present[kf]) return RSC_OK;
    RSC_HIP(hipSetDevice(db->ctx->device));
    RSC_HIP(hipMemsetAsync(db->len.p + kf, 0, 4, db->ctx->stream));
    RSC_HIP(hipStreamSynchronize(db->ctx->stream));
    db->present[kf] = 0;
    return RSC_OK;
}

int rsc_kfdb_release(rsc_kfdb* db, int kf) {
    if (!db || kf < 0 || kf >= db->cap) return RSC_ERR_ARG;
    rsc_context* C = db->ctx;
    RSC_HIP(hipSetDevice(C->device));
    const size_t K = (size_t)db->cap;
    RSC_HIP(hipMemsetAsync(db->len.p + kf, 0, 4, C->stream));
    for (int t = 0; t < 2; ++t) {
        RSC_HIP(hipMemsetAsync(db->query.p + t * K + kf, 0, 8, C->stream));
        RSC_HIP(hipMemsetAsync(db->words.p + t * K + kf, 0, 4, C->stream));
        RSC_HIP(hipMemsetAsync(db->score.p + t * K + kf, 0, 4, C->stream));
    }
    RSC_HIP(hipMemsetAsync(db->covis.p + (size_t)kf * kKfdbCovis, 0, 4 * kKfdbCovis, C->stream));
    RSC_HIP(hipMemsetAsync(db->covis_n.p + kf, 0, 4, C->stream));
    RSC_HIP(hipStreamSynchronize(C->stream));
    std::fill(db->covis_h.p + (size_t)kf * kKfdbCovis, db->covis_h.p + (size_t)(kf + 1) * kKfdbCovis, 0);
    db->covis_n_h.p[kf] = 0;
    db->present[kf] = 0;
    return RSC_OK;
}

int rsc_kfdb_clear(rsc_kfdb* db) {
    if (!db) return RSC_ERR_ARG;
    RSC_HIP(hipSetDevice(db->ctx->device));
    RSC_HIP(hipMemsetAsync(db->len.p, 0, 4 * (size_t)db->cap, db->ctx->stream));
    RSC_HIP(hipStreamSynchronize(db->ctx->stream));
    std::fill(db->present.begin(), db->present.end(), 0);
    return RSC_OK;
}

int rsc_kfdb_set_covisibility(rsc_kfdb* db, int kf, int n, const int32_t* best) {
    if (!db || kf < 0 || kf >= db->cap || n < 0 || n > kKfdbCovis || (n && !best)) return RSC_ERR_ARG;
    const int32_t nn = n;
    // one covisibility row padded to kKfdbCovis entries (the _many form reads rows of that stride)
    std::array<int32_t, kKfdbCovis> row{};
    for (int i = 0; i < n && i < kKfdbCovis; ++i) row[i] = best[i];
    return rsc_kfdb_set_covisibility_many(db, 1, &kf, &nn, row.data());
}

int rsc_kfdb_set_covisibility_many(rsc_kfdb* db, int count, const int32_t* kf, const int32_t* n,
                                   const int32_t* best) {
    if (!db || count < 0 || (count && (!kf || !n || !best))) return RSC_ERR_ARG;
    for (int c = 0; c < count; ++c) {  // validate everything before touching the mirror
        if (kf[c] < 0 || kf[c] >= db->cap || n[c] < 0 || n[c] > kKfdbCovis) return RSC_ERR_ARG;
        for (int i = 0; i < n[c]; ++i)
            if (best[(size_t)c * kKfdbCovis + i] < 0 || best[(size_t)c * kKfdbCovis + i] >= db->cap) return RSC_ERR_ARG;
    }
    // a copy of the mirror from the previous call may still be in flight
    RSC_HIP(hipSetDevice(db->ctx->device));
    RSC_HIP(hipStreamSynchronize(db->ctx->stream));
    // rows whose content changed go up as one span [lo, hi] (the mirror keeps the rest)
    int lo = INT32_MAX, hi = -1;
    for (int c = 0; c < count; ++c) {
        int32_t* row = db->covis_h.p + (size_t)kf[c] * kKfdbCovis;
        bool changed = db->covis_n_h.p[kf[c]] != n[c];
        for (int i = 0; i < kKfdbCovis; ++i) {
            const int32_t v = i < n[c] ? best[(size_t)c * kKfdbCovis + i] : 0;
            changed |= row[i] != v;
            row[i] = v;
            if (i < n[c]) db->touch(v);
        }
        db->covis_n_h.p[kf[c]] = n[c];
        db->touch(kf[c]);
        if (changed) {
            lo = std::min(lo, kf[c]);
            hi = std::max(hi, kf[c]);
        }
    }
    if (hi < 0) return RSC_OK;
    // two copy kernels on the context stream (stream order puts them before the next query's
    // kernels; the next call that rewrites the mirror synchronises first)
    const size_t rows = (size_t)(hi - lo + 1);
    RSC_HIP(launch_copy_bytes(db->covis_h.p + (size_t)lo * kKfdbCovis, db->covis.p + (size_t)lo * kKfdbCovis,
                              4 * kKfdbCovis * rows, db->ctx->stream));
    RSC_HIP(launch_copy_bytes(db->covis_n_h.p + lo, db->covis_n.p + lo, 4 * rows, db->ctx->stream));
    return RSC_OK;
}

namespace {
int kfdb_query(rsc_kfdb* db, uint64_t qid, int n, const uint32_t* id, const double* val, int loop, int n_conn,
               const int32_t* conn, float min_score, int32_t* cand, int32_t* n_cand) {
    if (!db || !cand || !n_cand) return RSC_ERR_ARG;
    if (int e = check_bow_vector(db, n, id, val)) return e;
    if (loop && (n_conn < 0 || (n_conn && !conn))) return RSC_ERR_ARG;
    rsc_context* C = db->ctx;
    const size_t K = (size_t)db->cap;
    RSC_HIP(hipSetDevice(C->device));
    RSC_HIP(hipStreamSynchronize(C->stream));  // the staging buffer is free again
    char* h = db->stage.p;
    const size_t vo = (4 * (size_t)n + 7) & ~(size_t)7;  // vals offset in the packed query
    if (n) {
        std::memcpy(h, id, 4 * (size_t)n);
        std::memcpy(h + vo, val, 8 * (size_t)n);
        RSC_HIP(launch_copy_bytes(h, db->qbuf.p, vo + 8 * (size_t)n, C->stream));
    }
    if (loop) {
        for (int i = 0; i < n_conn; ++i)
            if (conn[i] < 0 || conn[i] >= db->cap) return RSC_ERR_ARG;
        for (int i = 0; i < n_conn; ++i) db->touch(conn[i]);
    }
    if (db->hw == 0) {  // nothing was ever added: no candidates, no state to update
        *n_cand = 0;
        return RSC_OK;
    }
    const size_t H = (size_t)db->hw;  // the sweeps and the copies cover the slots in use only
    if (loop) {
        uint8_t* m = reinterpret_cast<uint8_t*>(h + 16 * (size_t)db->max_words + 16);
        std::memset(m, 0, H);
        for (int i = 0; i < n_conn; ++i) m[conn[i]] = 1;
        RSC_HIP(launch_copy_bytes(m, db->conn.p, H, C->stream));
    }
    KfdbQuery q;
    q.id = (unsigned long long)qid;
    q.n = n;
    q.loop = loop;
    q.min_score = min_score;
    DevKFDB d = db->dev();
    d.qvals = reinterpret_cast<const double*>(db->qbuf.p + vo);
    RSC_HIP(timed_launch(C, [&] { return launch_kfdb_query(d, q, C->stream); }));
    RSC_HIP(launch_copy_bytes(db->out.p, h, 4 * (H + 1), C->stream));  // written into pinned memory
    RSC_HIP(hipStreamSynchronize(C->stream));
    timing_read(C);
    const int32_t* o = reinterpret_cast<const int32_t*>(h);
    *n_cand = o[0];
    std::memcpy(cand, o + 1, 4 * (size_t)o[0]);
    return RSC_OK;
}
}  // namespace

int rsc_kfdb_detect_relocalization(rsc_kfdb* db, uint64_t frame_id, int n, const uint32_t* id, const double* val,
                                   int32_t* cand, int32_t* n_cand) {
    return kfdb_query(db, frame_id, n, id, val, 0, 0, nullptr, 0.0f, cand, n_cand);
}

int rsc_kfdb_detect_loop(rsc_kfdb* db, uint64_t kf_id, int n, const uint32_t* id, const double* val, int n_conn,
                         const int32_t* conn, float min_score, int32_t* cand, int32_t* n_cand) {
    return kfdb_query(db, kf_id, n, id, val, 1, n_conn, conn, min_score, cand, n_cand);
}

int rsc_kfdb_state(rsc_kfdb* db, int kf, uint64_t* q, int32_t* w, float* s) {
    if (!db || kf < 0 || kf >= db->cap || !q || !w || !s) return RSC_ERR_ARG;
    RSC_HIP(hipSetDevice(db->ctx->device));
    RSC_HIP(hipStreamSynchronize(db->ctx->stream));
    for (int t = 0; t < 2; ++t) {
        unsigned long long qq = 0;
        RSC_HIP(hipMemcpy(&qq, db->query.p + (size_t)t * db->cap + kf, 8, hipMemcpyDeviceToHost));
        q[t] = qq;
        RSC_HIP(hipMemcpy(&w[t], db->words.p + (size_t)t * db->cap + kf, 4, hipMemcpyDeviceToHost));
        RSC_HIP(hipMemcpy(&s[t], db->score.p + (size_t)t * db->cap + kf, 4, hipMemcpyDeviceToHost));
    }
    return RSC_OK;
}

int rsc_diag_kfdb_stamps(rsc_context* C, uint64_t* out, int cap) {
    if (!C || !out || cap < 4096 * 4) return RSC_ERR_ARG;
    RSC_HIP(hipSetDevice(C->device));
    RSC_HIP(hipStreamSynchronize(C->stream));
    RSC_HIP(read_kfdb_stamps(out));
    return RSC_OK;
}

}  // extern "C"
