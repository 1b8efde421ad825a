// rsc_voc.cpp — the vocabulary of the C ABI: create, transform, and the BoW view built from a transform.
#include <algorithm>
#include <cstring>
#include <memory>
#include "rsc_host.h"

extern "C" {

// ---- ORBVocabulary::transform (DBoW2 TemplatedVocabulary.h:1127-1194, :1218-1259) ----
int rsc_voc_create(rsc_context* C, const rsc_vocabulary_nodes* v, rsc_voc** out) {
    if (!C || !v || !out) return RSC_ERR_ARG;
    *out = nullptr;
    const int nn = v->n_nodes;
    if (nn < 2 || !v->parent || !v->is_leaf || !v->desc || !v->weight || v->lds_budget_bytes < 0) return RSC_ERR_ARG;
    if (v->scoring != RSC_VOC_L1_NORM || v->weighting != RSC_VOC_TF_IDF) {
        g_last_error = "vocabulary: only TF_IDF weighting with L1_NORM scoring is supported";
        return RSC_ERR_UNSUPPORTED;
    }
    std::vector<int32_t> nch((size_t)nn, 0), first((size_t)nn + 1, 0);
    for (int i = 1; i < nn; ++i) {
        if (v->parent[i] < 0 || v->parent[i] >= i) {
            g_last_error = "vocabulary: parent[i] must be in [0, i)";
            return RSC_ERR_ARG;
        }
        ++nch[v->parent[i]];
    }
    int max_children = 0;
    for (int i = 0; i < nn; ++i) max_children = std::max(max_children, nch[i]);
    if (max_children > kVocMaxChildren) {
        g_last_error = "vocabulary: more than 32 children under one node";
        return RSC_ERR_UNSUPPORTED;
    }
    // children vectors in push order (ascending node id) as CSR
    for (int i = 0; i < nn; ++i) first[i + 1] = first[i] + nch[i];
    std::vector<int32_t> child((size_t)nn - 1), fill(first.begin(), first.end() - 1);
    for (int i = 1; i < nn; ++i) child[fill[v->parent[i]]++] = i;
    // breadth-first order: a node's children are one run, the levels are prefixes
    std::vector<int32_t> order((size_t)nn), depth((size_t)nn, 0);
    order[0] = 0;
    int tail = 1;
    for (int head = 0; head < nn; ++head) {
        const int o = order[head];
        for (int e = first[o]; e < first[o + 1]; ++e) {
            depth[tail] = depth[head] + 1;
            order[tail++] = child[e];
        }
    }
    std::vector<uint32_t> word_of((size_t)nn, 0);
    uint32_t n_words = 0;
    for (int i = 1; i < nn; ++i)  // the loader's loop starts at node 1 (:1378-1415)
        if (v->is_leaf[i] > 0) word_of[i] = n_words++;
    const int budget = std::min(v->lds_budget_bytes ? v->lds_budget_bytes : kVocLdsBudgetDefault, kVocLdsBudgetMax);
    int lds_nodes = 0, lds_levels = 0, min_leaf = nn, max_depth = 0;
    for (int d = 0, i = 0; i < nn; ++d) {
        int j = i;
        while (j < nn && depth[j] == d) ++j;
        if ((size_t)j * kVocLdsNodeBytes > (size_t)budget) break;
        lds_nodes = j;
        lds_levels = d + 1;
        i = j;
    }
    std::unique_ptr<rsc_voc> V(new rsc_voc);
    ViewImage img(56 * (size_t)nn + 5 * 256);  // every piece in breadth-first order, filled below
    const auto desc = img.hold(V->dev.desc, 2 * (size_t)nn);  // a descriptor is two uint4
    const auto rec = img.hold(V->dev.rec, (size_t)nn);
    const auto orig = img.hold(V->dev.orig, (size_t)nn);
    const auto word = img.hold(V->dev.word, (size_t)nn);
    const auto wt = img.hold(V->dev.weight, (size_t)nn);
    char* h = img.h.data();
    int next = 1;  // dense index of the next child run
    for (int p = 0; p < nn; ++p) {
        const int o = order[p];
        std::memcpy(at(h, desc) + 2 * p, v->desc + 32 * (size_t)o, 32);
        at(h, rec)[p] = make_uint2((uint32_t)next, (uint32_t)nch[o]);
        next += nch[o];
        at(h, orig)[p] = (uint32_t)o;
        at(h, word)[p] = word_of[o];
        at(h, wt)[p] = v->weight[o];
        if (nch[o] == 0) {
            min_leaf = std::min(min_leaf, depth[p]);
            max_depth = std::max(max_depth, depth[p]);
        }
    }
    V->ctx = C;
    V->n_words = n_words;
    V->L = v->L;
    V->lds_levels = lds_levels;
    V->min_leaf_depth = min_leaf;
    V->max_children = max_children;
    if (int e = upload_image(C, V->mem, img)) return e;
    for (auto& e : V->ev) RSC_HIP(hipEventCreate(&e));
    V->dev.n_nodes = nn;
    V->dev.lds_nodes = lds_nodes;
    V->dev.max_depth = max_depth;
    C->vocs.push_back(V.get());
    *out = V.release();
    return RSC_OK;
}

void rsc_voc_destroy(rsc_voc* V) {
    if (V) {
        auto& vs = V->ctx->vocs;
        vs.erase(std::remove(vs.begin(), vs.end(), V), vs.end());
    }
    destroy_on_stream(V);
}

int rsc_voc_size(const rsc_voc* V, uint32_t* n_words) {
    if (!V || !n_words) return RSC_ERR_ARG;
    *n_words = V->n_words;
    return RSC_OK;
}

int rsc_voc_info(const rsc_voc* V, int32_t* info) {
    if (!V || !info) return RSC_ERR_ARG;
    info[0] = V->dev.lds_nodes;
    info[1] = V->lds_levels;
    info[2] = V->min_leaf_depth;
    info[3] = V->dev.max_depth;
    info[4] = V->max_children;
    return RSC_OK;
}

namespace {
// A view whose descriptors and FeatureVector arrays already live on the device (rsc_bow_create_transformed)
struct VocResident {
    const uint4* desc;
    uint32_t* node_id;
    int32_t* node_begin;
    uint32_t* feat;
};

// The transform of `count` views: descriptors from desc[c] (host) or from resident (count == 1).
// When `resident` is given the FeatureVector stays on the device and only its feat entries come back
// (to feat_back).
int voc_transform(rsc_voc* V, int count, const int32_t* n, const uint8_t* const* desc, const VocResident* resident,
                  int levelsup, rsc_voc_output* out, std::vector<uint32_t>* feat_back) {
    rsc_context* C = V->ctx;
    if (count < 0 || count > 65535 || (count && (!n || !out))) return RSC_ERR_ARG;
    if (count == 0) return RSC_OK;
    int max_n = 0;
    for (int c = 0; c < count; ++c) {
        if (n[c] < 0 || (n[c] > 0 && !resident && (!desc || !desc[c]))) return RSC_ERR_ARG;
        if (n[c] > kVocMaxFeatures) {
            g_last_error = "more than 8192 descriptors in one view";
            return RSC_ERR_UNSUPPORTED;
        }
        max_n = std::max(max_n, n[c]);
    }
    const int nid_level = V->L - levelsup;
    if (nid_level > V->min_leaf_depth) {
        g_last_error = "vocabulary transform: L - levelsup lies below the shallowest leaf (the reference leaves the "
                       "node id uninitialised)";
        return RSC_ERR_UNSUPPORTED;
    }
    // job table | descriptors || per view: counts, f_word, f_node, f_weight, word_id, word_value,
    // node_id, node_begin, feat (the part after || comes back)
    struct Off { size_t desc, cnt, fw, fn, fwt, wid, wval, nid, nbeg, feat; };
    std::vector<Off> off((size_t)count);
    size_t at = al256(sizeof(VocJob) * (size_t)count);
    for (int c = 0; c < count; ++c) {
        off[c].desc = at;
        if (!resident) at += al256(32 * (size_t)n[c]);
    }
    const size_t o_back = at;
    for (int c = 0; c < count; ++c) {
        const size_t m = (size_t)n[c];
        Off& o = off[c];
        o.cnt = at;  at += 256;
        o.fwt = at;  at += al256(8 * m);
        o.wval = at; at += al256(8 * m);
        o.fw = at;   at += al256(4 * m);
        o.fn = at;   at += al256(4 * m);
        o.wid = at;  at += al256(4 * m);
        o.nid = at;  at += al256(4 * m);
        o.nbeg = at; at += al256(4 * (m + 1));
        o.feat = at; at += al256(4 * m);
    }
    const size_t bytes = at;
    RSC_HIP(hipSetDevice(C->device));
    if (int e = V->d_work.ensure(bytes)) return e;
    if (int e = V->h_work.ensure(bytes)) return e;
    RSC_HIP(hipStreamSynchronize(C->stream));  // the pinned mirror is free again
    char* d = V->d_work.p;
    char* h = V->h_work.p;
    VocJob* jobs = reinterpret_cast<VocJob*>(h);
    for (int c = 0; c < count; ++c) {
        const Off& o = off[c];
        VocJob& j = jobs[c];
        j.n = n[c];
        j.f_word = reinterpret_cast<uint32_t*>(d + o.fw);
        j.f_node = reinterpret_cast<uint32_t*>(d + o.fn);
        j.f_weight = reinterpret_cast<double*>(d + o.fwt);
        j.word_id = reinterpret_cast<uint32_t*>(d + o.wid);
        j.word_value = reinterpret_cast<double*>(d + o.wval);
        j.counts = reinterpret_cast<int32_t*>(d + o.cnt);
        if (resident) {
            j.desc = resident->desc;
            j.node_id = resident->node_id;
            j.node_begin = resident->node_begin;
            j.feat = resident->feat;
        } else {
            j.desc = reinterpret_cast<const uint4*>(d + o.desc);
            j.node_id = reinterpret_cast<uint32_t*>(d + o.nid);
            j.node_begin = reinterpret_cast<int32_t*>(d + o.nbeg);
            j.feat = reinterpret_cast<uint32_t*>(d + o.feat);
            if (n[c]) std::memcpy(h + o.desc, desc[c], 32 * (size_t)n[c]);
        }
    }
    RSC_HIP(hipMemcpyAsync(d, h, o_back, hipMemcpyHostToDevice, C->stream));
    RSC_HIP(launch_voc_transform(V->dev, reinterpret_cast<const VocJob*>(d), count, max_n, nid_level,
                                 V->max_children > 16, C->timing ? V->ev : nullptr, C->stream));
    RSC_HIP(hipMemcpyAsync(h + o_back, d + o_back, bytes - o_back, hipMemcpyDeviceToHost, C->stream));
    if (resident && feat_back && n[0]) {
        feat_back->resize((size_t)n[0]);
        RSC_HIP(hipMemcpyAsync(feat_back->data(), resident->feat, 4 * (size_t)n[0], hipMemcpyDeviceToHost, C->stream));
    }
    RSC_HIP(hipStreamSynchronize(C->stream));
    if (C->timing) {
        float a = 0, b = 0;
        (void)hipEventElapsedTime(&a, V->ev[0], V->ev[1]);
        (void)hipEventElapsedTime(&b, V->ev[1], V->ev[2]);
        V->last_ms[0] = a;
        V->last_ms[1] = b;
    }
    for (int c = 0; c < count; ++c) {
        const Off& o = off[c];
        rsc_voc_output& r = out[c];
        const int32_t* cnt = reinterpret_cast<const int32_t*>(h + o.cnt);
        const int nw = cnt[0], nnod = cnt[1], m = cnt[2];
        if (nw < 0 || nw > n[c] || nnod < 0 || nnod > n[c] || m < 0 || m > n[c]) {
            g_last_error = "vocabulary transform: inconsistent counts from the device";
            return RSC_ERR_INTERNAL;
        }
        r.n_words = nw;
        r.n_nodes = nnod;
        if (r.word_id && nw) std::memcpy(r.word_id, h + o.wid, 4 * (size_t)nw);
        if (r.word_value && nw) std::memcpy(r.word_value, h + o.wval, 8 * (size_t)nw);
        if (!resident) {
            if (r.node_id && nnod) std::memcpy(r.node_id, h + o.nid, 4 * (size_t)nnod);
            if (r.node_begin) std::memcpy(r.node_begin, h + o.nbeg, 4 * ((size_t)nnod + 1));
            if (r.feat && m) std::memcpy(r.feat, h + o.feat, 4 * (size_t)m);
        }
        if (r.feature_word && n[c]) std::memcpy(r.feature_word, h + o.fw, 4 * (size_t)n[c]);
        if (r.feature_node && n[c]) std::memcpy(r.feature_node, h + o.fn, 4 * (size_t)n[c]);
        if (r.feature_stopped) {
            const double* wt = reinterpret_cast<const double*>(h + o.fwt);
            for (int i = 0; i < n[c]; ++i) r.feature_stopped[i] = wt[i] > 0.0 ? 0 : 1;
        }
        if (resident && feat_back) feat_back->resize((size_t)m);
    }
    return RSC_OK;
}
}  // namespace

int rsc_voc_transform_many(rsc_voc* V, int count, const int32_t* n, const uint8_t* const* desc, int levelsup,
                           rsc_voc_output* out) {
    if (!V) return RSC_ERR_ARG;
    return voc_transform(V, count, n, desc, nullptr, levelsup, out, nullptr);
}

int rsc_voc_last_kernel_timing(rsc_voc* V, double* ms2) {
    if (!V || !ms2) return RSC_ERR_ARG;
    ms2[0] = V->last_ms[0];
    ms2[1] = V->last_ms[1];
    return RSC_OK;
}

int rsc_bow_create_transformed(rsc_context* C, rsc_voc* V, const rsc_bow_features* f, int levelsup, rsc_bow** out,
                               rsc_voc_output* bow) {
    if (!C || !V || !f || !out || V->ctx != C) return RSC_ERR_ARG;
    *out = nullptr;
    const int n = f->n;
    if (n < 0 || (n > 0 && (!f->desc || !f->angle))) return RSC_ERR_ARG;
    if (n > kBowMaxFeatures) {
        g_last_error = "more than 8192 keypoints in one view";
        return RSC_ERR_UNSUPPORTED;
    }
    // the view's allocation sized for the largest FeatureVector n descriptors can give (n nodes of
    // one feature); the uploaded part is desc | angle | valid
    std::unique_ptr<rsc_bow> b(new rsc_bow);
    b->ctx = C;
    b->n = n;
    const size_t o_desc = 0, o_ang = al256(32 * (size_t)n), o_val = o_ang + al256(4 * (size_t)n);
    const size_t o_dfv = o_val + al256((size_t)n), o_id = o_dfv + al256(32 * (size_t)n);
    const size_t o_beg = o_id + al256(4 * (size_t)n), o_feat = o_beg + al256(4 * ((size_t)n + 1));
    const size_t bytes = o_feat + al256(4 * (size_t)n);
    RSC_HIP(hipSetDevice(C->device));
    if (int e = b->mem.ensure(bytes)) return e;
    char* d = b->mem.p;
    if (n) {
        std::vector<char> h(o_dfv, 0);
        std::memcpy(h.data() + o_desc, f->desc, 32 * (size_t)n);
        std::memcpy(h.data() + o_ang, f->angle, 4 * (size_t)n);
        if (f->valid) std::memcpy(h.data() + o_val, f->valid, (size_t)n);
        RSC_HIP(hipMemcpy(d, h.data(), o_dfv, hipMemcpyHostToDevice));
    }
    VocResident res;
    res.desc = reinterpret_cast<const uint4*>(d + o_desc);
    res.node_id = reinterpret_cast<uint32_t*>(d + o_id);
    res.node_begin = reinterpret_cast<int32_t*>(d + o_beg);
    res.feat = reinterpret_cast<uint32_t*>(d + o_feat);
    rsc_voc_output tmp{};
    rsc_voc_output* r = bow ? bow : &tmp;
    const int32_t nv = n;
    // the FeatureVector's feat entries are downloaded before the validity flags go on (the host copy
    // rsc_bow_set_valid re-flags)
    if (int e = voc_transform(V, 1, &nv, nullptr, &res, levelsup, r, &b->feat)) return e;
    b->n_nodes = r->n_nodes;
    b->n_feat = (int)b->feat.size();
    VocGather g;
    g.desc = res.desc;
    g.desc_fv = reinterpret_cast<uint4*>(d + o_dfv);
    g.feat = res.feat;
    g.valid = f->valid ? reinterpret_cast<const uint8_t*>(d + o_val) : nullptr;
    g.counts = reinterpret_cast<const int32_t*>(V->d_work.p + al256(sizeof(VocJob)));
    g.n = n;
    RSC_HIP(launch_voc_gather(g, kBowInvalid, C->stream));
    RSC_HIP(hipStreamSynchronize(C->stream));  // the counts live in the vocabulary's work buffer
    flag_invalid(b->feat, f->valid);
    DevBow hd;
    hd.desc = res.desc;
    hd.desc_fv = g.desc_fv;
    hd.angle = reinterpret_cast<const float*>(d + o_ang);
    hd.node_id = res.node_id;
    hd.node_begin = res.node_begin;
    hd.feat = res.feat;
    hd.n = n;
    hd.n_nodes = b->n_nodes;
    b->off_feat = o_feat;
    b->hdr = hd;
    *out = b.release();
    return RSC_OK;
}

}  // extern "C"
