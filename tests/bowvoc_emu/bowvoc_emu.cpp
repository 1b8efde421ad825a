// TEST-ONLY single-core sequential vocabulary transform: what a host caller runs per Frame with
// DBoW2 (TemplatedVocabulary::transform, TemplatedVocabulary.h:1127-1194): one descent per feature,
// a std::map BowVector with += per hit, the L1 normalisation in key order, a std::map FeatureVector.
// The CPU baseline of tools/bowvoc_bench.py and a second restatement beside tests/bowvoc_ref.py.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

namespace {
struct Node {
    std::vector<uint32_t> children;
    uint64_t d[4];
    double weight;
    uint32_t word_id;
};
struct Voc {
    std::vector<Node> nodes;
    int L;
};

inline int distance(const uint64_t* a, const uint64_t* b) {
    return __builtin_popcountll(a[0] ^ b[0]) + __builtin_popcountll(a[1] ^ b[1]) + __builtin_popcountll(a[2] ^ b[2]) +
           __builtin_popcountll(a[3] ^ b[3]);
}
}  // namespace

extern "C" {

// parent[i] < i for i > 0 is the caller's duty (the reference indexes m_nodes[pid] unchecked)
void* bve_create(int L, int n_nodes, const int32_t* parent, const uint8_t* is_leaf, const uint8_t* desc,
                 const double* weight) {
    Voc* v = new Voc;
    v->L = L;
    v->nodes.resize((size_t)n_nodes);
    uint32_t words = 0;
    for (int i = 0; i < n_nodes; ++i) {
        Node& nd = v->nodes[i];
        std::memcpy(nd.d, desc + 32 * (size_t)i, 32);
        nd.weight = weight[i];
        nd.word_id = 0;
        if (i == 0) continue;
        v->nodes[parent[i]].children.push_back((uint32_t)i);
        if (is_leaf[i] > 0) nd.word_id = words++;
    }
    return v;
}

void bve_destroy(void* h) { delete static_cast<Voc*>(h); }

// Outputs have room for n entries (node_begin: n + 1); counts[0] = words, counts[1] = nodes.
// Returns 0, or -1 when a descent ends above nid_level (the reference's node id is unset there).
int bve_transform(const void* h, int n, const uint8_t* desc, int levelsup, uint32_t* word_id, double* word_value,
                  uint32_t* node_id, int32_t* node_begin, uint32_t* feat, int32_t* counts) {
    const Voc& V = *static_cast<const Voc*>(h);
    std::map<uint32_t, double> v;
    std::map<uint32_t, std::vector<uint32_t>> fv;
    const int nid_level = V.L - levelsup;
    for (int i = 0; i < n; ++i) {
        uint64_t q[4];
        std::memcpy(q, desc + 32 * (size_t)i, 32);
        uint32_t cur = 0, nid = 0;
        bool have = nid_level <= 0;
        int level = 0;
        do {
            ++level;
            const std::vector<uint32_t>& ch = V.nodes[cur].children;
            cur = ch[0];
            int best = distance(q, V.nodes[cur].d);
            for (size_t c = 1; c < ch.size(); ++c) {
                const int d = distance(q, V.nodes[ch[c]].d);
                if (d < best) {
                    best = d;
                    cur = ch[c];
                }
            }
            if (level == nid_level) {
                nid = cur;
                have = true;
            }
        } while (!V.nodes[cur].children.empty());
        if (!have) return -1;
        const double w = V.nodes[cur].weight;
        if (w > 0) {
            auto it = v.lower_bound(V.nodes[cur].word_id);
            if (it != v.end() && it->first == V.nodes[cur].word_id)
                it->second += w;
            else
                v.insert(it, {V.nodes[cur].word_id, w});
            fv[nid].push_back((uint32_t)i);
        }
    }
    double norm = 0.0;
    for (auto& e : v) norm += std::fabs(e.second);
    if (norm > 0.0)
        for (auto& e : v) e.second /= norm;
    int k = 0;
    for (auto& e : v) {
        word_id[k] = e.first;
        word_value[k++] = e.second;
    }
    counts[0] = k;
    int j = 0, at = 0;
    for (auto& e : fv) {
        node_id[j] = e.first;
        node_begin[j++] = at;
        for (uint32_t f : e.second) feat[at++] = f;
    }
    node_begin[j] = at;
    counts[1] = j;
    return 0;
}
}

#ifdef BVE_MAIN
#include <cstdio>
// A k = 3, L = 3 tree and 200 pseudo-random descriptors: exercises every path under the sanitizers.
int main() {
    std::vector<int32_t> parent{0};
    std::vector<int> level_begin{0, 1};
    for (int l = 1; l <= 3; ++l) {
        for (int p = level_begin[l - 1]; p < level_begin[l]; ++p)
            for (int c = 0; c < 3; ++c) parent.push_back(p);
        level_begin.push_back((int)parent.size());
    }
    const int nn = (int)parent.size();
    std::vector<uint8_t> leaf((size_t)nn, 0), desc(32 * (size_t)nn);
    std::vector<double> w((size_t)nn, 0.0);
    uint32_t s = 12345;
    auto rnd = [&] { s = s * 1664525u + 1013904223u; return (uint8_t)(s >> 24); };
    for (auto& b : desc) b = rnd();
    for (int i = level_begin[3]; i < nn; ++i) { leaf[i] = 1; w[i] = (i % 5) ? 0.1 * (i % 7 + 1) : 0.0; }
    void* h = bve_create(3, nn, parent.data(), leaf.data(), desc.data(), w.data());
    const int n = 200;
    std::vector<uint8_t> q(32 * (size_t)n);
    for (auto& b : q) b = rnd();
    std::vector<uint32_t> wid(n), nid(n), feat(n);
    std::vector<double> wv(n);
    std::vector<int32_t> nb(n + 1);
    int32_t counts[2];
    for (int lu = 0; lu <= 4; ++lu) {
        if (bve_transform(h, n, q.data(), lu, wid.data(), wv.data(), nid.data(), nb.data(), feat.data(), counts)) return 1;
        double sum = 0;
        for (int i = 0; i < counts[0]; ++i) sum += wv[i];
        std::printf("levelsup %d: words %d nodes %d entries %d sum %.17g\n", lu, counts[0], counts[1], nb[counts[1]], sum);
    }
    bve_destroy(h);
    return 0;
}
#endif
