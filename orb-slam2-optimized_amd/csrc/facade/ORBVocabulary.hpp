// ORBVocabulary.hpp — drop-in facade of ORB_SLAM_CUSTOM::ORBVocabulary (DBoW2
// TemplatedVocabulary<FORB::TDescriptor, FORB>, Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h) over the
// rsc C ABI, for the calls ORB-SLAM2 makes: loadFromTextFile (System.cpp), size() (KeyFrameDatabase)
// and transform(features, BowVector, FeatureVector, levelsup) (Frame::ComputeBoW, KeyFrame::ComputeBoW).
// The tree is uploaded once (rsc_voc_create); every transform runs on the MI355X and fills the
// caller's std::map-shaped vectors with the reference's keys, values (bit for bit) and order.
//
// Descriptor needs ptr<uint8_t>(0) giving its 32 bytes (cv::Mat rows as the reference stores them).
// BowVec is a std::map<WordId, WordValue>, FeatVec a std::map<NodeId, std::vector<unsigned int>>
// (DBoW2::BowVector, DBoW2::FeatureVector).
//
// Loader: the reference's `while(!f.eof())` (:1378) turns the file's trailing newline into one more
// node whose parent and nIsLeaf are uninitialised reads (Q21 in DESIGN.md).  As built with gcc it is
// one more child of the last line's parent and a WORD of weight 0 with an unwritten descriptor; this
// loader skips empty lines, so that node does not exist here and size() is ONE LESS than the
// reference's for such a file (the missing word has weight 0: no feature can score with it).  A
// caller that wants to model it appends the node to Nodes (the last line's parent, is_leaf 1, weight
// 0, a descriptor of its choice) and calls upload().
// Only TF_IDF weighting with L1_NORM scoring (what ORBvoc.txt declares) is supported.
// One mutex serialises transform(): Tracking and LocalMapping share the vocabulary.  In the reference tree:
//     mpVocabulary = new rsc_orb::ORBVocabulary();  mpVocabulary->loadFromTextFile(strVocFile);
#pragma once
#include <cstdint>
#include <fstream>
#include <mutex>
#include <sstream>
#include <string>
#include <vector>
#include "rsc_context.hpp"

namespace rsc_orb {

class ORBVocabulary {
public:
    // The tree as the text file lists it; node 0 is the root.
    struct Nodes {
        int k = 0, L = 0, scoring = 0, weighting = 0;
        std::vector<int32_t> parent{0};
        std::vector<uint8_t> is_leaf{0};
        std::vector<uint8_t> desc = std::vector<uint8_t>(32, 0);
        std::vector<double> weight{0.0};
        int size() const { return (int)parent.size(); }
    };

    ORBVocabulary() = default;
    ORBVocabulary(const ORBVocabulary&) = delete;
    ORBVocabulary& operator=(const ORBVocabulary&) = delete;
    ~ORBVocabulary() { release(); }

    // Host-only parse of the ORBvoc.txt format: the header line `k L scoring weighting`, then one
    // line per node: `parent isLeaf b0 .. b31 weight`.  Returns false on a malformed file (the
    // reference's header check, :1359, plus per-line checks it does not make).
    static bool parseTextFile(const std::string& filename, Nodes& out) {
        std::ifstream f(filename.c_str());
        if (!f) return false;
        Nodes n;
        std::string line;
        if (!std::getline(f, line)) return false;
        {
            std::stringstream ss(line);
            if (!(ss >> n.k >> n.L >> n.scoring >> n.weighting)) return false;
            if (n.k < 0 || n.k > 20 || n.L < 1 || n.L > 10 || n.scoring < 0 || n.scoring > 5 || n.weighting < 0 ||
                n.weighting > 3)
                return false;
        }
        while (std::getline(f, line)) {
            if (line.find_first_not_of(" \t\r") == std::string::npos) continue;  // empty: see the header comment
            std::stringstream ss(line);
            int pid = 0, leaf = 0;
            if (!(ss >> pid >> leaf)) return false;
            if (pid < 0 || pid >= n.size()) return false;
            for (int i = 0; i < 32; ++i) {
                int b = 0;
                if (!(ss >> b) || b < 0 || b > 255) return false;
                n.desc.push_back((uint8_t)b);
            }
            double w = 0;
            if (!(ss >> w)) return false;
            n.parent.push_back(pid);
            n.is_leaf.push_back(leaf > 0 ? 1 : 0);
            n.weight.push_back(w);
        }
        if (n.size() < 2) return false;
        out = std::move(n);
        return true;
    }

    bool loadFromTextFile(const std::string& filename) {
        Nodes n;
        if (!parseTextFile(filename, n)) return false;
        upload(n);
        return true;
    }

    // Uploads a tree (replacing the resident one).
    void upload(const Nodes& n) {
        std::lock_guard<std::mutex> lock(mutex_);
        release();
        check(rsc_context_create(device(), &ctx_), "rsc_context_create");
        rsc_vocabulary_nodes v{};
        v.k = n.k;
        v.L = n.L;
        v.scoring = n.scoring;
        v.weighting = n.weighting;
        v.n_nodes = n.size();
        v.parent = n.parent.data();
        v.is_leaf = n.is_leaf.data();
        v.desc = n.desc.data();
        v.weight = n.weight.data();
        check(rsc_voc_create(ctx_, &v, &voc_), "rsc_voc_create");
        check(rsc_voc_size(voc_, &words_), "rsc_voc_size");
    }

    bool empty() const { return voc_ == nullptr; }
    unsigned int size() const { return words_; }

    // transform(features, v, fv, levelsup) (:1127-1194)
    template <class Descriptor, class BowVec, class FeatVec>
    void transform(const std::vector<Descriptor>& features, BowVec& v, FeatVec& fv, int levelsup) {
        v.clear();
        fv.clear();
        if (empty()) return;
        std::lock_guard<std::mutex> lock(mutex_);
        const int32_t n = (int32_t)features.size();
        bytes_.resize(32 * (size_t)n);
        for (int32_t i = 0; i < n; ++i) {
            const uint8_t* p = features[i].template ptr<uint8_t>(0);
            std::copy(p, p + 32, bytes_.begin() + 32 * (size_t)i);
        }
        const size_t room = (size_t)n + 1;
        word_id_.resize(room);
        word_value_.resize(room);
        node_id_.resize(room);
        node_begin_.resize(room + 1);
        feat_.resize(room);
        rsc_voc_output o{};
        o.word_id = word_id_.data();
        o.word_value = word_value_.data();
        o.node_id = node_id_.data();
        o.node_begin = node_begin_.data();
        o.feat = feat_.data();
        const uint8_t* d = bytes_.data();
        check(rsc_voc_transform_many(voc_, 1, &n, &d, levelsup, &o), "ORBVocabulary::transform");
        for (int i = 0; i < o.n_words; ++i)
            v.insert(v.end(), typename BowVec::value_type(word_id_[i], word_value_[i]));
        for (int j = 0; j < o.n_nodes; ++j) {
            auto it = fv.insert(fv.end(), typename FeatVec::value_type(node_id_[j], typename FeatVec::mapped_type()));
            it->second.assign(feat_.begin() + node_begin_[j], feat_.begin() + node_begin_[j + 1]);
        }
    }

    rsc_voc* handle() const { return voc_; }

private:
    static int device() {
        const char* d = std::getenv("RSC_DEVICE");
        return d ? std::atoi(d) : 0;
    }
    void release() {
        if (voc_) rsc_voc_destroy(voc_);
        if (ctx_) rsc_context_destroy(ctx_);
        voc_ = nullptr;
        ctx_ = nullptr;
        words_ = 0;
    }

    rsc_context* ctx_ = nullptr;
    rsc_voc* voc_ = nullptr;
    uint32_t words_ = 0;
    std::mutex mutex_;
    std::vector<uint8_t> bytes_;
    std::vector<uint32_t> word_id_, node_id_, feat_;
    std::vector<double> word_value_;
    std::vector<int32_t> node_begin_;
};

}  // namespace rsc_orb
