// TEST INFRASTRUCTURE — this project's own main() around the reference's DBoW2, compiled unmodified from
// the reference tree (oracle/Makefile target `ref`, binary oracle/_ref/ref_dbow2).  It calls only the
// reference's public API and writes what it returns as raw little-endian binary: a double never
// passes through decimal text.  tests/ref_dbow2_io.py holds the readers and writers of these files.
//
//   ref_dbow2 load <voc.txt> <out>
//       u32 size(), u32 nl; then size x nl u32 getParentNode(w, l) for l = 0..nl-1 (l = 0 is the
//       word's node id; nl = getDepthLevels() + 2); then size doubles getWordWeight(w)
//   ref_dbow2 transform <voc.txt> <desc.bin> <levelsup> <out>
//       desc.bin: 32 bytes per feature.  u32 nw, nw u32 word ids, nw doubles (the BowVector in key
//       order); u32 nn, nn u32 node ids, nn+1 u32 begins, then the feature indices (FeatureVector)
//   ref_dbow2 score <a.bin> <b.bin> <out>
//       a.bin / b.bin: u32 n, n u32 ids, n doubles, inserted as given (no normalize).  One double:
//       L1Scoring::score(a, b); one float: the same through `float si = ...` (KeyFrameDatabase.cpp)
//   ref_dbow2 normalize <a.bin> <out>
//       the vector after BowVector::normalize(L1), in the layout of a.bin
//   ref_dbow2 randint <seed> <N> <minset> <count> <out>
//       srand(seed); count i32 draws RandomInt(0, N-1-j), j cycling over 0..minset-1
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "DBoW2/BowVector.h"
#include "DBoW2/FORB.h"
#include "DBoW2/FeatureVector.h"
#include "DBoW2/ScoringObject.h"
#include "DBoW2/TemplatedVocabulary.h"
#include "DUtils/Random.h"

typedef DBoW2::TemplatedVocabulary<DBoW2::FORB::TDescriptor, DBoW2::FORB> ORBVocabulary;

namespace {

struct Out {
    FILE* f;
    explicit Out(const char* path) : f(std::fopen(path, "wb")) {}
    ~Out() {
        if (f) std::fclose(f);
    }
    template <class T> void put(const T& x) { std::fwrite(&x, sizeof(T), 1, f); }
    void u32(uint32_t x) { put(x); }
};

bool read_all(const char* path, std::vector<unsigned char>& buf) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    unsigned char tmp[4096];
    size_t n;
    while ((n = std::fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
    std::fclose(f);
    return true;
}

bool read_bow(const char* path, DBoW2::BowVector& v) {
    std::vector<unsigned char> buf;
    if (!read_all(path, buf) || buf.size() < 4) return false;
    uint32_t n;
    std::memcpy(&n, buf.data(), 4);
    if (buf.size() != 4 + (size_t)n * 12) return false;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t id;
        double val;
        std::memcpy(&id, buf.data() + 4 + 4 * (size_t)i, 4);
        std::memcpy(&val, buf.data() + 4 + 4 * (size_t)n + 8 * (size_t)i, 8);
        v.insert(std::make_pair(id, val));
    }
    return v.size() == n;
}

void write_bow(Out& o, const DBoW2::BowVector& v) {
    o.u32((uint32_t)v.size());
    for (DBoW2::BowVector::const_iterator it = v.begin(); it != v.end(); ++it) o.u32(it->first);
    for (DBoW2::BowVector::const_iterator it = v.begin(); it != v.end(); ++it) o.put(it->second);
}

int usage() {
    std::fprintf(stderr, "usage: ref_dbow2 load|transform|score|normalize|randint ... <out>\n");
    return 64;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return usage();
    const std::string verb = argv[1];
    if (verb == "load" && argc == 4) {
        ORBVocabulary voc;
        if (!voc.loadFromTextFile(argv[2])) return 2;
        Out o(argv[3]);
        if (!o.f) return 3;
        const uint32_t size = voc.size(), nl = (uint32_t)voc.getDepthLevels() + 2;
        o.u32(size);
        o.u32(nl);
        for (uint32_t w = 0; w < size; ++w)
            for (uint32_t l = 0; l < nl; ++l) o.u32(voc.getParentNode(w, (int)l));
        for (uint32_t w = 0; w < size; ++w) o.put((double)voc.getWordWeight(w));
        return 0;
    }
    if (verb == "transform" && argc == 6) {
        ORBVocabulary voc;
        if (!voc.loadFromTextFile(argv[2])) return 2;
        std::vector<unsigned char> buf;
        if (!read_all(argv[3], buf) || buf.size() % 32) return 2;
        std::vector<cv::Mat> features(buf.size() / 32);
        for (size_t i = 0; i < features.size(); ++i) {
            features[i].create(1, 32, CV_8U);
            std::memcpy(features[i].ptr<unsigned char>(), buf.data() + 32 * i, 32);
        }
        DBoW2::BowVector v;
        DBoW2::FeatureVector fv;
        voc.transform(features, v, fv, std::atoi(argv[4]));
        Out o(argv[5]);
        if (!o.f) return 3;
        write_bow(o, v);
        o.u32((uint32_t)fv.size());
        for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) o.u32(it->first);
        uint32_t begin = 0;
        o.u32(begin);
        for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it)
            o.u32(begin += (uint32_t)it->second.size());
        for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it)
            for (size_t j = 0; j < it->second.size(); ++j) o.u32(it->second[j]);
        return 0;
    }
    if (verb == "score" && argc == 5) {
        DBoW2::BowVector a, b;
        if (!read_bow(argv[2], a) || !read_bow(argv[3], b)) return 2;
        Out o(argv[4]);
        if (!o.f) return 3;
        const DBoW2::L1Scoring l1;
        const double s = l1.score(a, b);
        float si = s;  // KeyFrameDatabase.cpp: float si = mpVoc->score(...)
        o.put(s);
        o.put(si);
        return 0;
    }
    if (verb == "normalize" && argc == 4) {
        DBoW2::BowVector a;
        if (!read_bow(argv[2], a)) return 2;
        a.normalize(DBoW2::L1);
        Out o(argv[3]);
        if (!o.f) return 3;
        write_bow(o, a);
        return 0;
    }
    if (verb == "randint" && argc == 7) {
        const int seed = std::atoi(argv[2]), N = std::atoi(argv[3]), minset = std::atoi(argv[4]);
        const int count = std::atoi(argv[5]);
        if (N < minset || minset < 1 || count < 0) return 2;
        Out o(argv[6]);
        if (!o.f) return 3;
        srand((unsigned)seed);
        for (int i = 0; i < count; ++i) o.put((int32_t)DUtils::Random::RandomInt(0, N - 1 - i % minset));
        return 0;
    }
    return usage();
}
