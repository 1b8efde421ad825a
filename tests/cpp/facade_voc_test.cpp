// Drives rsc_orb::ORBVocabulary (csrc/facade/ORBVocabulary.hpp) on files written by the tests.
//   facade_voc_test parse <voc.txt>
//       host only (tests/test_cpu_bowvoc.py): parses the text vocabulary and prints the header and
//       one line per node, for the test to compare with what it wrote.
//   facade_voc_test device <voc.txt> <desc.bin> <levelsup> <out.txt>
//       needs a GPU (tests/test_gpu_bowvoc.py): loads the vocabulary, transforms the descriptors of
//       desc.bin (32 bytes each) into a std::map BowVector / FeatureVector and writes them as text,
//       the doubles as their 64 bits.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "ORBVocabulary.hpp"

struct Desc {  // a 1 x 32 CV_8U row
    uint8_t b[32];
    template <class T> const T* ptr(int) const { return reinterpret_cast<const T*>(b); }
};

int main(int argc, char** argv) {
    using rsc_orb::ORBVocabulary;
    if (argc >= 3 && !std::strcmp(argv[1], "parse")) {
        ORBVocabulary::Nodes n;
        if (!ORBVocabulary::parseTextFile(argv[2], n)) {
            std::printf("parse failed\n");
            return 2;
        }
        std::printf("%d %d %d %d %d\n", n.k, n.L, n.scoring, n.weighting, n.size());
        for (int i = 1; i < n.size(); ++i) {
            std::printf("%d %d", n.parent[i], (int)n.is_leaf[i]);
            for (int j = 0; j < 32; ++j) std::printf(" %d", (int)n.desc[32 * (size_t)i + j]);
            uint64_t bits;
            std::memcpy(&bits, &n.weight[i], 8);
            std::printf(" %016llx\n", (unsigned long long)bits);
        }
        return 0;
    }
    if (argc >= 6 && !std::strcmp(argv[1], "device")) {
        try {
            ORBVocabulary voc;
            if (!voc.loadFromTextFile(argv[2])) {
                std::printf("load failed\n");
                return 2;
            }
            std::vector<Desc> features;
            if (FILE* f = std::fopen(argv[3], "rb")) {
                Desc d;
                while (std::fread(d.b, 1, 32, f) == 32) features.push_back(d);
                std::fclose(f);
            } else {
                return 2;
            }
            std::map<unsigned int, double> bow;
            std::map<unsigned int, std::vector<unsigned int>> fv;
            voc.transform(features, bow, fv, std::atoi(argv[4]));
            FILE* o = std::fopen(argv[5], "w");
            if (!o) return 2;
            std::fprintf(o, "size %u features %zu\n", voc.size(), features.size());
            for (auto& e : bow) {
                uint64_t bits;
                std::memcpy(&bits, &e.second, 8);
                std::fprintf(o, "W %u %016llx\n", e.first, (unsigned long long)bits);
            }
            for (auto& e : fv) {
                std::fprintf(o, "N %u", e.first);
                for (unsigned int x : e.second) std::fprintf(o, " %u", x);
                std::fprintf(o, "\n");
            }
            std::fclose(o);
            std::printf("facade_voc_test device: ok\n");
            return 0;
        } catch (const std::exception& e) {
            std::printf("error: %s\n", e.what());
            return 1;
        }
    }
    std::printf("usage: facade_voc_test parse <voc.txt> | device <voc.txt> <desc.bin> <levelsup> <out.txt>\n");
    return 64;
}
