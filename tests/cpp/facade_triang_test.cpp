// Drives rsc_orb::ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) with mock
// KeyFrame / MapPoint types built from the case file tests/triang_emu_lib.py writes (the one the emulation's
// stand-alone program reads), and writes per case the return value and vMatchedPairs, which enters every call
// holding one sentinel pair: a call that returns at den == 0 must leave it there.  Needs a GPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>
#include "ORBmatcher.hpp"

struct Vec3 { float v[3]; float operator()(int i) const { return v[i]; } };
struct Mat3 { float m[3][3]; float operator()(int r, int c) const { return m[r][c]; } };
struct Pt { float x, y; };
struct KeyPoint { Pt pt; int octave; float angle; };
struct DescMat {
    std::vector<uint8_t> d;
    template <class T> const T* ptr(int row) const { return reinterpret_cast<const T*>(d.data() + 32 * (size_t)row); }
};
struct MapPoint {
    bool bad = false; DescMat d;
    bool isBad() const { return bad; }
    Vec3 GetWorldPos() const { return Vec3{}; }
    DescMat GetDescriptor() const { return d; }
    float GetMaxDistance() const { return 1.0f; }
    float GetMinDistance() const { return 1.0f; }
};
using MPPtr = std::shared_ptr<MapPoint>;
struct Iso {
    Mat3 R; Vec3 t;
    Mat3 rotation() const { return R; }
    Vec3 translation() const { return t; }
};
struct KeyFrame {
    int N = 0; std::vector<KeyPoint> mvKeysUn, mvKeys; DescMat mDescriptors;
    std::vector<float> mvuRight, mvDepth;
    std::map<unsigned, std::vector<unsigned>> mFeatVec;
    int mnMinX = 0, mnMinY = 0, mnMaxX = 640, mnMaxY = 480;
    float mfGridElementWidthInv = 0.1f, mfGridElementHeightInv = 0.1f, fx = 0, fy = 0, cx = 0, cy = 0;
    float invfx = 0, invfy = 0, mb = 0, mbf = 0, mfScaleFactor = 0;
    std::vector<float> mvScaleFactors; int mnScaleLevels = 0; float mfLogScaleFactor = 0.18232156f;
    Mat3 R{}, mKinv{}; Vec3 t{}; Iso Twc{};
    std::vector<std::vector<std::vector<std::size_t>>> grid;
    std::vector<MPPtr> mps;
    std::vector<MPPtr> GetMapPointMatches() const { return mps; }
    const std::vector<std::vector<std::vector<std::size_t>>>& GetGrid() const { return grid; }
    Mat3 GetRotation() const { return R; }
    Vec3 GetTranslation() const { return t; }
    Iso GetPoseInverse() const { return Twc; }
};

struct Reader {
    std::vector<char> buf;
    size_t off = 0;
    template <class T> const T* take(size_t n) {
        const size_t bytes = (n * sizeof(T) + 7) & ~(size_t)7;
        if (off + bytes > buf.size()) { std::fprintf(stderr, "case file truncated\n"); std::exit(2); }
        const T* p = reinterpret_cast<const T*>(buf.data() + off);
        off += bytes;
        return p;
    }
    int32_t word() { return *take<int32_t>(1); }
};

static std::shared_ptr<KeyFrame> read_kf(Reader& r) {
    auto k = std::make_shared<KeyFrame>();
    const int n = r.word(), nn = r.word(), nl = r.word(), nf = r.word();
    k->N = n;
    const float* kp = r.take<float>(2 * (size_t)n);
    const float* raw = r.take<float>(2 * (size_t)n);
    const int32_t* oct = r.take<int32_t>((size_t)n);
    const uint8_t* desc = r.take<uint8_t>(32 * (size_t)n);
    const float* ang = r.take<float>((size_t)n);
    const float* ur = r.take<float>((size_t)n);
    const float* dp = r.take<float>((size_t)n);
    (void)r.take<float>((size_t)n);  // the caller's cosine: the facade evaluates its own
    const uint8_t* st = r.take<uint8_t>((size_t)n);
    const uint32_t* id = r.take<uint32_t>((size_t)nn);
    const int32_t* beg = r.take<int32_t>((size_t)nn + 1);
    const uint32_t* feat = r.take<uint32_t>((size_t)nf);
    const float* sc = r.take<float>((size_t)nl);
    const float* s = r.take<float>(42);
    k->mDescriptors.d.assign(desc, desc + 32 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        k->mvKeysUn.push_back(KeyPoint{Pt{kp[2 * i], kp[2 * i + 1]}, oct[i], ang[i]});
        k->mvKeys.push_back(KeyPoint{Pt{raw[2 * i], raw[2 * i + 1]}, oct[i], ang[i]});
        MPPtr mp;
        if (st[i]) {
            mp = std::make_shared<MapPoint>();
            mp->bad = st[i] == 2;
            mp->d.d.assign(32, 0);
        }
        k->mps.push_back(mp);
    }
    k->mvuRight.assign(ur, ur + n);
    k->mvDepth.assign(dp, dp + n);
    for (int j = 0; j < nn; ++j) k->mFeatVec[id[j]].assign(feat + beg[j], feat + beg[j + 1]);
    k->mvScaleFactors.assign(sc, sc + nl);
    k->mnScaleLevels = nl;
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) {
            k->R.m[a][b] = s[3 * a + b];
            k->Twc.R.m[a][b] = s[12 + 3 * a + b];
            k->mKinv.m[a][b] = s[33 + 3 * a + b];
        }
        k->t.v[a] = s[9 + a];
        k->Twc.t.v[a] = s[21 + a];
    }
    k->fx = s[24]; k->fy = s[25]; k->cx = s[26]; k->cy = s[27]; k->invfx = s[28]; k->invfy = s[29];
    k->mb = s[30]; k->mbf = s[31]; k->mfScaleFactor = s[32];
    k->grid.assign(64, std::vector<std::vector<std::size_t>>(48));
    return k;
}

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
    Reader r;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    r.buf.resize((size_t)std::ftell(f));
    std::fseek(f, 0, SEEK_SET);
    if (std::fread(r.buf.data(), 1, r.buf.size(), f) != r.buf.size()) return 2;
    std::fclose(f);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const int ncases = r.word();
    for (int c = 0; c < ncases; ++c) {
        auto k1 = read_kf(r), k2 = read_kf(r);
        const float* F = r.take<float>(9);
        Mat3 F12;
        std::memcpy(F12.m, F, sizeof(F12.m));
        const int only_stereo = r.word(), check_ori = r.word(), npairs = r.word();
        (void)r.take<int32_t>(2 * (size_t)npairs);
        rsc_orb::ORBmatcher matcher(0.6f, check_ori != 0);
        std::vector<std::pair<size_t, size_t>> pairs(1, std::make_pair((size_t)7, (size_t)7));  // the sentinel
        const int32_t ret = matcher.SearchForTriangulation(k1, k2, F12, pairs, only_stereo != 0);
        const int32_t np = (int32_t)pairs.size();
        std::fwrite(&ret, 4, 1, o);
        std::fwrite(&np, 4, 1, o);
        for (const auto& p : pairs) {
            const int32_t ab[2] = {(int32_t)p.first, (int32_t)p.second};
            std::fwrite(ab, 4, 2, o);
        }
    }
    std::fclose(o);
    std::printf("%d cases\n", ncases);
    return 0;
}
