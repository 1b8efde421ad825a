// Drives rsc_orb::ORBmatcher::SearchByProjection(Frame&, KeyFrame, sAlreadyFound, th, ORBdist) with mock
// Frame / KeyFrame / MapPoint types built from a binary file written by tests/test_gpu_reloc_refined.py,
// and writes the return value and CurrentFrame.mvpMapPoints (as MapPoint ids) of every call back: first
// each problem through the single-call form, then the problems whose orientation setting is `true`
// through one SearchByProjectionMany call.  Needs a GPU.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <set>
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
    int id = -1; bool bad = false; Vec3 X{}; DescMat d; float dmax = 0, dmin = 0;
    bool isBad() const { return bad; }
    Vec3 GetWorldPos() const { return X; }
    DescMat GetDescriptor() const { return d; }
    float GetMaxDistance() const { return dmax; }
    float GetMinDistance() const { return dmin; }
};
using MPPtr = std::shared_ptr<MapPoint>;
// Sophus::SE3f stand-in: rotation() / translation()
struct SE3 {
    Mat3 R; Vec3 t;
    Mat3 rotation() const { return R; }
    Vec3 translation() const { return t; }
};
struct Frame {
    int N = 0; std::vector<KeyPoint> mvKeysUn; DescMat mDescriptors;
    std::vector<std::size_t> mGrid[64][48];
    float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0, mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    std::vector<float> mvScaleFactors; int mnScaleLevels = 0; float mfLogScaleFactor = 0;
    SE3 mTcw;
    std::vector<MPPtr> mvpMapPoints;
};
struct KeyFrame {
    int N = 0; std::vector<KeyPoint> mvKeysUn; DescMat mDescriptors;
    int mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;
    float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0, fx = 0, fy = 0, cx = 0, cy = 0;
    std::vector<float> mvScaleFactors; int mnScaleLevels = 0; float mfLogScaleFactor = 0;
    Mat3 R{}; Vec3 t{};
    std::vector<std::vector<std::vector<std::size_t>>> grid;
    std::vector<MPPtr> mps;
    std::vector<MPPtr> GetMapPointMatches() const { return mps; }
    const std::vector<std::vector<std::vector<std::size_t>>>& GetGrid() const { return grid; }
    Mat3 GetRotation() const { return R; }
    Vec3 GetTranslation() const { return t; }
};

struct Reader {
    std::vector<uint8_t> buf; size_t pos = 0;
    template <class T> T get() { T v; std::memcpy(&v, buf.data() + pos, sizeof(T)); pos += sizeof(T); return v; }
    template <class T> std::vector<T> arr(size_t n) {
        std::vector<T> v(n);
        if (n) std::memcpy(v.data(), buf.data() + pos, n * sizeof(T));
        pos += n * sizeof(T);
        return v;
    }
};

struct Problem {
    Frame F; std::shared_ptr<KeyFrame> K; std::set<MPPtr> found; float th; int orb_dist, check;
    std::vector<MPPtr> entry;  // mvpMapPoints before the call
};

static Problem read_problem(Reader& r) {
    Problem p;
    Frame& F = p.F;
    const int nf = r.get<int32_t>(), nk = r.get<int32_t>();
    F.N = nf;
    F.fx = r.get<float>(); F.fy = r.get<float>(); F.cx = r.get<float>(); F.cy = r.get<float>();
    F.mnMinX = r.get<float>(); F.mnMaxX = r.get<float>(); F.mnMinY = r.get<float>(); F.mnMaxY = r.get<float>();
    F.mfGridElementWidthInv = r.get<float>(); F.mfGridElementHeightInv = r.get<float>();
    F.mnScaleLevels = r.get<int32_t>();
    F.mvScaleFactors = r.arr<float>((size_t)F.mnScaleLevels);
    F.mfLogScaleFactor = r.get<float>();
    const auto T = r.arr<float>(16);
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) F.mTcw.R.m[a][b] = T[4 * a + b];
        F.mTcw.t.v[a] = T[4 * a + 3];
    }
    const auto kp = r.arr<float>(2 * (size_t)nf);
    const auto oct = r.arr<int32_t>((size_t)nf);
    const auto ang = r.arr<float>((size_t)nf);
    F.mDescriptors.d = r.arr<uint8_t>(32 * (size_t)nf);
    F.mvKeysUn.resize((size_t)nf);
    for (int i = 0; i < nf; ++i) F.mvKeysUn[i] = KeyPoint{{kp[2 * i], kp[2 * i + 1]}, oct[i], ang[i]};
    const auto cb = r.arr<int32_t>(64 * 48 + 1);
    const auto cf = r.arr<int32_t>((size_t)cb[64 * 48]);
    for (int ix = 0; ix < 64; ++ix)
        for (int iy = 0; iy < 48; ++iy)
            for (int e = cb[ix * 48 + iy]; e < cb[ix * 48 + iy + 1]; ++e) F.mGrid[ix][iy].push_back((std::size_t)cf[e]);
    const auto fmp = r.arr<int32_t>((size_t)nf);
    F.mvpMapPoints.assign((size_t)nf, nullptr);
    for (int i = 0; i < nf; ++i)
        if (fmp[i] >= 0) {  // a MapPoint the Frame already holds (any MapPoint: only its presence is read)
            F.mvpMapPoints[i] = std::make_shared<MapPoint>();
            F.mvpMapPoints[i]->id = fmp[i];
        }
    p.entry = F.mvpMapPoints;
    auto K = std::make_shared<KeyFrame>();
    K->N = nk;
    K->fx = F.fx; K->fy = F.fy; K->cx = F.cx; K->cy = F.cy;
    K->mnMaxX = 752; K->mnMaxY = 480;
    K->mfGridElementWidthInv = F.mfGridElementWidthInv; K->mfGridElementHeightInv = F.mfGridElementHeightInv;
    K->mvScaleFactors = F.mvScaleFactors; K->mnScaleLevels = F.mnScaleLevels; K->mfLogScaleFactor = F.mfLogScaleFactor;
    for (int a = 0; a < 3; ++a) K->R.m[a][a] = 1.f;
    K->grid.assign(64, std::vector<std::vector<std::size_t>>(48));
    const auto kang = r.arr<float>((size_t)nk);
    const auto state = r.arr<uint8_t>((size_t)nk);
    const auto pos = r.arr<float>(3 * (size_t)nk);
    const auto dmax = r.arr<float>((size_t)nk);
    const auto dmin = r.arr<float>((size_t)nk);
    const auto mdesc = r.arr<uint8_t>(32 * (size_t)nk);
    const auto already = r.arr<uint8_t>((size_t)nk);
    K->mvKeysUn.resize((size_t)nk);
    K->mDescriptors.d.assign(32 * (size_t)nk, 0);
    K->mps.assign((size_t)nk, nullptr);
    for (int i = 0; i < nk; ++i) {
        K->mvKeysUn[i] = KeyPoint{{0.f, 0.f}, 0, kang[i]};
        if (!state[i]) continue;
        auto m = std::make_shared<MapPoint>();
        m->id = i;
        m->bad = state[i] == 2;
        m->X = Vec3{{pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]}};
        m->dmax = dmax[i];
        m->dmin = dmin[i];
        m->d.d.assign(mdesc.begin() + 32 * (size_t)i, mdesc.begin() + 32 * (size_t)(i + 1));
        K->mps[i] = m;
        if (already[i]) p.found.insert(m);
    }
    p.K = K;
    p.th = r.get<float>();
    p.orb_dist = r.get<int32_t>();
    p.check = r.get<int32_t>();
    return p;
}

static void write_result(FILE* f, int n, const Frame& F) {
    std::vector<int32_t> out(1 + (size_t)F.N);
    out[0] = n;
    for (int i = 0; i < F.N; ++i) out[1 + i] = F.mvpMapPoints[i] ? F.mvpMapPoints[i]->id : -1;
    std::fwrite(out.data(), 4, out.size(), f);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    Reader r;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    r.buf.resize((size_t)std::ftell(f));
    std::fseek(f, 0, SEEK_SET);
    if (std::fread(r.buf.data(), 1, r.buf.size(), f) != r.buf.size()) return 2;
    std::fclose(f);
    const int count = r.get<int32_t>();
    std::vector<Problem> ps;
    for (int c = 0; c < count; ++c) ps.push_back(read_problem(r));
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    try {
        for (Problem& p : ps) {
            rsc_orb::ORBmatcher matcher(0.9f, p.check != 0);
            const int n = matcher.SearchByProjection(p.F, p.K, p.found, p.th, p.orb_dist);
            write_result(o, n, p.F);
            p.F.mvpMapPoints = p.entry;
        }
        // the Many form: the problems matched with the orientation check (they share th / ORBdist) in one launch
        std::vector<Frame*> fr;
        std::vector<std::shared_ptr<KeyFrame>> kf;
        std::vector<const std::set<MPPtr>*> s;
        for (Problem& p : ps) {
            if (!p.check) continue;
            fr.push_back(&p.F);
            kf.push_back(p.K);
            s.push_back(&p.found);
        }
        if (!fr.empty()) {
            rsc_orb::ORBmatcher matcher(0.9f, true);
            const Problem* first = nullptr;
            for (const Problem& p : ps)
                if (p.check && !first) first = &p;
            const std::vector<int> n = matcher.SearchByProjectionMany(fr, kf, s, first->th, first->orb_dist);
            for (size_t c = 0; c < fr.size(); ++c) write_result(o, n[c], *fr[c]);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "facade_proj_test: %s\n", e.what());
        return 1;
    }
    std::fclose(o);
    return 0;
}
