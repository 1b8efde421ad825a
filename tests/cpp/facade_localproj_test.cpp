// Drives rsc_orb::SearchLocalPoints(F, vpLocalMapPoints, th, nnratio) and
// rsc_orb::ORBmatcher::SearchByProjection(F, vpMapPoints, th) with mock Frame / MapPoint types built from a
// binary file written by tests/test_gpu_facade_localproj.py, and writes the results back: the return values,
// F.mvpMapPoints as MapPoint ids, and every MapPoint's track members and visible count.  Per problem: first
// the helper on fresh objects, then the bare overload on fresh objects that carry the track members the
// helper left (mbTrackInView false on the points the caller's first loop has seen).  Needs a GPU.
#include <cstdint>
#include <cstdio>
#include <cstring>
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
    int id = -1; bool bad = false; Vec3 X{}, N{}; DescMat d; float dmax = 0, dmin = 0;
    int nobs = 0, visible = 0;
    long unsigned int mnLastFrameSeen = 0;
    // include/MapPoint.hpp: variables used by the tracking
    float mTrackProjX = 0, mTrackProjY = 0, mTrackProjXR = 0;
    bool mbTrackInView = true;  // stale on purpose: the helper must write false where isInFrustum says so
    int mnTrackScaleLevel = 0;
    float mTrackViewCos = 0;
    bool isBad() const { return bad; }
    int Observations() const { return nobs; }
    void IncreaseVisible(int n = 1) { visible += n; }
    Vec3 GetWorldPos() const { return X; }
    Vec3 GetNormal() const { return N; }
    DescMat GetDescriptor() const { return d; }
    float GetMaxDistance() const { return dmax; }
    float GetMinDistance() const { return dmin; }
};
using MPPtr = std::shared_ptr<MapPoint>;
// Eigen::Isometry3f stand-in: rotation() / translation()
struct Iso {
    Mat3 R; Vec3 t;
    Mat3 rotation() const { return R; }
    Vec3 translation() const { return t; }
};
struct Frame {
    int N = 0; long unsigned int mnId = 7;
    std::vector<KeyPoint> mvKeysUn; DescMat mDescriptors;
    float mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;
    float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0, fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    std::vector<float> mvScaleFactors, mvuRight; int mnScaleLevels = 0; float mfLogScaleFactor = 0;
    Iso mTcw{};
    std::vector<std::size_t> mGrid[64][48];
    std::vector<MPPtr> mvpMapPoints;
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
    std::vector<uint8_t> state, desc, has_obs, skip, occ;
    std::vector<float> pos, nrm, dmax, dmin;
    std::shared_ptr<Frame> F;  // without mvpMapPoints
    float th = 1, nn = 0.8f;
    int np = 0;
};

static Problem read_problem(Reader& r) {
    Problem p;
    const int np = p.np = r.get<int32_t>();
    p.state = r.arr<uint8_t>((size_t)np);
    p.pos = r.arr<float>(3 * (size_t)np);
    p.nrm = r.arr<float>(3 * (size_t)np);
    p.dmax = r.arr<float>((size_t)np);
    p.dmin = r.arr<float>((size_t)np);
    p.desc = r.arr<uint8_t>(32 * (size_t)np);
    p.has_obs = r.arr<uint8_t>((size_t)np);
    p.skip = r.arr<uint8_t>((size_t)np);
    auto F = std::make_shared<Frame>();
    const int nf = F->N = r.get<int32_t>();
    F->fx = r.get<float>(); F->fy = r.get<float>(); F->cx = r.get<float>(); F->cy = r.get<float>();
    F->mnMinX = r.get<float>(); F->mnMaxX = r.get<float>(); F->mnMinY = r.get<float>(); F->mnMaxY = r.get<float>();
    F->mfGridElementWidthInv = r.get<float>(); F->mfGridElementHeightInv = r.get<float>();
    F->mnScaleLevels = r.get<int32_t>();
    F->mvScaleFactors = r.arr<float>((size_t)F->mnScaleLevels);
    F->mfLogScaleFactor = r.get<float>();
    const auto T = r.arr<float>(16);
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) F->mTcw.R.m[a][b] = T[4 * a + b];
        F->mTcw.t.v[a] = T[4 * a + 3];
    }
    const auto kp = r.arr<float>(2 * (size_t)nf);
    const auto oct = r.arr<int32_t>((size_t)nf);
    F->mDescriptors.d = r.arr<uint8_t>(32 * (size_t)nf);
    F->mvKeysUn.resize((size_t)nf);
    for (int i = 0; i < nf; ++i) F->mvKeysUn[i] = KeyPoint{{kp[2 * i], kp[2 * i + 1]}, oct[i], 0.f};
    const auto cb = r.arr<int32_t>(64 * 48 + 1);
    const auto cf = r.arr<int32_t>((size_t)cb[64 * 48]);
    for (int ix = 0; ix < 64; ++ix)
        for (int iy = 0; iy < 48; ++iy)
            for (int e = cb[ix * 48 + iy]; e < cb[ix * 48 + iy + 1]; ++e) F->mGrid[ix][iy].push_back((std::size_t)cf[e]);
    F->mvuRight = r.arr<float>((size_t)nf);
    F->mbf = r.get<float>();
    p.occ = r.arr<uint8_t>((size_t)nf);
    p.th = r.get<float>();
    p.nn = r.get<float>();
    p.F = F;
    return p;
}

static std::vector<MPPtr> make_points(const Problem& p, const Frame& F) {
    std::vector<MPPtr> pts((size_t)p.np);
    for (int i = 0; i < p.np; ++i) {
        auto m = std::make_shared<MapPoint>();
        m->id = i;
        m->bad = p.state[i] == 2;
        m->X = Vec3{{p.pos[3 * i], p.pos[3 * i + 1], p.pos[3 * i + 2]}};
        m->N = Vec3{{p.nrm[3 * i], p.nrm[3 * i + 1], p.nrm[3 * i + 2]}};
        m->dmax = p.dmax[i];
        m->dmin = p.dmin[i];
        m->d.d.assign(p.desc.begin() + 32 * (size_t)i, p.desc.begin() + 32 * (size_t)(i + 1));
        m->nobs = p.has_obs[i] ? 3 : 0;
        m->mnLastFrameSeen = p.skip[i] ? F.mnId : 0;
        pts[i] = m;
    }
    return pts;
}

// F.mvpMapPoints on entry: 0 NULL, 1 another MapPoint without observations, 2 one with
static void fill_slots(const Problem& p, Frame& F) {
    F.mvpMapPoints.assign((size_t)F.N, nullptr);
    for (int f = 0; f < F.N; ++f)
        if (p.occ[f]) {
            auto m = std::make_shared<MapPoint>();
            m->id = 1000000 + f;
            m->nobs = p.occ[f] == 2 ? 1 : 0;
            F.mvpMapPoints[f] = m;
        }
}

static void write_result(FILE* o, int n, int ntm, const Frame& F, const std::vector<MPPtr>& pts) {
    std::vector<int32_t> head(2 + (size_t)F.N);
    head[0] = n;
    head[1] = ntm;
    for (int f = 0; f < F.N; ++f) head[2 + f] = F.mvpMapPoints[f] ? F.mvpMapPoints[f]->id : -1;
    std::fwrite(head.data(), 4, head.size(), o);
    for (const auto& m : pts) {
        const int32_t iv = m->mbTrackInView, lv = m->mnTrackScaleLevel, vis = m->visible;
        std::fwrite(&iv, 4, 1, o);
        std::fwrite(&m->mTrackProjX, 4, 1, o);
        std::fwrite(&m->mTrackProjY, 4, 1, o);
        std::fwrite(&m->mTrackProjXR, 4, 1, o);
        std::fwrite(&lv, 4, 1, o);
        std::fwrite(&m->mTrackViewCos, 4, 1, o);
        std::fwrite(&vis, 4, 1, o);
    }
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
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    try {
        const int n_problems = r.get<int32_t>();
        for (int c = 0; c < n_problems; ++c) {
            Problem p = read_problem(r);
            Frame& F = *p.F;
            // Tracking::SearchLocalPoints from :1003 on
            std::vector<MPPtr> pts = make_points(p, F);
            fill_slots(p, F);
            int ntm = -1;
            const int n = rsc_orb::SearchLocalPoints(F, pts, p.th, p.nn, &ntm);
            write_result(o, n, ntm, F, pts);
            // the bare matcher on the members the helper left
            std::vector<MPPtr> pts2 = make_points(p, F);
            for (int i = 0; i < p.np; ++i) {
                pts2[i]->mbTrackInView = p.skip[i] ? false : pts[i]->mbTrackInView;  // Tracking.cpp:995
                pts2[i]->mTrackProjX = pts[i]->mTrackProjX;
                pts2[i]->mTrackProjY = pts[i]->mTrackProjY;
                pts2[i]->mTrackProjXR = pts[i]->mTrackProjXR;
                pts2[i]->mnTrackScaleLevel = pts[i]->mnTrackScaleLevel;
                pts2[i]->mTrackViewCos = pts[i]->mTrackViewCos;
            }
            fill_slots(p, F);
            rsc_orb::ORBmatcher matcher(p.nn);
            const int n2 = matcher.SearchByProjection(F, pts2, p.th);
            write_result(o, n2, -1, F, pts2);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "facade_localproj_test: %s\n", e.what());
        return 1;
    }
    std::fclose(o);
    return 0;
}
