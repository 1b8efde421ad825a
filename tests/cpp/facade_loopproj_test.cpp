// Drives rsc_orb::ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) and
// rsc_orb::ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) with mock KeyFrame / MapPoint types built
// from a binary file written by tests/test_gpu_facade_loopproj.py, and writes the results back as MapPoint
// ids: first every problem through the single-call form, then all search problems through one
// SearchByProjectionMany call and all Fuse problems (they share one point list) through one FuseMany call.
// Needs a GPU.
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
struct KeyFrame;
struct MapPoint {
    int id = -1; bool bad = false; Vec3 X{}, N{}; DescMat d; float dmax = 0, dmin = 0;
    std::vector<std::pair<const KeyFrame*, int>> obs;
    bool isBad() const { return bad; }
    Vec3 GetWorldPos() const { return X; }
    Vec3 GetNormal() const { return N; }
    DescMat GetDescriptor() const { return d; }
    float GetMaxDistance() const { return dmax; }
    float GetMinDistance() const { return dmin; }
    void AddObservation(const std::shared_ptr<KeyFrame>& kf, int idx) { obs.emplace_back(kf.get(), idx); }
};
using MPPtr = std::shared_ptr<MapPoint>;
// Eigen::Isometry3f stand-in: rotation() / translation()
struct Iso {
    Mat3 R; Vec3 t;
    Mat3 rotation() const { return R; }
    Vec3 translation() const { return t; }
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
    std::set<MPPtr> GetMapPoints() const {
        std::set<MPPtr> s;
        for (const auto& m : mps)
            if (m && !m->isBad()) s.insert(m);
        return s;
    }
    MPPtr GetMapPoint(int idx) const { return mps[idx]; }
    void AddMapPoint(const MPPtr& m, int idx) { mps[idx] = m; }
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

static std::vector<MPPtr> read_points(Reader& r) {
    const int np = r.get<int32_t>();
    const auto state = r.arr<uint8_t>((size_t)np);
    const auto pos = r.arr<float>(3 * (size_t)np);
    const auto nrm = r.arr<float>(3 * (size_t)np);
    const auto dmax = r.arr<float>((size_t)np);
    const auto dmin = r.arr<float>((size_t)np);
    const auto desc = r.arr<uint8_t>(32 * (size_t)np);
    std::vector<MPPtr> pts((size_t)np);
    for (int i = 0; i < np; ++i) {
        auto m = std::make_shared<MapPoint>();
        m->id = i;
        m->bad = state[i] == 2;
        m->X = Vec3{{pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]}};
        m->N = Vec3{{nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]}};
        m->dmax = dmax[i];
        m->dmin = dmin[i];
        m->d.d.assign(desc.begin() + 32 * (size_t)i, desc.begin() + 32 * (size_t)(i + 1));
        pts[i] = m;
    }
    return pts;
}

// slot codes: -1 empty, -2 another good MapPoint, -3 another bad MapPoint, >= 0 the point of that index
static std::vector<MPPtr> slots_from(const std::vector<int32_t>& code, const std::vector<MPPtr>& pts) {
    std::vector<MPPtr> s(code.size(), nullptr);
    for (size_t i = 0; i < code.size(); ++i) {
        if (code[i] >= 0) s[i] = pts[code[i]];
        else if (code[i] <= -2) {
            s[i] = std::make_shared<MapPoint>();
            s[i]->id = 1000000 + (int)i;
            s[i]->bad = code[i] == -3;
            s[i]->d.d.assign(32, 0);  // a MapPoint always has a descriptor row (the KeyFrame view uploads it)
        }
    }
    return s;
}

struct Problem {
    std::shared_ptr<KeyFrame> K; Iso S; std::vector<int32_t> slots; float th;
};

static Problem read_problem(Reader& r, const std::vector<MPPtr>& pts) {
    Problem p;
    auto K = std::make_shared<KeyFrame>();
    const int nk = r.get<int32_t>();
    K->N = nk;
    K->fx = r.get<float>(); K->fy = r.get<float>(); K->cx = r.get<float>(); K->cy = r.get<float>();
    K->mnMinX = r.get<int32_t>(); K->mnMaxX = r.get<int32_t>(); K->mnMinY = r.get<int32_t>(); K->mnMaxY = r.get<int32_t>();
    K->mfGridElementWidthInv = r.get<float>(); K->mfGridElementHeightInv = r.get<float>();
    K->mnScaleLevels = r.get<int32_t>();
    K->mvScaleFactors = r.arr<float>((size_t)K->mnScaleLevels);
    K->mfLogScaleFactor = r.get<float>();
    const auto T = r.arr<float>(16);
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) p.S.R.m[a][b] = T[4 * a + b];
        p.S.t.v[a] = T[4 * a + 3];
        K->R.m[a][a] = 1.f;
    }
    const auto kp = r.arr<float>(2 * (size_t)nk);
    const auto oct = r.arr<int32_t>((size_t)nk);
    K->mDescriptors.d = r.arr<uint8_t>(32 * (size_t)nk);
    K->mvKeysUn.resize((size_t)nk);
    for (int i = 0; i < nk; ++i) K->mvKeysUn[i] = KeyPoint{{kp[2 * i], kp[2 * i + 1]}, oct[i], 0.f};
    const auto cb = r.arr<int32_t>(64 * 48 + 1);
    const auto cf = r.arr<int32_t>((size_t)cb[64 * 48]);
    K->grid.assign(64, std::vector<std::vector<std::size_t>>(48));
    for (int ix = 0; ix < 64; ++ix)
        for (int iy = 0; iy < 48; ++iy)
            for (int e = cb[ix * 48 + iy]; e < cb[ix * 48 + iy + 1]; ++e) K->grid[ix][iy].push_back((std::size_t)cf[e]);
    p.slots = r.arr<int32_t>((size_t)nk);
    K->mps.assign((size_t)nk, nullptr);
    p.th = r.get<float>();
    p.K = K;
    (void)pts;
    return p;
}

static void write_ids(FILE* f, int n, const std::vector<MPPtr>& v) {
    std::vector<int32_t> out(1 + v.size());
    out[0] = n;
    for (size_t i = 0; i < v.size(); ++i) out[1 + i] = v[i] ? v[i]->id : -1;
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
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    try {
        // ---- SearchByProjection: each problem has its own point list; slots = vpMatched on entry ----
        const int n_search = r.get<int32_t>();
        std::vector<std::vector<MPPtr>> pts((size_t)n_search);
        std::vector<Problem> sp;
        for (int c = 0; c < n_search; ++c) {
            pts[c] = read_points(r);
            sp.push_back(read_problem(r, pts[c]));
        }
        rsc_orb::ORBmatcher matcher(0.75f, true);
        for (int c = 0; c < n_search; ++c) {
            std::vector<MPPtr> matched = slots_from(sp[c].slots, pts[c]);
            const int n = matcher.SearchByProjection(sp[c].K, sp[c].S, pts[c], matched, (int)sp[c].th);
            write_ids(o, n, matched);
        }
        {
            std::vector<std::shared_ptr<KeyFrame>> kfs;
            std::vector<Iso> S;
            std::vector<std::unique_ptr<rsc_orb::LoopMapPoints<MPPtr>>> views;
            std::vector<const rsc_orb::LoopMapPoints<MPPtr>*> pv;
            std::vector<std::vector<MPPtr>> matched((size_t)n_search);
            std::vector<std::vector<MPPtr>*> pm;
            for (int c = 0; c < n_search; ++c) {
                kfs.push_back(sp[c].K);
                S.push_back(sp[c].S);
                views.emplace_back(new rsc_orb::LoopMapPoints<MPPtr>(pts[c]));
                pv.push_back(views.back().get());
                matched[c] = slots_from(sp[c].slots, pts[c]);
                pm.push_back(&matched[c]);
            }
            const std::vector<int> n = matcher.SearchByProjectionMany(kfs, S, pv, pm, n_search ? (int)sp[0].th : 10);
            for (int c = 0; c < n_search; ++c) write_ids(o, n[c], matched[c]);
        }
        // ---- Fuse: one point list, several KeyFrames; slots = the KeyFrame's own MapPoints ----
        const int n_fuse = r.get<int32_t>();
        std::vector<MPPtr> fpts = read_points(r);
        std::vector<Problem> fp;
        for (int c = 0; c < n_fuse; ++c) fp.push_back(read_problem(r, fpts));
        for (int c = 0; c < n_fuse; ++c) {
            fp[c].K->mps = slots_from(fp[c].slots, fpts);
            std::vector<MPPtr> rep(fpts.size(), nullptr);
            const int n = matcher.Fuse(fp[c].K, fp[c].S, fpts, fp[c].th, rep);
            write_ids(o, n, rep);
            write_ids(o, n, fp[c].K->mps);
        }
        {
            for (auto& m : fpts) m->obs.clear();
            std::vector<std::shared_ptr<KeyFrame>> kfs;
            std::vector<Iso> S;
            std::vector<std::vector<MPPtr>> rep((size_t)n_fuse, std::vector<MPPtr>(fpts.size(), nullptr));
            std::vector<std::vector<MPPtr>*> pr;
            for (int c = 0; c < n_fuse; ++c) {
                fp[c].K->mps = slots_from(fp[c].slots, fpts);
                kfs.push_back(fp[c].K);
                S.push_back(fp[c].S);
                pr.push_back(&rep[c]);
            }
            rsc_orb::LoopMapPoints<MPPtr> view(fpts);
            const std::vector<int> n = matcher.FuseMany(kfs, S, view, n_fuse ? fp[0].th : 4.f, pr);
            int nobs = 0;
            for (auto& m : fpts) nobs += (int)m->obs.size();
            for (int c = 0; c < n_fuse; ++c) {
                write_ids(o, n[c], rep[c]);
                write_ids(o, nobs, fp[c].K->mps);
            }
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "facade_loopproj_test: %s\n", e.what());
        return 1;
    }
    std::fclose(o);
    return 0;
}
