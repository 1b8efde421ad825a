// Drives rsc_orb::ORBmatcher::Fuse(pKF, vpMapPoints, th) and FuseMany(vpTargetKFs, vpMapPoints, th) with mock
// KeyFrame / MapPoint types built from a binary file written by tests/test_gpu_facade_fusekf.py, and writes the
// return values and the final map (slots, bad flags, observations, descriptors) back.  The mocks implement
// Replace, IsInKeyFrame, Observations, AddObservation and ComputeDistinctiveDescriptors as the map model of
// tests/fusekf_ref.py does (MapPoint.cpp:76-87, :158-197, :224-290; observations in KeyFrame-id order).
// Needs a GPU.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
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
struct Iso {
    Mat3 R; Vec3 t;
    Mat3 rotation() const { return R; }
    Vec3 translation() const { return t; }
};
struct KeyFrame;
struct MapPoint;
using KFPtr = std::shared_ptr<KeyFrame>;
using MPPtr = std::shared_ptr<MapPoint>;

struct KeyFrame {
    int id = 0, N = 0;
    std::vector<KeyPoint> mvKeysUn, mvKeys;
    DescMat mDescriptors;
    int mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;
    float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0, fx = 0, fy = 0, cx = 0, cy = 0;
    float mb = 0, mbf = 0, invfx = 0, invfy = 0, mfScaleFactor = 1.2f;
    std::vector<float> mvScaleFactors, mvInvLevelSigma2, mvuRight, mvDepth;
    int mnScaleLevels = 0;
    float mfLogScaleFactor = 0;
    Mat3 R{}, mKinv{};
    Vec3 t{};
    Iso Twc{};
    std::vector<std::vector<std::vector<std::size_t>>> grid;
    std::vector<MPPtr> mps;
    std::vector<MPPtr> GetMapPointMatches() const { return mps; }
    MPPtr GetMapPoint(int idx) const { return mps[idx]; }
    void AddMapPoint(const MPPtr& m, int idx) { mps[idx] = m; }
    const std::vector<std::vector<std::vector<std::size_t>>>& GetGrid() const { return grid; }
    Mat3 GetRotation() const { return R; }
    Vec3 GetTranslation() const { return t; }
    Iso GetPoseInverse() const { return Twc; }
};

static int desc_dist(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int k = 0; k < 32; ++k) d += __builtin_popcount((unsigned)(a[k] ^ b[k]));
    return d;
}

struct MapPoint {
    int id = -1, nObs = 0;
    bool bad = false;
    Vec3 X{}, Nrm{};
    DescMat d;
    float dmax = 0, dmin = 0;
    std::map<int, std::pair<KeyFrame*, int>> obs;  // by KeyFrame id
    bool isBad() const { return bad; }
    Vec3 GetWorldPos() const { return X; }
    Vec3 GetNormal() const { return Nrm; }
    DescMat GetDescriptor() const { return d; }
    float GetMaxDistance() const { return dmax; }
    float GetMinDistance() const { return dmin; }
    int Observations() const { return nObs; }
    bool IsInKeyFrame(const KFPtr& k) const { return obs.count(k->id) != 0; }
    void add(KeyFrame* k, int idx) {  // MapPoint.cpp:76-87
        if (obs.count(k->id)) return;
        obs[k->id] = std::make_pair(k, idx);
        nObs += k->mvuRight[idx] >= 0 ? 2 : 1;
    }
    void AddObservation(const KFPtr& k, int idx) { add(k.get(), idx); }
    void ComputeDistinctiveDescriptors() {  // MapPoint.cpp:224-290
        if (bad || obs.empty()) return;
        std::vector<const uint8_t*> ds;
        for (const auto& o : obs) ds.push_back(o.second.first->mDescriptors.ptr<uint8_t>(o.second.second));
        const size_t n = ds.size();
        int best_median = INT_MAX, best = 0;
        for (size_t i = 0; i < n; ++i) {
            std::vector<int> v(n);
            for (size_t j = 0; j < n; ++j) v[j] = desc_dist(ds[i], ds[j]);
            std::sort(v.begin(), v.end());
            const int median = v[(size_t)(0.5 * (n - 1))];
            if (median < best_median) {
                best_median = median;
                best = (int)i;
            }
        }
        d.d.assign(ds[best], ds[best] + 32);
    }
    void Replace(const MPPtr& pMP) {  // MapPoint.cpp:158-197
        if (pMP->id == id) return;
        auto old = obs;
        obs.clear();
        bad = true;
        for (const auto& o : old) {
            KeyFrame* k = o.second.first;
            const int idx = o.second.second;
            if (!pMP->obs.count(k->id)) {
                k->mps[idx] = pMP;
                pMP->add(k, idx);
            } else {
                k->mps[idx] = nullptr;
            }
        }
        pMP->ComputeDistinctiveDescriptors();
    }
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

static KFPtr read_kf(Reader& r, const std::vector<float>& scale, float log_sf) {
    auto K = std::make_shared<KeyFrame>();
    K->id = r.get<int32_t>();
    const int n = K->N = r.get<int32_t>();
    K->fx = r.get<float>(); K->fy = r.get<float>(); K->cx = r.get<float>(); K->cy = r.get<float>();
    K->mnMinX = r.get<int32_t>(); K->mnMaxX = r.get<int32_t>(); K->mnMinY = r.get<int32_t>(); K->mnMaxY = r.get<int32_t>();
    K->mfGridElementWidthInv = r.get<float>(); K->mfGridElementHeightInv = r.get<float>();
    K->mbf = r.get<float>();
    K->mb = K->mbf / K->fx;
    K->invfx = 1.0f / K->fx; K->invfy = 1.0f / K->fy;
    K->mvScaleFactors = scale;
    K->mnScaleLevels = (int)scale.size();
    K->mfLogScaleFactor = log_sf;
    for (float s : scale) K->mvInvLevelSigma2.push_back(1.0f / (s * s));
    const auto R = r.arr<float>(9), t = r.arr<float>(3), Rwc = r.arr<float>(9), Ow = r.arr<float>(3);
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) {
            K->R.m[a][b] = R[3 * a + b];
            K->Twc.R.m[a][b] = Rwc[3 * a + b];
        }
        K->t.v[a] = t[a];
        K->Twc.t.v[a] = Ow[a];
        K->mKinv.m[a][a] = 1.f;
    }
    const auto kp = r.arr<float>(2 * (size_t)n);
    const auto oct = r.arr<int32_t>((size_t)n);
    K->mDescriptors.d = r.arr<uint8_t>(32 * (size_t)n);
    K->mvuRight = r.arr<float>((size_t)n);
    K->mvDepth.assign((size_t)n, 1.f);
    K->mvKeysUn.resize((size_t)n);
    for (int i = 0; i < n; ++i) K->mvKeysUn[i] = KeyPoint{{kp[2 * i], kp[2 * i + 1]}, oct[i], 0.f};
    K->mvKeys = K->mvKeysUn;
    const auto cb = r.arr<int32_t>(64 * 48 + 1);
    const auto cf = r.arr<int32_t>((size_t)cb[64 * 48]);
    K->grid.assign(64, std::vector<std::vector<std::size_t>>(48));
    for (int ix = 0; ix < 64; ++ix)
        for (int iy = 0; iy < 48; ++iy)
            for (int e = cb[ix * 48 + iy]; e < cb[ix * 48 + iy + 1]; ++e) K->grid[ix][iy].push_back((std::size_t)cf[e]);
    K->mps.assign((size_t)n, nullptr);
    return K;
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
        const int n_levels = r.get<int32_t>();
        const auto scale = r.arr<float>((size_t)n_levels);
        const float log_sf = r.get<float>();
        const int nkf = r.get<int32_t>();
        std::vector<KFPtr> kfs;
        for (int k = 0; k < nkf; ++k) kfs.push_back(read_kf(r, scale, log_sf));
        const int np = r.get<int32_t>();
        const auto bad = r.arr<uint8_t>((size_t)np);
        const auto pos = r.arr<float>(3 * (size_t)np), nrm = r.arr<float>(3 * (size_t)np);
        const auto dmax = r.arr<float>((size_t)np), dmin = r.arr<float>((size_t)np);
        const auto desc = r.arr<uint8_t>(32 * (size_t)np);
        std::vector<MPPtr> pts;
        for (int i = 0; i < np; ++i) {
            auto m = std::make_shared<MapPoint>();
            m->id = i;
            m->bad = bad[i] != 0;
            m->X = Vec3{{pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]}};
            m->Nrm = Vec3{{nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]}};
            m->dmax = dmax[i];
            m->dmin = dmin[i];
            m->d.d.assign(desc.begin() + 32 * (size_t)i, desc.begin() + 32 * (size_t)(i + 1));
            pts.push_back(m);
        }
        const int nobs = r.get<int32_t>();  // (point, KeyFrame index, slot): a bad point sits in the slot unobserved
        for (int k = 0; k < nobs; ++k) {
            const int p = r.get<int32_t>(), kf = r.get<int32_t>(), idx = r.get<int32_t>();
            kfs[kf]->mps[idx] = pts[p];
            if (!pts[p]->bad) pts[p]->add(kfs[kf].get(), idx);
        }
        const int mode = r.get<int32_t>();  // 0 FuseMany, 1 one Fuse per KeyFrame, 2 LocalMapping.cpp:458-490
        const float th = r.get<float>();
        const int cur = r.get<int32_t>();
        const int nt = r.get<int32_t>();
        std::vector<KFPtr> targets;
        for (int k = 0; k < nt; ++k) targets.push_back(kfs[r.get<int32_t>()]);
        const int nl = r.get<int32_t>();
        std::vector<MPPtr> list;
        for (int k = 0; k < nl; ++k) {
            const int p = r.get<int32_t>();
            list.push_back(p < 0 ? nullptr : pts[p]);
        }
        rsc_orb::ORBmatcher matcher;
        std::vector<int32_t> ret;
        if (mode == 2) list = kfs[cur]->GetMapPointMatches();  // :460
        if (mode == 1) {
            for (const auto& k : targets) ret.push_back(matcher.Fuse(k, list, th));
        } else {
            for (int v : matcher.FuseMany(targets, list, th)) ret.push_back(v);
        }
        if (mode == 2) {  // :469-490
            std::vector<MPPtr> cand;
            std::set<int> seen;
            for (const auto& k : targets)
                for (const auto& m : k->GetMapPointMatches()) {
                    if (!m || m->isBad() || seen.count(m->id)) continue;
                    seen.insert(m->id);
                    cand.push_back(m);
                }
            ret.push_back((int32_t)cand.size());
            ret.push_back(matcher.Fuse(kfs[cur], cand, th));
        }
        std::vector<int32_t> out;
        out.push_back((int32_t)ret.size());
        out.insert(out.end(), ret.begin(), ret.end());
        for (const auto& k : kfs)
            for (const auto& m : k->mps) out.push_back(m ? m->id : -1);
        for (const auto& m : pts) {
            out.push_back(m->bad ? 1 : 0);
            out.push_back(m->nObs);
            out.push_back((int32_t)m->obs.size());
            for (const auto& ob : m->obs) {
                out.push_back(ob.first);
                out.push_back(ob.second.second);
            }
            for (int b = 0; b < 32; ++b) out.push_back(m->d.d[b]);
        }
        std::fwrite(out.data(), 4, out.size(), o);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "facade_fusekf_test: %s\n", e.what());
        return 1;
    }
    std::fclose(o);
    return 0;
}
