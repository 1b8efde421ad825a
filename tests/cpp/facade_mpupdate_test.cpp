// Drives rsc_orb::UpdateMapPoints(vpMapPoints, what) and UpdateMapPointsOf(pKF) (facade/MapPoint.hpp) with mock
// KeyFrame / MapPoint types built from a binary file written by tests/test_gpu_facade_mpupdate.py.  The mock
// MapPoint keeps its observations in a std::map<std::shared_ptr<KeyFrame>, size_t> as the reference does, and has
// the reference's ComputeDistinctiveDescriptors() and UpdateNormalAndDepth() restated sequentially
// (MapPoint.cpp:224-289, :312-353).  The program copies the MapPoints (the copies share the KeyFrames, so both maps
// iterate in the same pointer order), runs the restated functions on the copies and the facade on the originals,
// and writes the number of differing points and the facade's results back.  Mode 2 first runs
// LocalMapping.cpp:458-490 through ORBmatcher::FuseMany / Fuse, then compares the update loop of :493-506.
// Needs a GPU.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <vector>
#include "MapPoint.hpp"

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
    bool bad = false;
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
    bool isBad() const { return bad; }
    std::vector<MPPtr> GetMapPointMatches() const { return mps; }
    MPPtr GetMapPoint(int idx) const { return mps[idx]; }
    void AddMapPoint(const MPPtr& m, int idx) { mps[idx] = m; }
    const std::vector<std::vector<std::vector<std::size_t>>>& GetGrid() const { return grid; }
    Mat3 GetRotation() const { return R; }
    Vec3 GetTranslation() const { return t; }
    Iso GetPoseInverse() const { return Twc; }
    Vec3 GetCameraCenter() const { return Twc.t; }
};

static int desc_dist(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int k = 0; k < 32; ++k) d += __builtin_popcount((unsigned)(a[k] ^ b[k]));
    return d;
}

static float norm3(const float* x) { return sqrtf((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]); }

struct MapPoint {
    int id = -1, nObs = 0;
    bool bad = false;
    Vec3 X{}, Nrm{};
    DescMat d;
    float dmax = 0, dmin = 0;
    std::map<KFPtr, size_t> mObservations;
    KFPtr mpRefKF;
    bool isBad() const { return bad; }
    Vec3 GetWorldPos() const { return X; }
    Vec3 GetNormal() const { return Nrm; }
    DescMat GetDescriptor() const { return d; }
    float GetMaxDistance() const { return dmax; }
    float GetMinDistance() const { return dmin; }
    int Observations() const { return nObs; }
    std::map<KFPtr, size_t> GetObservations() const { return mObservations; }
    KFPtr GetReferenceKeyFrame() const { return mpRefKF; }
    bool IsInKeyFrame(const KFPtr& k) const { return mObservations.count(k) != 0; }
    void AddObservation(const KFPtr& k, size_t idx) {  // MapPoint.cpp:76-87
        if (mObservations.count(k)) return;
        mObservations[k] = idx;
        nObs += k->mvuRight[idx] >= 0 ? 2 : 1;
    }
    // the two members the integrator adds
    void SetDistinctiveDescriptor(const uint8_t* p) { d.d.assign(p, p + 32); }
    void SetNormalAndDepth(const float n[3], float minDist, float maxDist) {
        Nrm = Vec3{{n[0], n[1], n[2]}};
        dmin = minDist;
        dmax = maxDist;
    }
    void ComputeDistinctiveDescriptors() {  // MapPoint.cpp:224-289
        if (bad) return;
        const std::map<KFPtr, size_t> observations = mObservations;
        if (observations.empty()) return;
        std::vector<const uint8_t*> v;
        for (const auto& o : observations)
            if (!o.first->isBad()) v.push_back(o.first->mDescriptors.ptr<uint8_t>((int)o.second));
        if (v.empty()) return;
        const size_t N = v.size();
        std::vector<float> D(N * N);
        for (size_t i = 0; i < N; ++i) {
            D[i * N + i] = 0;
            for (size_t j = i + 1; j < N; ++j) D[i * N + j] = D[j * N + i] = (float)desc_dist(v[i], v[j]);
        }
        int BestMedian = INT_MAX, BestIdx = 0;
        for (size_t i = 0; i < N; ++i) {
            std::vector<int> vDists(D.begin() + i * N, D.begin() + (i + 1) * N);
            std::sort(vDists.begin(), vDists.end());
            const int median = vDists[0.5 * (N - 1)];
            if (median < BestMedian) {
                BestMedian = median;
                BestIdx = (int)i;
            }
        }
        d.d.assign(v[BestIdx], v[BestIdx] + 32);
    }
    void UpdateNormalAndDepth() {  // MapPoint.cpp:312-353
        if (bad) return;
        std::map<KFPtr, size_t> observations = mObservations;
        const KFPtr pRefKF = mpRefKF;
        const Vec3 Pos = X;
        if (observations.empty()) return;
        float normal[3] = {0.0f, 0.0f, 0.0f};
        int n = 0;
        for (const auto& o : observations) {
            const Vec3 Owi = o.first->GetCameraCenter();
            const float ni[3] = {Pos.v[0] - Owi.v[0], Pos.v[1] - Owi.v[1], Pos.v[2] - Owi.v[2]};
            const float nrm = norm3(ni);
            for (int k = 0; k < 3; ++k) normal[k] = normal[k] + ni[k] / nrm;
            n++;
        }
        const Vec3 Owr = pRefKF->GetCameraCenter();
        const float PC[3] = {Pos.v[0] - Owr.v[0], Pos.v[1] - Owr.v[1], Pos.v[2] - Owr.v[2]};
        const float dist = norm3(PC);
        const int level = pRefKF->mvKeysUn[observations[pRefKF]].octave;  // inserts index 0 when it is not there
        const float levelScaleFactor = pRefKF->mvScaleFactors[level];
        const int nLevels = pRefKF->mnScaleLevels;
        dmax = dist * levelScaleFactor;
        dmin = dmax / pRefKF->mvScaleFactors[nLevels - 1];
        for (int k = 0; k < 3; ++k) Nrm.v[k] = normal[k] / (float)n;
    }
    void Replace(const MPPtr& pMP);
};

void MapPoint::Replace(const MPPtr& pMP) {  // MapPoint.cpp:158-197
    if (pMP->id == id) return;
    auto obs = mObservations;
    mObservations.clear();
    bad = true;
    for (const auto& o : obs) {
        const KFPtr& k = o.first;
        if (!pMP->IsInKeyFrame(k)) {
            k->mps[o.second] = pMP;
            pMP->AddObservation(k, o.second);
        } else {
            k->mps[o.second] = nullptr;
        }
    }
    pMP->ComputeDistinctiveDescriptors();
}

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

// bit for bit, but a NaN matches any NaN (the sign and payload of a produced NaN are the hardware's choice)
static bool same_float(float a, float b) {
    if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
    return std::memcmp(&a, &b, 4) == 0;
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
        const auto kf_bad = r.arr<uint8_t>((size_t)nkf);
        for (int k = 0; k < nkf; ++k) kfs[k]->bad = kf_bad[k] != 0;
        const int np = r.get<int32_t>();
        const auto bad = r.arr<uint8_t>((size_t)np);
        const auto pos = r.arr<float>(3 * (size_t)np), nrm = r.arr<float>(3 * (size_t)np);
        const auto dmax = r.arr<float>((size_t)np), dmin = r.arr<float>((size_t)np);
        const auto desc = r.arr<uint8_t>(32 * (size_t)np);
        const auto ref = r.arr<int32_t>((size_t)np);
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
            if (ref[i] >= 0) m->mpRefKF = kfs[ref[i]];
            pts.push_back(m);
        }
        const int nobs = r.get<int32_t>();  // (point, KeyFrame index, slot): a bad point sits in the slot unobserved
        for (int k = 0; k < nobs; ++k) {
            const int p = r.get<int32_t>(), kf = r.get<int32_t>(), idx = r.get<int32_t>();
            kfs[kf]->mps[idx] = pts[p];
            if (!pts[p]->bad) pts[p]->AddObservation(kfs[kf], (size_t)idx);
        }
        const int mode = r.get<int32_t>();  // 0 UpdateMapPoints(list, what), 2 LocalMapping.cpp:458-506
        const int what = r.get<int32_t>();
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
        int fused = 0;
        if (mode == 2) {  // :458-490 through the matcher facade
            rsc_orb::ORBmatcher matcher;
            for (int v : matcher.FuseMany(targets, kfs[cur]->GetMapPointMatches(), th)) fused += v;
            std::vector<MPPtr> cand;
            std::set<int> seen;
            for (const auto& k : targets)
                for (const auto& m : k->GetMapPointMatches()) {
                    if (!m || m->isBad() || seen.count(m->id)) continue;
                    seen.insert(m->id);
                    cand.push_back(m);
                }
            fused += matcher.Fuse(kfs[cur], cand, th);
            list = kfs[cur]->GetMapPointMatches();  // :494
        }
        // the sequential model on copies of the MapPoints as they are now
        std::vector<MPPtr> model;
        for (const auto& m : pts) model.push_back(std::make_shared<MapPoint>(*m));
        for (const auto& m : list) {  // :495-506
            if (!m || m->isBad()) continue;
            if (what & 1) model[m->id]->ComputeDistinctiveDescriptors();
            if (what & 2) model[m->id]->UpdateNormalAndDepth();
        }
        const int n_updated = mode == 2 ? rsc_orb::UpdateMapPointsOf(kfs[cur])
                                        : rsc_orb::UpdateMapPoints(rsc_orb::thread_context(), list, what);
        int mismatches = 0;
        std::vector<int32_t> out;
        for (int i = 0; i < np; ++i) {
            const MapPoint &a = *pts[i], &b = *model[i];
            bool same = a.d.d == b.d.d && same_float(a.dmax, b.dmax) && same_float(a.dmin, b.dmin);
            for (int k = 0; k < 3; ++k) same = same && same_float(a.Nrm.v[k], b.Nrm.v[k]);
            mismatches += !same;
        }
        out.push_back(mismatches);
        out.push_back(n_updated);
        out.push_back(fused);
        for (const auto& m : pts) {
            out.push_back(m->bad ? 1 : 0);
            out.push_back((int32_t)m->mObservations.size());
            for (int b = 0; b < 32; ++b) out.push_back(m->d.d[b]);
            const float fl[5] = {m->Nrm.v[0], m->Nrm.v[1], m->Nrm.v[2], m->dmax, m->dmin};
            for (float x : fl) {
                int32_t w;
                std::memcpy(&w, &x, 4);
                out.push_back(w);
            }
        }
        std::fwrite(out.data(), 4, out.size(), o);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "facade_mpupdate_test: %s\n", e.what());
        return 1;
    }
    std::fclose(o);
    return 0;
}
