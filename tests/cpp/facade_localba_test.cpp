// Drives rsc_orb::LocalBundleAdjustment(pKF, pbStopFlag, pMap) (facade/Optimizer.hpp) with mock KeyFrame / MapPoint /
// Map types on maps drawn here.  Every scenario is built twice from the same seed.  On one copy the facade runs.  On
// the other this file follows Optimizer.cpp:426-787 itself — the three lists with their mnBALocalForKF /
// mnBAFixedForKF marks, the vertices and edges in the reference's order with the bad KeyFrames left out (:574), the
// sequential host restatement of the optimisation (tests/localba_emu, mode 0) in place of g2o, vToErase replayed
// through EraseMapPointMatch / EraseObservation, SetPose, SetWorldPos and the per-point UpdateNormalAndDepth() —
// and the two maps are compared field by field: poses, positions, normals, distances, bad flags, every
// observation map and every KeyFrame slot.  The KeyFrames of a map live in one array, so that the pointer order of
// std::map<KeyFrame*, size_t>, which is the edge order, is the same in both copies.  Needs a GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>
#include "Optimizer.hpp"
#include "../localba_emu/localba_emu.cpp"

struct Vec3 {
    float v[3];
    float operator()(int i) const { return v[i]; }
    float& operator()(int i) { return v[i]; }
};
struct Mat3 { float m[3][3]; float operator()(int r, int c) const { return m[r][c]; } };
struct Pose44 {
    float m[4][4];
    float operator()(int r, int c) const { return m[r][c]; }
    float& operator()(int r, int c) { return m[r][c]; }
};
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
    unsigned long mnId = 0, mnBALocalForKF = ~0ul, mnBAFixedForKF = ~0ul;
    int N = 0;
    bool bad = false;
    std::vector<KeyPoint> mvKeysUn, mvKeys;
    DescMat mDescriptors;
    int mnMinX = 0, mnMinY = 0, mnMaxX = 640, mnMaxY = 480;
    float mfGridElementWidthInv = 0.1f, mfGridElementHeightInv = 0.1f, fx = 500, fy = 500, cx = 320, cy = 240;
    float mb = 0.08f, mbf = 40.0f, invfx = 1 / 500.f, invfy = 1 / 500.f, mfScaleFactor = 1.2f;
    std::vector<float> mvScaleFactors, mvInvLevelSigma2, mvuRight, mvDepth;
    int mnScaleLevels = 8;
    float mfLogScaleFactor = std::log(1.2f);
    Mat3 R{}, mKinv{};
    Vec3 t{};
    Iso Twc{};
    Pose44 Tcw{};
    std::vector<std::vector<std::vector<std::size_t>>> grid;
    std::vector<MPPtr> mps;
    std::vector<KFPtr> covisible;
    bool isBad() const { return bad; }
    std::vector<MPPtr> GetMapPointMatches() const { return mps; }
    std::vector<KFPtr> GetVectorCovisibleKeyFrames() const { return covisible; }
    const std::vector<std::vector<std::vector<std::size_t>>>& GetGrid() const { return grid; }
    Mat3 GetRotation() const { return R; }
    Vec3 GetTranslation() const { return t; }
    Iso GetPoseInverse() const { return Twc; }
    Vec3 GetCameraCenter() const { return Twc.t; }
    Pose44 GetPose() const { return Tcw; }
    void SetPose(const Pose44& T) {  // KeyFrame.cpp: Tcw, then Twc and Ow from it
        Tcw = T;
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) {
                R.m[a][b] = T.m[a][b];
                Twc.R.m[b][a] = T.m[a][b];
            }
            t.v[a] = T.m[a][3];
        }
        for (int a = 0; a < 3; ++a)
            Twc.t.v[a] = -((Twc.R.m[a][0] * t.v[0] + Twc.R.m[a][1] * t.v[1]) + Twc.R.m[a][2] * t.v[2]);
    }
    void EraseMapPointMatch(const MPPtr& pMP);
    void EraseMapPointMatch(size_t idx) { mps[idx] = nullptr; }
};

static float norm3(const float* x) { return sqrtf((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]); }

struct MapPoint {
    unsigned long mnId = 0, mnBALocalForKF = ~0ul;
    int nObs = 0;
    bool bad = false;
    Vec3 X{}, Nrm{};
    DescMat d;
    float dmax = 0, dmin = 0;
    std::map<KFPtr, size_t> mObservations;
    KFPtr mpRefKF;
    bool isBad() const { return bad; }
    Vec3 GetWorldPos() const { return X; }
    void SetWorldPos(const Vec3& p) { X = p; }
    std::map<KFPtr, size_t> GetObservations() const { return mObservations; }
    KFPtr GetReferenceKeyFrame() const { return mpRefKF; }
    Vec3 GetNormal() const { return Nrm; }
    DescMat GetDescriptor() const { return d; }
    float GetMaxDistance() const { return dmax; }
    float GetMinDistance() const { return dmin; }
    int Observations() const { return nObs; }
    bool IsInKeyFrame(const KFPtr& k) const { return mObservations.count(k) != 0; }
    void AddObservation(const KFPtr& k, size_t idx) {
        mObservations[k] = idx;
        nObs += k->mvuRight[idx] >= 0 ? 2 : 1;
    }
    void SetDistinctiveDescriptor(const uint8_t* p) { d.d.assign(p, p + 32); }
    void SetNormalAndDepth(const float n[3], float minDist, float maxDist) {
        Nrm = Vec3{{n[0], n[1], n[2]}};
        dmin = minDist;
        dmax = maxDist;
    }
    void SetBadFlag() {  // MapPoint.cpp:134-150
        const auto obs = mObservations;
        mObservations.clear();
        bad = true;
        for (const auto& o : obs) o.first->EraseMapPointMatch(o.second);
    }
    void EraseObservation(const KFPtr& pKF) {  // MapPoint.cpp:89-118
        bool bBad = false;
        if (mObservations.count(pKF)) {
            const size_t idx = mObservations[pKF];
            nObs -= pKF->mvuRight[idx] >= 0 ? 2 : 1;
            mObservations.erase(pKF);
            if (mpRefKF == pKF && !mObservations.empty()) mpRefKF = mObservations.begin()->first;
            if (nObs <= 2) bBad = true;
        }
        if (bBad) SetBadFlag();
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
        const int level = pRefKF->mvKeysUn[observations[pRefKF]].octave;
        const float levelScaleFactor = pRefKF->mvScaleFactors[level];
        const int nLevels = pRefKF->mnScaleLevels;
        dmax = dist * levelScaleFactor;
        dmin = dmax / pRefKF->mvScaleFactors[nLevels - 1];
        for (int k = 0; k < 3; ++k) Nrm.v[k] = normal[k] / (float)n;
    }
};

void KeyFrame::EraseMapPointMatch(const MPPtr& pMP) {  // KeyFrame.cpp: GetIndexInKeyFrame, then the slot
    for (const auto& o : pMP->mObservations)
        if (o.first.get() == this) mps[o.second] = nullptr;
}

struct Map { std::mutex mMutexMapUpdate; };

struct Rng {
    uint64_t s;
    double next() {
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        return (double)(s >> 11) / 9007199254740992.0;
    }
    double sym(double a) { return (2.0 * next() - 1.0) * a; }
};

struct World {
    std::vector<KeyFrame> store;  // one array: pointer order is index order
    std::vector<KFPtr> kfs;
    std::vector<MPPtr> pts;
    Map map;
    KFPtr cur;
};

struct Scenario {
    uint64_t seed;
    int n_kfs, n_neigh, n_points;
    double outlier_frac;
    bool with_kf0, bad_neighbour, bad_observer;
};

// KeyFrames along x looking down +z; the current one is the last, its covisible ones the n_neigh before it (the
// highest ids first, as a covisibility order would be: list order is not id order); the others see the points too
// and end up as fixed cameras.  with_kf0: KeyFrame id 0 is covisible.  One MapPoint is bad and one slot is empty.
static void build(World& W, const Scenario& S) {
    Rng g{S.seed};
    const int K = S.n_kfs;
    W.store.resize((size_t)K);
    for (int k = 0; k < K; ++k) {
        KeyFrame& F = W.store[k];
        F.mnId = S.with_kf0 ? (unsigned long)k : (unsigned long)(k + 3);
        for (int l = 0; l < 8; ++l) {
            F.mvScaleFactors.push_back(std::pow(1.2f, (float)l));
            F.mvInvLevelSigma2.push_back(1.0f / (F.mvScaleFactors[l] * F.mvScaleFactors[l]));
        }
        for (int a = 0; a < 3; ++a) F.mKinv.m[a][a] = 1.f;
        F.grid.assign(64, std::vector<std::vector<std::size_t>>(48));
        Pose44 T{};
        for (int a = 0; a < 4; ++a) T.m[a][a] = 1.f;
        const bool moves = k >= K - 1 - S.n_neigh && F.mnId != 0;
        T.m[0][3] = (float)(-0.3 * k + (moves ? g.sym(0.01) : 0.0));
        T.m[1][3] = (float)(moves ? g.sym(0.01) : 0.0);
        F.SetPose(T);
        W.kfs.push_back(KFPtr(&F, [](KeyFrame*) {}));
    }
    W.cur = W.kfs[K - 1];
    for (int k = K - 2; k >= K - 1 - S.n_neigh; --k) W.cur->covisible.push_back(W.kfs[k]);
    if (S.with_kf0) W.cur->covisible.push_back(W.kfs[0]);
    for (int i = 0; i < S.n_points; ++i) {
        auto m = std::make_shared<MapPoint>();
        m->mnId = (unsigned long)(100 + 2 * ((i * 7) % S.n_points));
        const double X[3] = {g.sym(1.0) + 0.15 * K, g.sym(1.0), 4.0 + 5.0 * g.next()};
        for (int j = 0; j < 3; ++j) m->X.v[j] = (float)(X[j] + g.sym(0.03));
        m->d.d.assign(32, (uint8_t)i);
        const int nobs = std::min(K, 3 + (int)(3 * g.next()));
        const int first = (int)(g.next() * K);
        for (int o = 0; o < nobs; ++o) {
            const int k = (first + o) % K;
            KeyFrame& F = W.store[k];
            const double x = X[0] - 0.3 * k, z = X[2];
            double u = 500 * x / z + 320 + g.sym(0.5), v = 500 * X[1] / z + 240 + g.sym(0.5);
            if (g.next() < S.outlier_frac) {
                u += 70.0;
                v -= 50.0;
            }
            F.mvKeysUn.push_back(KeyPoint{{(float)u, (float)v}, (int)(4 * g.next()), 0.f});
            F.mvuRight.push_back(g.next() < 0.6 ? (float)(u - 40.0 / z) : -1.0f);
            F.mvDepth.push_back((float)z);
            F.mDescriptors.d.insert(F.mDescriptors.d.end(), 32, (uint8_t)i);
            F.mps.push_back(m);
            m->AddObservation(W.kfs[k], F.mps.size() - 1);
            if (!m->mpRefKF) m->mpRefKF = W.kfs[k];
        }
        W.pts.push_back(m);
    }
    for (auto& F : W.store) {
        // an empty slot and a slot with a bad MapPoint in every KeyFrame
        for (int extra = 0; extra < 2; ++extra) {
            F.mvKeysUn.push_back(KeyPoint{{10.f, 10.f}, 0, 0.f});
            F.mvuRight.push_back(-1.f);
            F.mvDepth.push_back(-1.f);
            F.mDescriptors.d.insert(F.mDescriptors.d.end(), 32, 0);
        }
        F.mps.push_back(nullptr);
        auto dead = std::make_shared<MapPoint>();
        dead->mnId = 9000 + F.mnId;
        dead->bad = true;
        F.mps.push_back(dead);
        F.N = (int)F.mps.size();
        F.mvKeys = F.mvKeysUn;
    }
    if (S.bad_neighbour) W.kfs[K - 2]->bad = true;  // covisible, marked local, not optimised, its edges left out
    if (S.bad_observer) W.kfs[0]->bad = true;       // would be a fixed camera
}

// Optimizer.cpp:426-787 on the mock map, the optimisation itself by the sequential host restatement
static bool reference_flow(World& W, bool* pbStopFlag) {
    const KFPtr pKF = W.cur;
    std::vector<KFPtr> lLocalKeyFrames, lFixedCameras;
    std::vector<MPPtr> lLocalMapPoints;
    lLocalKeyFrames.push_back(pKF);
    pKF->mnBALocalForKF = pKF->mnId;
    for (const KFPtr& pKFi : pKF->GetVectorCovisibleKeyFrames()) {
        pKFi->mnBALocalForKF = pKF->mnId;
        if (!pKFi->isBad()) lLocalKeyFrames.push_back(pKFi);
    }
    for (const KFPtr& k : lLocalKeyFrames)
        for (const MPPtr& pMP : k->GetMapPointMatches())
            if (pMP)
                if (!pMP->isBad())
                    if (pMP->mnBALocalForKF != pKF->mnId) {
                        lLocalMapPoints.push_back(pMP);
                        pMP->mnBALocalForKF = pKF->mnId;
                    }
    for (const MPPtr& pMP : lLocalMapPoints)
        for (const auto& o : pMP->GetObservations()) {
            const KFPtr pKFi = o.first;
            if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
                pKFi->mnBAFixedForKF = pKF->mnId;
                if (!pKFi->isBad()) lFixedCameras.push_back(pKFi);
            }
        }
    std::vector<KFPtr> vertices;
    std::vector<int64_t> kf_id, mp_id;
    std::vector<uint8_t> fixed, bad;
    std::vector<float> Tcw, cam, pos, uv, ur, inv;
    std::vector<int32_t> begin(1, 0), obs_kf;
    std::vector<std::pair<KFPtr, MPPtr>> edge;
    auto add_vertex = [&](const KFPtr& k, bool fix) {
        vertices.push_back(k);
        kf_id.push_back((int64_t)k->mnId);
        fixed.push_back(fix ? 1 : 0);
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) Tcw.push_back(k->Tcw.m[r][c]);
        for (float v : {k->fx, k->fy, k->cx, k->cy, k->mbf}) cam.push_back(v);
    };
    for (const KFPtr& k : lLocalKeyFrames) add_vertex(k, k->mnId == 0);  // :505-515
    for (const KFPtr& k : lFixedCameras) add_vertex(k, true);            // :519-529
    for (const MPPtr& pMP : lLocalMapPoints) {                            // :557-638
        mp_id.push_back((int64_t)pMP->mnId);
        bad.push_back(pMP->isBad() ? 1 : 0);
        for (int j = 0; j < 3; ++j) pos.push_back(pMP->X.v[j]);
        for (const auto& o : pMP->GetObservations()) {
            if (o.first->isBad()) continue;
            int at = -1;
            for (size_t v = 0; v < vertices.size(); ++v)
                if (vertices[v] == o.first) at = (int)v;
            if (at < 0) return false;
            obs_kf.push_back(at);
            uv.push_back(o.first->mvKeysUn[o.second].pt.x);
            uv.push_back(o.first->mvKeysUn[o.second].pt.y);
            ur.push_back(o.first->mvuRight[o.second]);
            inv.push_back(o.first->mvInvLevelSigma2[o.first->mvKeysUn[o.second].octave]);
            edge.push_back({o.first, pMP});
        }
        begin.push_back((int32_t)obs_kf.size());
    }
    if (pbStopFlag && *pbStopFlag) return true;
    const size_t E = obs_kf.size(), K = vertices.size(), N = lLocalMapPoints.size();
    bad.push_back(0); pos.push_back(0); obs_kf.push_back(0); uv.push_back(0); ur.push_back(0); inv.push_back(0);
    rsc_localba_problem q;
    q.n_kfs = (int32_t)K; q.kf_id = kf_id.data(); q.fixed = fixed.data(); q.Tcw = Tcw.data(); q.cam = cam.data();
    q.n_points = (int32_t)N; q.mp_id = mp_id.data(); q.pos = pos.data(); q.bad = bad.data(); q.obs_begin = begin.data();
    q.obs_kf = obs_kf.data(); q.uv = uv.data(); q.u_right = ur.data(); q.inv_sigma2 = inv.data();
    std::vector<float> To(16 * K + 1), Xo(3 * N + 1);
    std::vector<int32_t> er(E + 1);
    const rsc_localba_out o{To.data(), Xo.data(), nullptr, er.data()};
    rsc_localba_result res;
    if (lbae_run(&q, 0, &o, &res) != 0) return false;
    std::unique_lock<std::mutex> lock(W.map.mMutexMapUpdate);
    for (int i = 0; i < res.n_erase; ++i) {
        const KFPtr pKFi = edge[er[i]].first;
        const MPPtr pMPi = edge[er[i]].second;
        pKFi->EraseMapPointMatch(pMPi);
        pMPi->EraseObservation(pKFi);
    }
    for (size_t k = 0; k < lLocalKeyFrames.size(); ++k) {
        Pose44 T;
        std::memcpy(T.m, To.data() + 16 * k, 64);
        lLocalKeyFrames[k]->SetPose(T);
    }
    for (size_t p = 0; p < N; ++p) {
        lLocalMapPoints[p]->SetWorldPos(Vec3{{Xo[3 * p], Xo[3 * p + 1], Xo[3 * p + 2]}});
        lLocalMapPoints[p]->UpdateNormalAndDepth();
    }
    std::printf("   model: %zu KeyFrames (%zu local), %zu points, %zu edges, %d erased\n", K, lLocalKeyFrames.size(), N, E,
                res.n_erase);
    return true;
}

static bool same_float(float a, float b) {
    if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
    return std::memcmp(&a, &b, 4) == 0;
}

// the number of fields that differ between the two maps
static int compare(const World& A, const World& B) {
    int diff = 0;
    for (size_t k = 0; k < A.store.size(); ++k) {
        const KeyFrame &a = A.store[k], &b = B.store[k];
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) diff += !same_float(a.Tcw.m[r][c], b.Tcw.m[r][c]);
        for (int j = 0; j < 3; ++j) diff += !same_float(a.Twc.t.v[j], b.Twc.t.v[j]);
        diff += a.mnBALocalForKF != b.mnBALocalForKF || a.mnBAFixedForKF != b.mnBAFixedForKF;
        for (size_t s = 0; s < a.mps.size(); ++s) {
            diff += (a.mps[s] == nullptr) != (b.mps[s] == nullptr);
            if (a.mps[s] && b.mps[s]) diff += a.mps[s]->mnId != b.mps[s]->mnId;
        }
    }
    for (size_t p = 0; p < A.pts.size(); ++p) {
        const MapPoint &a = *A.pts[p], &b = *B.pts[p];
        for (int j = 0; j < 3; ++j) diff += !same_float(a.X.v[j], b.X.v[j]) + !same_float(a.Nrm.v[j], b.Nrm.v[j]);
        diff += !same_float(a.dmax, b.dmax) + !same_float(a.dmin, b.dmin);
        diff += a.bad != b.bad || a.nObs != b.nObs || a.mnBALocalForKF != b.mnBALocalForKF;
        diff += a.mObservations.size() != b.mObservations.size();
        auto ia = a.mObservations.begin();
        auto ib = b.mObservations.begin();
        for (; ia != a.mObservations.end() && ib != b.mObservations.end(); ++ia, ++ib)
            diff += ia->first->mnId != ib->first->mnId || ia->second != ib->second;
        diff += (a.mpRefKF ? a.mpRefKF->mnId : ~0ul) != (b.mpRefKF ? b.mpRefKF->mnId : ~0ul);
    }
    return diff;
}

static int run(const char* name, const Scenario& S, bool stop) {
    World A, B, C;
    build(A, S);
    build(B, S);
    build(C, S);  // untouched: what the call changed
    bool flagA = stop, flagB = stop;
    rsc_orb::LocalBundleAdjustment(A.cur, &flagA, &A.map);
    if (!reference_flow(B, &flagB)) {
        std::printf("%s: the model could not run\n", name);
        return 1;
    }
    const int diff = compare(A, B);
    const int changed = compare(A, C);
    int erased = 0;
    for (size_t p = 0; p < A.pts.size(); ++p) erased += (int)(C.pts[p]->mObservations.size() - A.pts[p]->mObservations.size());
    // a stopped call leaves only the marks behind; a run one moves the map
    const bool ok = diff == 0 && (stop ? erased == 0 : changed > 0) && (S.outlier_frac > 0 && !stop ? erased > 0 : true);
    std::printf("%s: differing fields %d, changed by the call %d, observations erased %d %s\n", name, diff, changed, erased,
                ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
}

int main() {
    int bad = 0;
    try {
        bad += run("window", Scenario{1, 8, 3, 60, 0.0, false, false, false}, false);
        bad += run("outliers", Scenario{2, 8, 3, 60, 0.10, false, false, false}, false);
        bad += run("kf0_covisible", Scenario{3, 7, 3, 50, 0.05, true, false, false}, false);
        bad += run("bad_keyframes", Scenario{4, 8, 4, 60, 0.05, false, true, true}, false);
        bad += run("all_local", Scenario{5, 4, 3, 30, 0.0, false, false, false}, false);
        bad += run("stop_flag", Scenario{6, 8, 3, 40, 0.10, false, false, false}, true);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "facade_localba_test: %s\n", e.what());
        return 1;
    }
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
