// Drives rsc_orb::ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th) and
// rsc_orb::TrackWithMotionModel(CurrentFrame, LastFrame, th, bOnlyTracking) with mock Frame / MapPoint types
// built from a binary file written by tests/test_gpu_facade_lastproj.py, and writes the results back: the
// return values, CurrentFrame.mvpMapPoints as MapPoint ids, mvbOutlier, the pose, and the track members of the
// LastFrame's MapPoints.  Needs a GPU.
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
    int id = -1; Vec3 X{}; DescMat d; int nobs = 0;
    long unsigned int mnLastFrameSeen = 0;
    bool mbTrackInView = true;
    int Observations() const { return nobs; }
    Vec3 GetWorldPos() const { return X; }
    DescMat GetDescriptor() const { return d; }
};
using MPPtr = std::shared_ptr<MapPoint>;
// Eigen::Isometry3f stand-in: rotation() / translation() and operator()(r, c)
struct Iso {
    float a[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    Mat3 rotation() const {
        Mat3 R;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) R.m[r][c] = a[4 * r + c];
        return R;
    }
    Vec3 translation() const { return Vec3{{a[3], a[7], a[11]}}; }
    float& operator()(int r, int c) { return a[4 * r + c]; }
    float operator()(int r, int c) const { return a[4 * r + c]; }
};
struct Frame {
    int N = 0; long unsigned int mnId = 7;
    std::vector<KeyPoint> mvKeys, mvKeysUn; DescMat mDescriptors;
    float mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;
    float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0, fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0, mb = 0;
    std::vector<float> mvScaleFactors, mvuRight; int mnScaleLevels = 0; float mfLogScaleFactor = 0;
    Iso mTcw{};
    std::vector<std::size_t> mGrid[64][48];
    std::vector<MPPtr> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    int set_pose_calls = 0;
    void SetPose(const Iso& T) { mTcw = T; ++set_pose_calls; }
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
    int kind = 0;  // 0 the matcher, 1 the driver
    std::shared_ptr<Frame> cur, last;
    std::vector<uint8_t> occ;
    float th = 0;
    int check_ori = 1, only_tracking = 0;
};

static Problem read_problem(Reader& r) {
    Problem p;
    p.kind = r.get<int32_t>();
    auto F = std::make_shared<Frame>();
    const int nf = F->N = r.get<int32_t>();
    F->fx = r.get<float>(); F->fy = r.get<float>(); F->cx = r.get<float>(); F->cy = r.get<float>();
    F->mnMinX = r.get<float>(); F->mnMaxX = r.get<float>(); F->mnMinY = r.get<float>(); F->mnMaxY = r.get<float>();
    F->mfGridElementWidthInv = r.get<float>(); F->mfGridElementHeightInv = r.get<float>();
    F->mnScaleLevels = r.get<int32_t>();
    F->mvScaleFactors = r.arr<float>((size_t)F->mnScaleLevels);
    F->mfLogScaleFactor = r.get<float>();
    const auto Tc = r.arr<float>(16);
    std::memcpy(F->mTcw.a, Tc.data(), sizeof(F->mTcw.a));
    const auto kp = r.arr<float>(2 * (size_t)nf);
    const auto oct = r.arr<int32_t>((size_t)nf);
    const auto ang = r.arr<float>((size_t)nf);
    F->mDescriptors.d = r.arr<uint8_t>(32 * (size_t)nf);
    F->mvKeysUn.resize((size_t)nf);
    for (int i = 0; i < nf; ++i) F->mvKeysUn[i] = KeyPoint{{kp[2 * i], kp[2 * i + 1]}, oct[i], ang[i]};
    F->mvKeys = F->mvKeysUn;
    const auto cb = r.arr<int32_t>(64 * 48 + 1);
    const auto cf = r.arr<int32_t>((size_t)cb[64 * 48]);
    for (int ix = 0; ix < 64; ++ix)
        for (int iy = 0; iy < 48; ++iy)
            for (int e = cb[ix * 48 + iy]; e < cb[ix * 48 + iy + 1]; ++e) F->mGrid[ix][iy].push_back((std::size_t)cf[e]);
    F->mvuRight = r.arr<float>((size_t)nf);
    F->mbf = r.get<float>();
    F->mb = r.get<float>();
    p.occ = r.arr<uint8_t>((size_t)nf);
    // the last Frame: what the matcher reads of it.  mvKeys carries the octave and a poisoned angle, mvKeysUn the
    // angle and a poisoned octave: the facade must read each from the member the reference reads
    auto L = std::make_shared<Frame>();
    const int nl = L->N = r.get<int32_t>();
    const auto Tl = r.arr<float>(16);
    std::memcpy(L->mTcw.a, Tl.data(), sizeof(L->mTcw.a));
    const auto loct = r.arr<int32_t>((size_t)nl);
    const auto lang = r.arr<float>((size_t)nl);
    const auto state = r.arr<uint8_t>((size_t)nl);
    const auto pos = r.arr<float>(3 * (size_t)nl);
    const auto desc = r.arr<uint8_t>(32 * (size_t)nl);
    const auto has_obs = r.arr<uint8_t>((size_t)nl);
    L->mvKeys.resize((size_t)nl);
    L->mvKeysUn.resize((size_t)nl);
    L->mvpMapPoints.assign((size_t)nl, nullptr);
    L->mvbOutlier.assign((size_t)nl, false);
    for (int i = 0; i < nl; ++i) {
        L->mvKeys[i] = KeyPoint{{0, 0}, loct[i], 123.0f};
        L->mvKeysUn[i] = KeyPoint{{0, 0}, 99, lang[i]};
        if (!state[i]) continue;
        auto m = std::make_shared<MapPoint>();
        m->id = i;
        m->X = Vec3{{pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]}};
        m->d.d.assign(desc.begin() + 32 * (size_t)i, desc.begin() + 32 * (size_t)(i + 1));
        m->nobs = has_obs[i] ? 3 : 0;
        L->mvpMapPoints[i] = m;
        L->mvbOutlier[i] = state[i] == 2;
    }
    p.th = r.get<float>();
    p.check_ori = r.get<int32_t>();
    p.only_tracking = r.get<int32_t>();
    p.cur = F;
    p.last = L;
    return p;
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

static void write_ids(FILE* o, const Frame& F) {
    std::vector<int32_t> ids((size_t)F.N);
    for (int f = 0; f < F.N; ++f) ids[f] = F.mvpMapPoints[f] ? F.mvpMapPoints[f]->id : -1;
    std::fwrite(ids.data(), 4, ids.size(), o);
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
            Frame& F = *p.cur;
            const Frame& L = *p.last;
            if (p.kind == 0) {
                fill_slots(p, F);
                rsc_orb::ORBmatcher matcher(0.9f, p.check_ori != 0);
                const int32_t n = matcher.SearchByProjection(F, L, p.th);
                std::fwrite(&n, 4, 1, o);
                write_ids(o, F);
            } else {
                // stale state the helper must clear: every slot occupied, every flag set (Tracking.cpp:724)
                F.mvpMapPoints.assign((size_t)F.N, std::make_shared<MapPoint>());
                F.mvbOutlier.assign((size_t)F.N, true);
                bool vo = false;
                rsc_track_motion_result rec;
                const bool ok = rsc_orb::TrackWithMotionModel(F, L, (int)p.th, p.only_tracking != 0, &vo, &rec);
                const int32_t head[8] = {ok, vo, rec.searches, rec.nmatches_search[0], rec.nmatches_search[1],
                                         rec.nmatches, rec.nmatches_map, F.set_pose_calls};
                std::fwrite(head, 4, 8, o);
                std::fwrite(F.mTcw.a, 4, 16, o);
                write_ids(o, F);
                for (int i = 0; i < F.N; ++i) {
                    // mvbOutlier of the slots the optimisation or the discard touched; others stay as they were
                    const int32_t b = F.mvbOutlier[i];
                    std::fwrite(&b, 4, 1, o);
                }
                for (int i = 0; i < L.N; ++i) {
                    int32_t t[2] = {-1, -1};
                    if (L.mvpMapPoints[i]) {
                        t[0] = L.mvpMapPoints[i]->mbTrackInView;
                        t[1] = (int32_t)L.mvpMapPoints[i]->mnLastFrameSeen;
                    }
                    std::fwrite(t, 4, 2, o);
                }
            }
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "facade_lastproj_test: %s\n", e.what());
        return 1;
    }
    std::fclose(o);
    return 0;
}
