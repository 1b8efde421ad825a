// Drives rsc_orb::ComputeStereoMatches(F) and ComputeStereoMatches(F, view) (facade/Frame.hpp) with a mock Frame
// built from a binary file written by tests/test_gpu_facade_stereo.py, and writes what the two calls left in
// mvuRight / mvDepth and their records back.  After the call on a kept view the program also runs
// rsc_frameview_set_stereo-dependent code on it: the local-map matcher over an empty point list, which refuses a
// view without mvuRight.  Needs a GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "Frame.hpp"

struct Pt { float x, y; };
struct KeyPoint { Pt pt; int octave; float angle; };
struct DescMat {
    std::vector<uint8_t> d;
    template <class T> const T* ptr(int row) const { return reinterpret_cast<const T*>(d.data() + 32 * (size_t)row); }
};

struct Frame {
    int N = 0;
    std::vector<KeyPoint> mvKeysUn, mvKeysRight;
    DescMat mDescriptors, mDescriptorsRight;
    std::vector<std::size_t> mGrid[64][48];
    float mnMinX = 0, mnMaxX = 752, mnMinY = 0, mnMaxY = 480;
    float mfGridElementWidthInv = 64.0f / 752.0f, mfGridElementHeightInv = 48.0f / 480.0f;
    float fx = 458.654f, fy = 457.296f, cx = 367.215f, cy = 248.375f;
    std::vector<float> mvScaleFactors;
    int mnScaleLevels = 0;
    float mfLogScaleFactor = 0;
    float mbf = 0, mb = 0;
    std::vector<float> mvuRight, mvDepth;
    void AssignFeaturesToGrid() {  // Frame.cpp:267-280 with PosInGrid (:449-461)
        for (int i = 0; i < N; ++i) {
            const int px = (int)std::round((mvKeysUn[i].pt.x - mnMinX) * mfGridElementWidthInv);
            const int py = (int)std::round((mvKeysUn[i].pt.y - mnMinY) * mfGridElementHeightInv);
            if (px < 0 || px >= 64 || py < 0 || py >= 48) continue;
            mGrid[px][py].push_back((std::size_t)i);
        }
    }
};

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

static bool read_keys(FILE* f, std::vector<KeyPoint>& keys, DescMat& desc) {
    int32_t n = 0;
    if (!rd(f, &n, 1) || n < 0) return false;
    std::vector<float> kp(2 * (size_t)n);
    std::vector<int32_t> oct((size_t)n);
    desc.d.resize(32 * (size_t)n);
    if (!rd(f, kp.data(), kp.size()) || !rd(f, oct.data(), oct.size()) || !rd(f, desc.d.data(), desc.d.size())) return false;
    keys.resize((size_t)n);
    for (int i = 0; i < n; ++i) keys[i] = KeyPoint{{kp[2 * i], kp[2 * i + 1]}, oct[i], 0.0f};
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    Frame F;
    int32_t levels = 0;
    bool ok = rd(f, &levels, 1) && levels > 0 && levels <= 64;
    if (ok) {
        F.mvScaleFactors.resize((size_t)levels);
        F.mnScaleLevels = levels;
        ok = rd(f, F.mvScaleFactors.data(), (size_t)levels) && rd(f, &F.mfLogScaleFactor, 1) && rd(f, &F.mbf, 1) &&
             rd(f, &F.mb, 1) && read_keys(f, F.mvKeysUn, F.mDescriptors) && read_keys(f, F.mvKeysRight, F.mDescriptorsRight);
    }
    std::fclose(f);
    if (!ok) return 2;
    F.N = (int)F.mvKeysUn.size();
    F.AssignFeaturesToGrid();
    const size_t n = (size_t)F.N;
    int32_t status = 0;
    std::vector<float> u0, z0, u1, z1;
    rsc_stereo_result r0{}, r1{};
    try {
        r0 = rsc_orb::ComputeStereoMatches(F);
        u0 = F.mvuRight;
        z0 = F.mvDepth;
        F.mvuRight.assign(n, 123.0f);
        F.mvDepth.assign(n, 123.0f);
        rsc_orb::detail::FrameViewUpload view = rsc_orb::detail::upload_frameview(F);
        // the matcher over no points: RSC_ERR_ARG before the stereo call, RSC_OK after it
        auto local = [&]() {
            rsc_mappoints none{};
            rsc_mpview* mv = nullptr;
            rsc_orb::check(rsc_mpview_create(rsc_orb::thread_context(), &none, &mv), "rsc_mpview_create");
            const float Tcw[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
            std::vector<uint8_t> zeros(n + 1, 0);
            std::vector<int32_t> out(n + 1, 0);
            const uint8_t* zp = zeros.data();
            int32_t* op = out.data();
            int32_t nm = 0, ntm = 0;
            rsc_track_record rec{};
            rsc_track_record* tp = &rec;
            const int st = rsc_search_local_points_many(rsc_orb::thread_context(), &view.h, &mv, 1, Tcw, &zp, &zp, &zp, 0.5f,
                                                        1.0f, 0.8f, &op, &tp, &nm, &ntm, nullptr);
            rsc_mpview_destroy(mv);
            return st;
        };
        if (local() != RSC_ERR_ARG) status |= 1;
        r1 = rsc_orb::ComputeStereoMatches(F, view);
        u1 = F.mvuRight;
        z1 = F.mvDepth;
        if (local() != RSC_OK) status |= 2;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    if (u0.size() != n || z0.size() != n || u1.size() != n || z1.size() != n) status |= 4;
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const int32_t head[2] = {status, (int32_t)n};
    std::fwrite(head, 4, 2, o);
    std::fwrite(&r0, sizeof(r0), 1, o);
    std::fwrite(&r1, sizeof(r1), 1, o);
    for (const auto* v : {&u0, &z0, &u1, &z1})
        if (n && v->size() == n) std::fwrite(v->data(), 4, n, o);
    std::fclose(o);
    return 0;
}
