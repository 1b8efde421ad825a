// TEST-ONLY host build of the KeyFrame Fuse matcher's device arithmetic (rsc_fusekf.h): the per-pair function
// the kernel runs, driven (a) by a literal sequential loop in the reference's order, which is also the one-core
// CPU baseline of tools/fusekf_bench.py, and (b) by a sequential restatement of the 16-lane window walk of
// fusekf.hip (every lane strides over the columns' entries, the smallest (distance, rank, feature) key wins).
// With -DFKFE_MAIN the file is a stand-alone program that draws its own crowded problem and compares the two
// (run under the host sanitizers by tests/test_cpu_fusekf.py).  The product library never contains this code.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../orb-slam2-optimized_amd/csrc/rsc_fusekf.h"
#include "../proj_emu_common.h"

using namespace rsc;

extern "C" {

struct fkfe_problem {
    // KeyFrame
    int32_t nk;
    const float* kp;
    const int32_t* octave;
    const uint8_t* desc;
    const int32_t* cell_begin;
    const int32_t* cell_feat;
    const float* scale;
    int32_t n_levels;
    float min_x, max_x, min_y, max_y, gw_inv, gh_inv, fx, fy, cx, cy, log_sf;
    const float* u_right;
    float Rcw[9], tcw[3], Ow[3], mbf;
    // points
    int32_t np;
    const uint8_t* state;
    const float* pos;
    const float* normal;
    const float* dmax;
    const float* dmin;
    const uint8_t* pdesc;
    // call
    const uint8_t* skip;
    float th;
};

}  // extern "C"

namespace {

struct Views {
    EmuFrame k;
    std::vector<ProjDesc> pdesc;  // aligned copy
    FuseKfProblem Q;
};

void make_views(const fkfe_problem& p, Views& v) {
    make_frame_view(p, p.nk, nullptr, v.k);
    v.pdesc = emu_aligned_descs(p.pdesc, p.np);
    v.Q = FuseKfProblem{};
    static_cast<DevProjFrame&>(v.Q.K) = v.k.F;
    v.Q.P = DevKfpPoints{p.state, p.pos, p.normal, p.dmax, p.dmin, v.pdesc.data(), p.np};
    std::memcpy(v.Q.Rcw, p.Rcw, sizeof(v.Q.Rcw));
    std::memcpy(v.Q.tcw, p.tcw, sizeof(v.Q.tcw));
    std::memcpy(v.Q.Ow, p.Ow, sizeof(v.Q.Ow));
    v.Q.mbf = p.mbf;
    v.Q.u_right = p.u_right;
    v.Q.skip = p.skip;
}

// proj_first_min_free_coop of rsc_projrounds.h with the lanes run one after another
int coop_point(const FuseKfProblem& Q, int i, float th, int lanes) {
    if (!kfp_eligible(Q.P, Q.skip, i)) return -1;
    const FuseKfRec q = fkf_setup(Q, i, th);
    if (q.cells < 0) return -1;
    const FuseKfGate gate(Q, q);
    const ProjCells w(q.cells);
    unsigned long long best = ~0ull;
    for (int lane = 0; lane < lanes; ++lane) {
        int rank0 = 0;
        for (int ix = w.x0; ix <= w.x1; ++ix) {
            const int b = Q.K.cell_begin[ix * kProjGridRows + w.y0], e1 = Q.K.cell_begin[ix * kProjGridRows + w.y1 + 1];
            for (int e = b + lane; e < e1; e += lanes) {
                const int f = Q.K.cell_feat[e];
                if (!gate(f)) continue;
                const unsigned long long key = (unsigned long long)proj_desc_dist(Q.P.desc[i], Q.K.desc[f]) << 32 |
                                               ((unsigned)(rank0 + (e - b)) << 16 | (unsigned)f);
                if (key < best) best = key;
            }
            rank0 += e1 - b;
        }
    }
    if (best == ~0ull) return -1;
    return (int)(best >> 32) <= kKfpThLow ? (int)(best & 0xffff) : -1;
}

}  // namespace

extern "C" {

// :688-798 point by point: best_idx[i] = bestIdx when bestDist <= TH_LOW, else -1.  Returns their number.
int fkfe_fuse(const fkfe_problem* p, int32_t* best_idx) {
    Views v;
    make_views(*p, v);
    int n = 0;
    for (int i = 0; i < p->np; ++i) {
        best_idx[i] = fkf_point(v.Q, i, p->th);
        n += best_idx[i] >= 0;
    }
    return n;
}

// the same through the window walk by `lanes` lanes
int fkfe_fuse_coop(const fkfe_problem* p, int lanes, int32_t* best_idx) {
    Views v;
    make_views(*p, v);
    int n = 0;
    for (int i = 0; i < p->np; ++i) {
        best_idx[i] = coop_point(v.Q, i, p->th, lanes);
        n += best_idx[i] >= 0;
    }
    return n;
}

// mvInvLevelSigma2 as the gate derives it, for the facade's comparison with the caller's vector
void fkfe_inv_sigma2(const float* scale, int n_levels, float* out) {
    for (int l = 0; l < n_levels; ++l) out[l] = 1.0f / (scale[l] * scale[l]);
}

}  // extern "C"

#ifdef FKFE_MAIN
// A crowded problem drawn here: clusters of keypoints a few pixels apart with near-identical descriptors, a third
// of them stereo, several points per cluster; identity pose, points at z = 4.
namespace {
uint32_t g_state = 4321u;
uint32_t rnd() {
    g_state = g_state * 1664525u + 1013904223u;
    return g_state >> 8;
}
float unif(float a, float b) { return a + (b - a) * (float)(rnd() & 0xffff) / 65536.0f; }
}  // namespace

int main() {
    const int clusters = 30, per_kp = 24, per_pt = 12, nk = clusters * per_kp + 200, np = clusters * per_pt + 400;
    const float W = 752.0f, H = 480.0f, fx = 435.0f, fy = 435.0f, cx = 367.0f, cy = 252.0f, mbf = 40.0f;
    std::vector<float> kp(2 * nk), ur(nk), pos(3 * np), normal(3 * np), dmax(np), dmin(np), scale(8);
    std::vector<int32_t> octave(nk), b1(np), b16(np), b3(np);
    std::vector<uint8_t> desc(32 * (size_t)nk), pdesc(32 * (size_t)np), state(np, 1), skip(np, 0);
    scale[0] = 1.0f;
    for (int l = 1; l < 8; ++l) scale[l] = scale[l - 1] * 1.2f;
    auto place = [&](int i, float u, float v, int level) {
        const float z = 4.0f;
        pos[3 * i] = (u - cx) / fx * z;
        pos[3 * i + 1] = (v - cy) / fy * z;
        pos[3 * i + 2] = z;
        const float d = sqrtf(pos[3 * i] * pos[3 * i] + pos[3 * i + 1] * pos[3 * i + 1] + z * z);
        for (int k = 0; k < 3; ++k) normal[3 * i + k] = pos[3 * i + k] / d;
        dmax[i] = d * powf(1.2f, (float)level - 0.5f);
        dmin[i] = dmax[i] / scale[7];
    };
    int k = 0, i = 0;
    for (int c = 0; c < clusters; ++c) {
        const float u = unif(40, W - 40), v = unif(40, H - 40);
        const int o = 4 + (int)(rnd() % 4);
        uint8_t base[32];
        for (int b = 0; b < 32; ++b) base[b] = (uint8_t)rnd();
        for (int m = 0; m < per_kp; ++m, ++k) {
            kp[2 * k] = u + unif(-6, 6);
            kp[2 * k + 1] = v + unif(-6, 6);
            octave[k] = o - (int)(rnd() % 3);
            ur[k] = rnd() % 3 == 0 ? kp[2 * k] - mbf / 4.0f + unif(-3, 3) : -1.0f;
            std::memcpy(&desc[32 * (size_t)k], base, 32);
            for (int f = 0; f < 3; ++f) desc[32 * (size_t)k + rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
        }
        for (int m = 0; m < per_pt; ++m, ++i) {
            place(i, u + unif(-1, 1), v + unif(-1, 1), o);
            std::memcpy(&pdesc[32 * (size_t)i], base, 32);
            for (int f = 0; f < 2; ++f) pdesc[32 * (size_t)i + rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
        }
    }
    for (; k < nk; ++k) {
        kp[2 * k] = unif(2, W - 2);
        kp[2 * k + 1] = unif(2, H - 2);
        octave[k] = (int)(rnd() % 8);
        ur[k] = rnd() % 3 == 0 ? kp[2 * k] - mbf / 4.0f : -1.0f;
        for (int b = 0; b < 32; ++b) desc[32 * (size_t)k + b] = (uint8_t)rnd();
    }
    for (; i < np; ++i) {
        const int src = (int)(rnd() % nk);
        place(i, kp[2 * src] + unif(-1, 1), kp[2 * src + 1] + unif(-1, 1), octave[src]);
        std::memcpy(&pdesc[32 * (size_t)i], &desc[32 * (size_t)src], 32);
        for (int f = 0; f < 8; ++f) pdesc[32 * (size_t)i + rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
        if (rnd() % 20 == 0) state[i] = 2;
        if (rnd() % 20 == 0) skip[i] = 1;
        if (rnd() % 20 == 0) pos[3 * i + 2] = rnd() % 2 ? -4.0f : 0.0f;  // behind the camera / z == 0
    }
    // mGrid as CSR with PosInGrid's rounding
    const float gw = 64.0f / W, gh = 48.0f / H;
    std::vector<int32_t> begin(64 * 48 + 1, 0), feat(nk), cell(nk);
    for (int f = 0; f < nk; ++f) {
        int px = (int)floorf(kp[2 * f] * gw + 0.5f), py = (int)floorf(kp[2 * f + 1] * gh + 0.5f);
        if (px > 63) px = 63;
        if (py > 47) py = 47;
        if (px < 0) px = 0;
        if (py < 0) py = 0;
        cell[f] = px * 48 + py;
        ++begin[cell[f] + 1];
    }
    for (int c = 0; c < 64 * 48; ++c) begin[c + 1] += begin[c];
    std::vector<int32_t> fill(begin.begin(), begin.end() - 1);
    for (int f = 0; f < nk; ++f) feat[fill[cell[f]]++] = f;
    fkfe_problem p{nk, kp.data(), octave.data(), desc.data(), begin.data(), feat.data(), scale.data(), 8,
                   0.0f, W, 0.0f, H, gw, gh, fx, fy, cx, cy, logf(1.2f), ur.data(),
                   {1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}, {0, 0, 0}, mbf,
                   np, state.data(), pos.data(), normal.data(), dmax.data(), dmin.data(), pdesc.data(),
                   skip.data(), 3.0f};
    const int n1 = fkfe_fuse(&p, b1.data());
    const int n16 = fkfe_fuse_coop(&p, 16, b16.data());
    const int n3 = fkfe_fuse_coop(&p, 3, b3.data());
    int mismatches = (n1 != n16) + (n1 != n3);
    for (int j = 0; j < np; ++j) mismatches += (b1[j] != b16[j]) + (b1[j] != b3[j]);
    std::printf("{\"mismatches\": %d, \"nfused\": %d}\n", mismatches, n1);
    return mismatches ? 1 : 0;
}
#endif
