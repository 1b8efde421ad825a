// TEST-ONLY host build of the MapPoint update's device arithmetic (rsc_mpupdate.h): the per-row and per-point
// functions the two kernels of mpupdate.hip run, driven in the kernels' lane decompositions with the lanes run one
// after another (mode 1: one row per lane for lists of up to 64 observations, rows strided over 256 lanes above),
// next to a plain sequential restatement of MapPoint.cpp:224-289 and :312-353 with the N x N matrix and the sorted
// rows (mode 0), which is also the one-core CPU baseline of tools/mpupdate_bench.py.  With -DMPUE_MAIN the file is
// a stand-alone program that draws its own problem and compares the two (run under the host sanitizers by
// tests/test_cpu_mpupdate.py).  The product library never contains this code.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../orb-slam2-optimized_amd/csrc/rsc_mpupdate.h"
#include "../proj_emu_common.h"

using namespace rsc;

extern "C" {

struct mpue_kf {
    int32_t n;
    const uint8_t* desc;
    const int32_t* octave;
    const float* scale;
    int32_t n_levels;
    float Ow[3];
};

struct mpue_problem {
    int32_t n_kfs;
    const mpue_kf* kfs;
    const uint8_t* kf_bad;  // may be NULL
    int32_t n_points;
    const uint8_t* skip;
    const float* pos;
    const int32_t* obs_begin;
    const int32_t* obs_kf;
    const int32_t* obs_idx;
    const int32_t* ref_kf;
    const int32_t* ref_idx;
};

struct mpue_out {
    uint8_t* desc;
    int32_t* best_obs;
    float* normal;
    float* dmax;
    float* dmin;
    uint8_t* updated;
};

}  // extern "C"

namespace {

int hamming(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int k = 0; k < 4; ++k) {
        uint64_t x, y;
        std::memcpy(&x, a + 8 * k, 8);
        std::memcpy(&y, b + 8 * k, 8);
        d += __builtin_popcountll(x ^ y);
    }
    return d;
}

bool active(const mpue_problem& p, int i) { return !p.skip[i] && p.obs_begin[i + 1] > p.obs_begin[i]; }

// ---- mode 0: the reference's two functions, line by line ------------------------------------------------------
void sequential_point(const mpue_problem& p, int i, int what, const mpue_out& out) {
    const int ob = p.obs_begin[i], n = p.obs_begin[i + 1] - ob;
    if (what & 1) {
        std::vector<const uint8_t*> v;  // vDescriptors
        std::vector<int> at;
        for (int o = 0; o < n; ++o) {
            const int k = p.obs_kf[ob + o];
            if (!(p.kf_bad && p.kf_bad[k])) {  // :247
                v.push_back(p.kfs[k].desc + 32 * (size_t)p.obs_idx[ob + o]);
                at.push_back(o);
            }
        }
        out.best_obs[i] = -1;
        if (!v.empty()) {  // :251
            const size_t N = v.size();
            std::vector<float> D(N * N);  // float Distances[N][N]
            for (size_t a = 0; a < N; ++a) {
                D[a * N + a] = 0;
                for (size_t b = a + 1; b < N; ++b) {
                    const int d = hamming(v[a], v[b]);
                    D[a * N + b] = (float)d;
                    D[b * N + a] = (float)d;
                }
            }
            int BestMedian = INT_MAX, BestIdx = 0;
            std::vector<int> vDists(N);
            for (size_t a = 0; a < N; ++a) {
                for (size_t b = 0; b < N; ++b) vDists[b] = (int)D[a * N + b];
                std::sort(vDists.begin(), vDists.end());
                const int median = vDists[(size_t)(0.5 * (N - 1))];
                if (median < BestMedian) {
                    BestMedian = median;
                    BestIdx = (int)a;
                }
            }
            out.best_obs[i] = at[BestIdx];
            std::memcpy(out.desc + 32 * (size_t)i, v[BestIdx], 32);
            out.updated[i] |= 1;
        }
    }
    if (what & 2) {
        const float* Pos = p.pos + 3 * (size_t)i;
        float normal[3] = {0.0f, 0.0f, 0.0f};
        for (int o = 0; o < n; ++o) {  // :332-339
            const float* Ow = p.kfs[p.obs_kf[ob + o]].Ow;
            const float ni[3] = {Pos[0] - Ow[0], Pos[1] - Ow[1], Pos[2] - Ow[2]};
            const float nrm = sqrtf((ni[0] * ni[0] + ni[1] * ni[1]) + ni[2] * ni[2]);
            for (int k = 0; k < 3; ++k) normal[k] = normal[k] + ni[k] / nrm;
        }
        const mpue_kf& ref = p.kfs[p.ref_kf[i]];
        const float PC[3] = {Pos[0] - ref.Ow[0], Pos[1] - ref.Ow[1], Pos[2] - ref.Ow[2]};
        const float dist = sqrtf((PC[0] * PC[0] + PC[1] * PC[1]) + PC[2] * PC[2]);
        const int level = ref.octave[p.ref_idx[i]];
        out.dmax[i] = dist * ref.scale[level];
        out.dmin[i] = out.dmax[i] / ref.scale[ref.n_levels - 1];
        for (int k = 0; k < 3; ++k) out.normal[3 * (size_t)i + k] = normal[k] / (float)n;
        out.updated[i] |= 2;
    }
}

// ---- mode 1: the kernels' decomposition ------------------------------------------------------------------------
struct DeviceImage {
    std::vector<std::vector<ProjDesc>> kdesc;
    std::vector<MpuKF> kfs;
    std::vector<int32_t> kept_begin, kept_pos;
    std::vector<ProjDesc> desc;
    std::vector<int32_t> best_obs;
    std::vector<float> normal, dmax, dmin;
    MpuProblem Q{};
};

void make_image(const mpue_problem& p, int what, DeviceImage& m) {
    for (int k = 0; k < p.n_kfs; ++k) {
        m.kdesc.push_back(emu_aligned_descs(p.kfs[k].desc, p.kfs[k].n));
        MpuKF e{m.kdesc.back().data(), p.kfs[k].octave, p.kfs[k].scale, {p.kfs[k].Ow[0], p.kfs[k].Ow[1], p.kfs[k].Ow[2]},
                p.kfs[k].n_levels};
        m.kfs.push_back(e);
    }
    for (int k = 0; k < p.n_kfs; ++k) m.kfs[k].desc = m.kdesc[k].data();
    m.kept_begin.assign((size_t)p.n_points + 1, 0);
    for (int i = 0; i < p.n_points; ++i) {
        m.kept_begin[i + 1] = m.kept_begin[i];
        if (!active(p, i)) continue;
        for (int o = p.obs_begin[i]; o < p.obs_begin[i + 1]; ++o)
            if (!(p.kf_bad && p.kf_bad[p.obs_kf[o]])) {
                m.kept_pos.push_back(o - p.obs_begin[i]);
                ++m.kept_begin[i + 1];
            }
    }
    m.kept_pos.push_back(0);
    const size_t n = (size_t)p.n_points;
    m.desc.resize(n + 1);
    m.best_obs.assign(n + 1, -9);
    m.normal.assign(3 * n + 1, 0.0f);
    m.dmax.assign(n + 1, 0.0f);
    m.dmin.assign(n + 1, 0.0f);
    MpuProblem& Q = m.Q;
    Q.kfs = m.kfs.data();
    Q.pos = p.pos;
    Q.obs_begin = p.obs_begin;
    Q.obs_kf = p.obs_kf;
    Q.obs_idx = p.obs_idx;
    Q.kept_begin = m.kept_begin.data();
    Q.kept_pos = m.kept_pos.data();
    Q.ref_kf = p.ref_kf;
    Q.ref_idx = p.ref_idx;
    Q.desc = m.desc.data();
    Q.best_obs = m.best_obs.data();
    Q.normal = m.normal.data();
    Q.dmax = m.dmax.data();
    Q.dmin = m.dmin.data();
    Q.what = what;
}

// mpupdate_wave_kernel for one point: lane i owns row i and observation i
void wave_point(const MpuProblem& Q, int p) {
    if (Q.what & 1) {
        const int N = Q.kept_begin[p + 1] - Q.kept_begin[p];
        ProjDesc sd[kMpuWaveObs];
        int my_pos[kMpuWaveObs];
        for (int lane = 0; lane < N; ++lane) {
            my_pos[lane] = mpu_kept_pos(Q, p, lane);
            sd[lane] = mpu_obs_desc(Q, p, my_pos[lane]);
        }
        int key = kMpuNoKey;
        for (int lane = 0; lane < kMpuWaveObs; ++lane)
            if (lane < N) key = std::min(key, mpu_key(mpu_row_median(sd[lane], sd, N), lane));
        if (N == 0) Q.best_obs[p] = -1;
        else mpu_store_desc(Q, p, my_pos[mpu_key_row(key)], sd[mpu_key_row(key)]);
    }
    if (Q.what & 2) {
        const int ob = Q.obs_begin[p], n = Q.obs_begin[p + 1] - ob;
        const float* pos = Q.pos + 3 * (size_t)p;
        float u[kMpuWaveObs][3];
        for (int lane = 0; lane < n; ++lane) mpu_unit(pos, Q.kfs[Q.obs_kf[ob + lane]].Ow, u[lane]);
        float sum[3] = {0.0f, 0.0f, 0.0f};
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k) sum[k] = sum[k] + u[i][k];
        float normal[3], dmax, dmin;
        mpu_finish(pos, Q.kfs[Q.ref_kf[p]], Q.ref_idx[p], sum, n, normal, dmax, dmin);
        mpu_store_normal(Q, p, normal, dmax, dmin);
    }
}

// mpupdate_block_kernel for one point: 256 lanes stride over the observations and the rows
void block_point(const MpuProblem& Q, int p) {
    if (Q.what & 2) {
        const int ob = Q.obs_begin[p], n = Q.obs_begin[p + 1] - ob;
        const float* pos = Q.pos + 3 * (size_t)p;
        std::vector<float> su(3 * (size_t)kMpuMaxObs);
        for (int tid = 0; tid < kMpuThreads; ++tid)
            for (int i = tid; i < n; i += kMpuThreads) {
                float u[3];
                mpu_unit(pos, Q.kfs[Q.obs_kf[ob + i]].Ow, u);
                su[i] = u[0];
                su[kMpuMaxObs + i] = u[1];
                su[2 * kMpuMaxObs + i] = u[2];
            }
        float sum[3] = {0.0f, 0.0f, 0.0f};
        for (int i = 0; i < n; ++i) {
            sum[0] = sum[0] + su[i];
            sum[1] = sum[1] + su[kMpuMaxObs + i];
            sum[2] = sum[2] + su[2 * kMpuMaxObs + i];
        }
        float normal[3], dmax, dmin;
        mpu_finish(pos, Q.kfs[Q.ref_kf[p]], Q.ref_idx[p], sum, n, normal, dmax, dmin);
        mpu_store_normal(Q, p, normal, dmax, dmin);
    }
    if (Q.what & 1) {
        const int N = Q.kept_begin[p + 1] - Q.kept_begin[p];
        if (N == 0) {
            Q.best_obs[p] = -1;
            return;
        }
        std::vector<ProjDesc> sd((size_t)N);
        for (int r = 0; r < N; ++r) sd[r] = mpu_obs_desc(Q, p, mpu_kept_pos(Q, p, r));
        int wave_key[kMpuThreads / 64];
        for (int& k : wave_key) k = kMpuNoKey;
        for (int tid = 0; tid < kMpuThreads; ++tid) {
            int key = kMpuNoKey;
            for (int r = tid; r < N; r += kMpuThreads) key = std::min(key, mpu_key(mpu_row_median(sd[r], sd.data(), N), r));
            wave_key[tid >> 6] = std::min(wave_key[tid >> 6], key);
        }
        int best = wave_key[0];
        for (int w = 1; w < kMpuThreads / 64; ++w) best = std::min(best, wave_key[w]);
        const int pos = mpu_kept_pos(Q, p, mpu_key_row(best));
        mpu_store_desc(Q, p, pos, mpu_obs_desc(Q, p, pos));
    }
}

}  // namespace

extern "C" {

// Both functions over the batch.  mode 0: the sequential restatement; 1: the kernels' decomposition.  Entries of
// `out` that are not written keep their values; updated is written for every point.  Returns 0, or -1 when a
// list of a point to update is longer than RSC_MPUPDATE_MAX_OBS (nothing is written then).
int mpue_update(const mpue_problem* p, int what, int mode, const mpue_out* out) {
    for (int i = 0; i < p->n_points; ++i)
        if (active(*p, i) && p->obs_begin[i + 1] - p->obs_begin[i] > kMpuMaxObs) return -1;
    for (int i = 0; i < p->n_points; ++i) out->updated[i] = 0;
    if (mode == 0) {
        for (int i = 0; i < p->n_points; ++i)
            if (active(*p, i)) sequential_point(*p, i, what, *out);
        return 0;
    }
    DeviceImage m;
    make_image(*p, what, m);
    for (int i = 0; i < p->n_points; ++i) {
        if (!active(*p, i)) continue;
        if (p->obs_begin[i + 1] - p->obs_begin[i] <= kMpuWaveObs) wave_point(m.Q, i);
        else block_point(m.Q, i);
        if (what & 1) {
            out->best_obs[i] = m.best_obs[i];
            if (m.best_obs[i] >= 0) {
                std::memcpy(out->desc + 32 * (size_t)i, &m.desc[i], 32);
                out->updated[i] |= 1;
            }
        }
        if (what & 2) {
            std::memcpy(out->normal + 3 * (size_t)i, &m.normal[3 * (size_t)i], 12);
            out->dmax[i] = m.dmax[i];
            out->dmin[i] = m.dmin[i];
            out->updated[i] |= 2;
        }
    }
    return 0;
}

// mpu_row_median of every kept row of point i (medians: as many entries as kept observations).  Returns their number.
int mpue_medians(const mpue_problem* p, int i, int32_t* medians) {
    DeviceImage m;
    make_image(*p, 1, m);
    const int N = m.kept_begin[i + 1] - m.kept_begin[i];
    std::vector<ProjDesc> sd((size_t)N + 1);
    for (int r = 0; r < N; ++r) sd[r] = mpu_obs_desc(m.Q, i, mpu_kept_pos(m.Q, i, r));
    for (int r = 0; r < N; ++r) medians[r] = mpu_row_median(sd[r], sd.data(), N);
    return N;
}

}  // extern "C"

#ifdef MPUE_MAIN
// A problem drawn here: three KeyFrames (one bad) of 1,100 keypoints whose descriptors are a few centres with
// flipped bits, one point per list length of both classes and their boundary, a bad point, an empty list, a
// point on a camera centre.
namespace {
uint32_t g_state = 97531u;
uint32_t rnd() {
    g_state = g_state * 1664525u + 1013904223u;
    return g_state >> 8;
}
float unif(float a, float b) { return a + (b - a) * (float)(rnd() & 0xffff) / 65536.0f; }
}  // namespace

int main() {
    const int n_kfs = 3, nk = 1100;
    const int sizes[] = {1, 2, 3, 63, 64, 65, 200, 1024, 0, 7, 9};
    const int np = (int)(sizeof(sizes) / sizeof(sizes[0]));
    std::vector<float> scale(8);
    scale[0] = 1.0f;
    for (int l = 1; l < 8; ++l) scale[l] = scale[l - 1] * 1.2f;
    uint8_t centre[5][32];
    for (auto& c : centre)
        for (int b = 0; b < 32; ++b) c[b] = (uint8_t)rnd();
    std::vector<std::vector<uint8_t>> desc(n_kfs, std::vector<uint8_t>(32 * (size_t)nk));
    std::vector<std::vector<int32_t>> octave(n_kfs, std::vector<int32_t>(nk));
    std::vector<mpue_kf> kfs(n_kfs);
    for (int k = 0; k < n_kfs; ++k) {
        for (int i = 0; i < nk; ++i) {
            std::memcpy(&desc[k][32 * (size_t)i], centre[rnd() % 5], 32);
            for (int f = (int)(rnd() % 30); f > 0; --f) desc[k][32 * (size_t)i + rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
            octave[k][i] = (int)(rnd() % 8);
        }
        kfs[k] = mpue_kf{nk, desc[k].data(), octave[k].data(), scale.data(), 8, {unif(-3, 3), unif(-3, 3), unif(-3, 3)}};
    }
    const uint8_t kf_bad[3] = {0, 1, 0};
    std::vector<int32_t> begin(np + 1, 0), okf, oidx, rkf(np), ridx(np);
    std::vector<float> pos(3 * (size_t)np);
    std::vector<uint8_t> skip(np, 0);
    for (int i = 0; i < np; ++i) {
        for (int o = 0; o < sizes[i]; ++o) {
            okf.push_back((int)(rnd() % n_kfs));
            oidx.push_back((int)(rnd() % nk));
        }
        begin[i + 1] = (int)okf.size();
        for (int k = 0; k < 3; ++k) pos[3 * (size_t)i + k] = unif(-2, 2) + (k == 2 ? 6.0f : 0.0f);
        rkf[i] = sizes[i] ? okf[begin[i]] : 0;
        ridx[i] = sizes[i] ? oidx[begin[i]] : 0;
    }
    skip[np - 1] = 1;                                                // a bad point
    for (int k = 0; k < 3; ++k) pos[3 * (size_t)(np - 2) + k] = kfs[okf[begin[np - 2]]].Ow[k];  // on a camera centre
    okf.push_back(0);
    oidx.push_back(0);
    mpue_problem p{n_kfs, kfs.data(), kf_bad, np, skip.data(), pos.data(), begin.data(), okf.data(), oidx.data(),
                   rkf.data(), ridx.data()};
    struct Result {
        std::vector<uint8_t> desc, updated;
        std::vector<int32_t> best;
        std::vector<float> normal, dmax, dmin;
        explicit Result(int n) : desc(32 * (size_t)n, 0xA5), updated(n, 0xFF), best(n, -7), normal(3 * (size_t)n, -77.0f),
                                 dmax(n, -77.0f), dmin(n, -77.0f) {}
        mpue_out out() { return mpue_out{desc.data(), best.data(), normal.data(), dmax.data(), dmin.data(), updated.data()}; }
    };
    int mismatches = 0, updated = 0;
    for (int what = 1; what <= 3; ++what) {
        Result a(np), b(np);
        const mpue_out oa = a.out(), ob = b.out();
        mismatches += mpue_update(&p, what, 0, &oa) != 0;
        mismatches += mpue_update(&p, what, 1, &ob) != 0;
        mismatches += a.desc != b.desc;
        mismatches += a.updated != b.updated;
        mismatches += a.best != b.best;
        mismatches += std::memcmp(a.normal.data(), b.normal.data(), 12 * (size_t)np) != 0;
        mismatches += std::memcmp(a.dmax.data(), b.dmax.data(), 4 * (size_t)np) != 0;
        mismatches += std::memcmp(a.dmin.data(), b.dmin.data(), 4 * (size_t)np) != 0;
        for (uint8_t u : a.updated) updated += u != 0;
    }
    // one observation too many is refused by both
    std::vector<int32_t> big_kf(kMpuMaxObs + 1, 0), big_idx(kMpuMaxObs + 1, 0);
    const int32_t big_begin[2] = {0, kMpuMaxObs + 1}, zero = 0;
    const uint8_t no_skip = 0;
    mpue_problem big{n_kfs, kfs.data(), nullptr, 1, &no_skip, pos.data(), big_begin, big_kf.data(), big_idx.data(), &zero,
                     &zero};
    Result r(1);
    const mpue_out orr = r.out();
    const int refused = (mpue_update(&big, 3, 0, &orr) == -1) + (mpue_update(&big, 3, 1, &orr) == -1);
    mismatches += refused != 2 || r.updated[0] != 0xFF;
    std::printf("{\"mismatches\": %d, \"updated\": %d, \"refused\": %d}\n", mismatches, updated, refused);
    return mismatches ? 1 : 0;
}
#endif
