// TEST-ONLY stand-alone program: the sequential LocalBundleAdjustment restatement (tests/localba_emu, mode 0) and the
// kernels' decomposition (mode 1) on four scenes drawn here — a regular mixed mono / stereo window, one with gross
// outliers that make vertices leave the active set, one without an edge and one with a NaN point — compared byte for
// byte, and the reduced solve alone on a singular system.  Built plain and under the host address / undefined-behaviour sanitizers (tests/test_cpu_localba.py runs
// both); nothing of it is loaded into Python.
#include "../localba_emu/localba_emu.cpp"

#include <cmath>
#include <cstdlib>

namespace {

struct Lcg {
    uint64_t s;
    double next() {  // [0, 1)
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        return (double)(s >> 11) / 9007199254740992.0;
    }
    double sym(double a) { return (2.0 * next() - 1.0) * a; }
};

struct Scene {
    std::vector<int64_t> kf_id, mp_id;
    std::vector<uint8_t> fixed, bad;
    std::vector<float> Tcw, cam, pos, uv, ur, inv;
    std::vector<int32_t> obs_begin, obs_kf;
    rsc_localba_problem view() const {
        rsc_localba_problem q;
        q.n_kfs = (int32_t)kf_id.size(); q.kf_id = kf_id.data(); q.fixed = fixed.data(); q.Tcw = Tcw.data();
        q.cam = cam.data(); q.n_points = (int32_t)mp_id.size(); q.mp_id = mp_id.data(); q.pos = pos.data();
        q.bad = bad.data(); q.obs_begin = obs_begin.data(); q.obs_kf = obs_kf.data(); q.uv = uv.data();
        q.u_right = ur.data(); q.inv_sigma2 = inv.data();
        return q;
    }
};

// K KeyFrames along x with identity rotations (the first n_fixed fixed, ids descending so that list order is not
// index order), N points in front of them, every point seen by 2..4 of them
Scene draw(uint64_t seed, int K, int n_fixed, int N, double outlier_frac, bool with_edges) {
    Lcg g{seed};
    Scene s;
    const double fx = 500, fy = 500, cx = 320, cy = 240, bf = 40;
    for (int k = 0; k < K; ++k) {
        s.kf_id.push_back(100 - 3 * k);
        s.fixed.push_back(k < n_fixed ? 1 : 0);
        float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        T[3] = (float)(-0.3 * k + (k >= n_fixed ? g.sym(0.01) : 0.0));
        T[7] = (float)(k >= n_fixed ? g.sym(0.01) : 0.0);
        s.Tcw.insert(s.Tcw.end(), T, T + 16);
        const float c[5] = {(float)fx, (float)fy, (float)cx, (float)cy, (float)bf};
        s.cam.insert(s.cam.end(), c, c + 5);
    }
    s.obs_begin.push_back(0);
    for (int i = 0; i < N; ++i) {
        s.mp_id.push_back(7 + 2 * (int64_t)((i * 7) % N));
        s.bad.push_back(0);
        const double X[3] = {g.sym(1.0) + 0.15 * K, g.sym(1.0), 4.0 + 5.0 * g.next()};
        for (int j = 0; j < 3; ++j) s.pos.push_back((float)(X[j] + g.sym(0.03)));
        if (with_edges) {
            const int m = std::min(K, 2 + (int)(3 * g.next()));
            const int first = (int)(g.next() * K);
            for (int o = 0; o < m; ++o) {
                const int k = (first + o) % K;
                const double x = X[0] - 0.3 * k, z = X[2];
                double u = fx * x / z + cx + g.sym(0.5), v = fy * X[1] / z + cy + g.sym(0.5);
                if (g.next() < outlier_frac) {
                    u += 80.0;
                    v -= 60.0;
                }
                s.obs_kf.push_back(k);
                s.uv.push_back((float)u);
                s.uv.push_back((float)v);
                s.ur.push_back(g.next() < 0.6 ? (float)(u - bf / z) : -1.0f);
                s.inv.push_back((float)(1.0 / std::pow(1.2, 2 * (int)(4 * g.next()))));
            }
        }
        s.obs_begin.push_back((int32_t)s.obs_kf.size());
    }
    return s;
}

int compare(const char* name, const Scene& s) {
    const rsc_localba_problem q = s.view();
    const size_t K = s.kf_id.size(), N = s.mp_id.size(), E = s.obs_kf.size();
    std::vector<float> T[2], X[2];
    std::vector<uint8_t> F[2];
    std::vector<int32_t> R[2];
    rsc_localba_result res[2];
    for (int mode = 0; mode < 2; ++mode) {
        T[mode].assign(16 * K + 1, -77.0f);
        X[mode].assign(3 * N + 1, -77.0f);
        F[mode].assign(E + 1, 0xA5);
        R[mode].assign(E + 1, -7);
        const rsc_localba_out o{T[mode].data(), X[mode].data(), F[mode].data(), R[mode].data()};
        const int st = lbae_run(&q, mode, &o, &res[mode]);
        if (st != 0) {
            std::printf("%s: mode %d status %d\n", name, mode, st);
            return 1;
        }
    }
    const bool same = std::memcmp(T[0].data(), T[1].data(), 4 * T[0].size()) == 0 &&
                      std::memcmp(X[0].data(), X[1].data(), 4 * X[0].size()) == 0 && F[0] == F[1] && R[0] == R[1] &&
                      std::memcmp(&res[0], &res[1], sizeof(res[0])) == 0;
    std::printf("%s: edges %zu erase %d level1 %d iterations %d+%d trials %d+%d status %d %s\n", name, E, res[0].n_erase,
                res[0].n_level1, res[0].phase[0].lm_iterations, res[0].phase[1].lm_iterations,
                res[0].phase[0].lm_trials, res[0].phase[1].lm_trials, res[0].status, same ? "same" : "DIFFERENT");
    return same ? 0 : 1;
}

}  // namespace

int main() {
    int bad = 0;
    bad += compare("regular", draw(1, 6, 2, 60, 0.0, true));
    bad += compare("outliers", draw(2, 5, 2, 40, 0.15, true));
    bad += compare("no_edges", draw(3, 3, 1, 5, 0.0, false));
    Scene nan = draw(4, 4, 2, 20, 0.0, true);
    nan.pos[4] = std::nanf("");
    bad += compare("nan_point", nan);
    // the reduced solve alone: a singular system is refused by both forms and leaves x alone
    const double A[4] = {0.0, 1.0, 1.0, 2.0}, b[2] = {1.0, 1.0};
    double x0[2] = {5.0, 6.0}, x1[2] = {5.0, 6.0};
    if (lbae_solve(2, A, b, 0, x0) != 0 || lbae_solve(2, A, b, 1, x1) != 0 || x0[0] != 5.0 || x1[1] != 6.0) {
        std::printf("zero pivot: not refused\n");
        ++bad;
    }
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
