// TEST-ONLY host program (tests/test_cpu_scan_bound.py): the continue rule of pnp_scan_kernel's
// two-segment counting (rsc_scanbound.h) over every N in 1..1100, PPT = ppt_for(N) and its doubles up
// to 32, every min_inliers in 1..N and every c1 in 0..kA.  The rule must reject exactly when
// c1 + max(0, N - kA) < min_inliers or segment B is empty, and never continue when kA >= N; with the
// bound off it continues exactly when B has points.  Prints one JSON line.
#include <cstdint>
#include <cstdio>

#include "../../orb-slam2-optimized_amd/csrc/rsc_scanbound.h"

static int ppt_for(int n) {  // rsc_api.cpp
    const int need = (n + 255) / 256;
    int p = 1;
    while (p < need) p <<= 1;
    return p;
}

int main() {
    int64_t cases = 0, mismatches = 0, continued = 0, rejected = 0, empty_b_continued = 0, ka_wrong = 0, off_wrong = 0;
    for (int n = 1; n <= 1100; ++n) {
        for (int ppt = ppt_for(n); ppt <= 32; ppt *= 2) {
            const int ka = rsc::scan_seg_a_points(n, ppt);
            // segment A is slices [0, PPT / 2) of 256 points for PPT >= 2, everything for PPT 1
            const int want_ka = ppt >= 2 ? (n < 128 * ppt ? n : 128 * ppt) : n;
            if (ka != want_ka || ka < 0 || ka > n) ++ka_wrong;
            const int rest = n - ka > 0 ? n - ka : 0;
            for (int c1 = 0; c1 <= ka; ++c1) {
                if (rsc::scan_continue(n, ka, c1, 1, false) != (rest > 0)) ++off_wrong;
                for (int mi = 1; mi <= n; ++mi) {
                    const bool go = rsc::scan_continue(n, ka, c1, mi, true);
                    // the model: a hypothesis is decided when even all of B cannot lift it to min_inliers;
                    // with B empty there is nothing left to count
                    const bool reject = c1 + rest < mi;
                    const bool want = !reject && rest > 0;
                    ++cases;
                    if (go != want) ++mismatches;
                    if (go && ka >= n) ++empty_b_continued;
                    // a rejected hypothesis with points left keeps c1, which must then be below min_inliers
                    if (!go && rest > 0 && !(c1 < mi)) ++mismatches;
                    go ? ++continued : ++rejected;
                }
            }
        }
    }
    std::printf("{\"cases\": %lld, \"mismatches\": %lld, \"continued\": %lld, \"rejected\": %lld, "
                "\"empty_b_continued\": %lld, \"ka_wrong\": %lld, \"off_wrong\": %lld}\n",
                (long long)cases, (long long)mismatches, (long long)continued, (long long)rejected,
                (long long)empty_b_continued, (long long)ka_wrong, (long long)off_wrong);
    return (mismatches || empty_b_continued || ka_wrong || off_wrong) ? 1 : 0;
}
