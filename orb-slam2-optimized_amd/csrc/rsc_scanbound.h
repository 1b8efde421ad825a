// rsc_scanbound.h — the continue rule of pnp_scan_kernel's two-segment counting (host and device).
//
// The replay (rsc_engine.h pnp_iterate_many), pnp_select_refine_kernel and the reference
// (PnPsolver.cpp:147: mnBestInliers moves only inside `if(mnInliersi>=mRansacMinInliers)`) use a
// hypothesis' inlier count in one way: they test it against mRansacMinInliers and look at the
// first hypothesis that reaches it.  A hypothesis with c1 inliers among the first kA of its N
// points can reach at most c1 + (N - kA): when that is below min_inliers it is decided, and the
// remaining N - kA point tests are work nobody reads.
//
// The scan's thread holds PPT slices of 256 points.  For PPT >= 2 segment A is slices
// [0, PPT / 2), kA = min(N, 128 PPT) points, and segment B the rest; PPT == 1 has no segments
// (kA = N).  Tested on the host over every (N, PPT, min_inliers, c1): tests/test_cpu_scan_bound.py.
#pragma once
#include "rsc_core.h"

namespace rsc {

// points of segment A
RSC_HD int scan_seg_a_points(int n, int ppt) {
    const int ka = ppt >= 2 ? 128 * ppt : 256 * ppt;
    return n < ka ? n : ka;
}

// Whether a hypothesis with c1 inliers among the kA points of segment A is counted over segment B.
// bound off: every hypothesis with points in B is.  A hypothesis for which this is false keeps c1 as
// its stored count: exact when kA >= N, below min_inliers otherwise.
RSC_HD bool scan_continue(int n, int ka, int c1, int min_inliers, bool bound) {
    if (n <= ka) return false;  // B is empty
    return !bound || c1 + (n - ka) >= min_inliers;
}

}  // namespace rsc
