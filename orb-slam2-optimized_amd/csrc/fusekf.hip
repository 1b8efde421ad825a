// fusekf.hip — ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cpp:671-821) kernel, the matcher of
// LocalMapping::SearchInNeighbors; see rsc_fusekf.h for the quirks kept.  Every (point, KeyFrame) pair is
// decided alone, so there are no rounds, no LDS and no hand-off: one launch over grid (pairs, problems).
#include <hip/hip_runtime.h>
#include "rsc_fusekf.h"
#include "rsc_projrounds.h"

// Lanes that walk one pair's window together: kProjSub (16), or 1 for the one-lane-per-pair form of
// kffuse_kernel (an A/B build: make -C tools variant NAME=fusekf1 SRC=fusekf DEFS=-DRSC_FUSEKF_LANES=1).
// Which of the two is the default and what each measured: DESIGN.md §7.
#ifndef RSC_FUSEKF_LANES
#define RSC_FUSEKF_LANES 16
#endif

namespace rsc {

namespace {

constexpr int kFkfThreads = 256;
static_assert(RSC_FUSEKF_LANES == 1 || RSC_FUSEKF_LANES == kProjSub, "RSC_FUSEKF_LANES is 1 or kProjSub");

// kLanes lanes per pair.  The lanes of a pair all run the projection (the same loads, one transaction) and
// stride over the window's columns (proj_walk_coop); the smallest (distance, visiting rank) key among them is
// the sequential walk's first strict minimum.  A pair's lanes leave together (i is theirs in common), so the
// shuffles of proj_min_coop stay inside one subgroup.
template <int kLanes>
__global__ __launch_bounds__(kFkfThreads) void fusekf_kernel(const FuseKfProblem* __restrict__ problems, float th) {
    const FuseKfProblem& Q = problems[blockIdx.y];
    if constexpr (kLanes == 1) {
        const int i = blockIdx.x * kFkfThreads + threadIdx.x;
        if (i < Q.P.n) Q.best_idx[i] = fkf_point(Q, i, th);
    } else {
        const int i = blockIdx.x * (kFkfThreads / kLanes) + threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
        if (i >= Q.P.n) return;
        int b = -1;
        if (kfp_eligible(Q.P, Q.skip, i)) {  // :695, the same for the pair's lanes
            const FuseKfRec q = fkf_setup(Q, i, th);
            b = proj_first_min_free_coop<kLanes>(Q.K, q.cells, Q.P.desc[i], FuseKfGate(Q, q), kKfpThLow, lane);
        }
        if (lane == 0) Q.best_idx[i] = b;
    }
}

}  // namespace

hipError_t launch_fuse_kf(int count, int max_points, const FuseKfProblem* problems, float th, hipStream_t st) {
    if (count <= 0 || max_points <= 0) return hipSuccess;
    constexpr int per_block = kFkfThreads / RSC_FUSEKF_LANES;
    const dim3 g((max_points + per_block - 1) / per_block, count);
    fusekf_kernel<RSC_FUSEKF_LANES><<<g, kFkfThreads, 0, st>>>(problems, th);
    return hipGetLastError();
}

}  // namespace rsc
