// TEST INFRASTRUCTURE — parity oracle, never linked into the product library.
//
// Branch record of OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:59-151)
// as the PoseOptimization and OptimizeSim3 oracles restate it: how often one call took each exit of
// the trial loop.  A test reads it to prove that an input reaches the branch it is named for.  The
// record only counts; it is written after the values it looks at are computed and never read back,
// so the oracle's arithmetic is the same with and without it.
#pragma once
#include <cstdint>

namespace rsc_oracle {

struct LmBranches {
    int32_t trials;               // Levenberg trials (linear solves)
    int32_t not_ok2;              // trials whose LDLT was not positive (stale _x reused, tempChi = DBL_MAX)
    int32_t tempchi_nonfinite;    // trials whose activeRobustChi2 was NaN or infinite (before that substitution)
    int32_t rho_nan;              // trials with rho NaN (the trial loop ends without Terminate)
    int32_t rejected;             // trials not accepted (lambda *= ni, estimate popped)
    int32_t end_qmax;             // iterations ended by qmax == 10
    int32_t end_rho0;             // iterations ended by rho == 0 (with qmax < 10)
    int32_t end_nbad;             // iterations ended by nBadLM >= 3
    int32_t no_active_edge;       // optimize() calls that found no level-0 edge
    int32_t currentchi_nonfinite; // iterations entered with a NaN or infinite currentChi
    int32_t not_ok2_accepted;     // trials with !ok2 that were accepted all the same: scale < 0 makes rho > 0,
                                  // and DBL_MAX is finite (the stale _x then moves the estimate)
};
constexpr int kLmBranchFields = sizeof(LmBranches) / sizeof(int32_t);

}  // namespace rsc_oracle
