// localba.hip — the stage kernels of Optimizer::LocalBundleAdjustment (rsc_localba.h holds the arithmetic of
// every item).  One problem is large and usually alone, so each stage of a Levenberg
// trial is a launch of its own spread over the device: edges one per lane, the vertex sums one lane per
// (vertex, entry) walking the vertex's edges in active-edge order, the Schur update one workgroup per pose block
// with one lane per entry walking the landmarks in ascending index, the reduced LDL^T on one workgroup, the
// back-substitution and update one lane per vertex, and the chi2 / scale sums and the LM bookkeeping on one lane.
// Whatever runs in parallel belongs to different sums; every sum meets its terms in the stated order.
#include <hip/hip_runtime.h>
#include "rsc_localba.h"

namespace rsc {

namespace {

constexpr int kLbaThreads = 256;
constexpr int kLbaSolveThreads = 1024;

// BUILD: linearise and write the 72 terms too (once per LM iteration); without it the trial's errors and chi2 terms
template <bool BUILD>
__global__ __launch_bounds__(kLbaThreads) void lba_edges_kernel(LbaDev D) {
    const int a = blockIdx.x * kLbaThreads + threadIdx.x;
    if (a < D.na) lba_edge_item(D, a, BUILD);
}

// items: [0, 12 L) the points' entries, then [0, 42 F) the poses'
__global__ __launch_bounds__(kLbaThreads) void lba_fold_kernel(LbaDev D) {
    const int i = blockIdx.x * kLbaThreads + threadIdx.x;
    const int np = 12 * D.L;
    if (i < np) lba_fold_point_item(D, i / 12, i % 12);
    else if (i - np < 42 * D.F) lba_fold_kf_item(D, (i - np) / 42, (i - np) % 42);
}

__global__ __launch_bounds__(64) void lba_ctl_begin_kernel(LbaDev D, int it) {
    if (threadIdx.x == 0) lba_ctl_begin(D, it);
}

__global__ __launch_bounds__(kLbaThreads) void lba_point_prep_kernel(LbaDev D) {
    const int l = blockIdx.x * kLbaThreads + threadIdx.x;
    if (l < D.L) lba_point_prep_item(D, l);
}

// one workgroup per block (i1, i2) of the F x F grid; lanes 0..35 its entries, lanes 36..41 of a diagonal
// block the pose's bschur entries.  Blocks below the diagonal are not part of the system.
__global__ __launch_bounds__(64) void lba_schur_kernel(LbaDev D) {
    const int i1 = blockIdx.x / D.F, i2 = blockIdx.x % D.F, t = threadIdx.x;
    if (i2 < i1) return;
    if (t < 36) lba_schur_item(D, i1, i2, t / 6, t % 6);
    else if (t < 42 && i1 == i2) lba_bschur_item(D, i1, t - 36);
}

// The reduced solve on one workgroup: the right-looking LDL^T over the upper triangle of S (n <= 384, in HBM / L2),
// then z = L^-1 bschur by columns, z_j = (1 / D_j) z_j, and x_j = z_j - sum over i > j, ascending, of L(i, j) x_i with
// the products of a row computed by the workgroup and folded by lane 0.  A zero pivot ends it with ok2 = 0 and x
// untouched.
__global__ __launch_bounds__(kLbaSolveThreads) void lba_solve_kernel(LbaDev D) {
    __shared__ double z[6 * kLbaMaxFree];
    __shared__ double pr[6 * kLbaMaxFree];
    const int n = D.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int kWaves = kLbaSolveThreads / 64;
    double* S = D.S;
    bool ok = true;
    for (int i = 0; i < n; ++i) {
        __syncthreads();
        const double d = S[(size_t)i * n + i];
        if (d == 0.0) {  // every lane reads the same word
            ok = false;
            break;
        }
        for (int j = i + 1 + tid; j < n; j += kLbaSolveThreads) lba_ldlt_scale_item(S, n, i, j, d);
        __syncthreads();
        for (int j = i + 1 + wave; j < n; j += kWaves)
            for (int k = j + lane; k < n; k += 64) lba_ldlt_update_item(S, n, i, j, k);
    }
    __syncthreads();
    if (!ok) {
        if (tid == 0) D.ctl->ok2 = 0;
        return;
    }
    for (int j = tid; j < n; j += kLbaSolveThreads) z[j] = D.bs[j];
    for (int i = 0; i < n; ++i) {
        __syncthreads();
        const double zi = z[i];
        for (int j = i + 1 + tid; j < n; j += kLbaSolveThreads) z[j] = z[j] - S[(size_t)j * n + i] * zi;
    }
    __syncthreads();
    for (int j = tid; j < n; j += kLbaSolveThreads) z[j] = (1.0 / S[(size_t)j * n + j]) * z[j];
    for (int j = n - 1; j >= 0; --j) {
        __syncthreads();
        for (int i = j + 1 + tid; i < n; i += kLbaSolveThreads) pr[i] = S[(size_t)i * n + j] * z[i];  // z[i] holds x_i
        __syncthreads();
        if (tid == 0) {
            double acc = z[j];
            for (int i = j + 1; i < n; ++i) acc = acc - pr[i];
            z[j] = acc;
        }
    }
    __syncthreads();
    for (int j = tid; j < n; j += kLbaSolveThreads) D.x[j] = z[j];
    if (tid == 0) D.ctl->ok2 = 1;
}

// items: [0, F) the poses, then [0, L) the points
__global__ __launch_bounds__(kLbaThreads) void lba_update_kernel(LbaDev D) {
    const int i = blockIdx.x * kLbaThreads + threadIdx.x;
    if (i < D.F) lba_kf_update_item(D, i);
    else if (i - D.F < D.L) lba_point_update_item(D, i - D.F);
}

__global__ __launch_bounds__(64) void lba_ctl_trial_kernel(LbaDev D) {
    if (threadIdx.x == 0) lba_ctl_trial(D);
}

__global__ __launch_bounds__(kLbaThreads) void lba_restore_kernel(LbaDev D) {
    const int i = blockIdx.x * kLbaThreads + threadIdx.x;
    if (i < D.F + D.L) lba_restore_item(D, i);
}

__global__ __launch_bounds__(kLbaThreads) void lba_classify_kernel(LbaDev D, int phase) {
    const int e = blockIdx.x * kLbaThreads + threadIdx.x;
    if (e < D.n_edges) lba_classify_item(D, e, phase);
}

inline int lba_grid(int items) { return (items + kLbaThreads - 1) / kLbaThreads; }

}  // namespace

hipError_t launch_lba_edges(const LbaDev& D, bool build, hipStream_t st) {
    if (D.na <= 0) return hipSuccess;
    if (build) lba_edges_kernel<true><<<lba_grid(D.na), kLbaThreads, 0, st>>>(D);
    else lba_edges_kernel<false><<<lba_grid(D.na), kLbaThreads, 0, st>>>(D);
    return hipGetLastError();
}

hipError_t launch_lba_fold(const LbaDev& D, hipStream_t st) {
    const int items = 12 * D.L + 42 * D.F;
    if (items <= 0) return hipSuccess;
    lba_fold_kernel<<<lba_grid(items), kLbaThreads, 0, st>>>(D);
    return hipGetLastError();
}

hipError_t launch_lba_ctl_begin(const LbaDev& D, int it, hipStream_t st) {
    lba_ctl_begin_kernel<<<1, 64, 0, st>>>(D, it);
    return hipGetLastError();
}

hipError_t launch_lba_point_prep(const LbaDev& D, hipStream_t st) {
    if (D.L <= 0) return hipSuccess;
    lba_point_prep_kernel<<<lba_grid(D.L), kLbaThreads, 0, st>>>(D);
    return hipGetLastError();
}

hipError_t launch_lba_schur(const LbaDev& D, hipStream_t st) {
    if (D.F <= 0) return hipSuccess;
    lba_schur_kernel<<<D.F * D.F, 64, 0, st>>>(D);
    return hipGetLastError();
}

hipError_t launch_lba_solve(const LbaDev& D, hipStream_t st) {
    lba_solve_kernel<<<1, kLbaSolveThreads, 0, st>>>(D);
    return hipGetLastError();
}

hipError_t launch_lba_update(const LbaDev& D, hipStream_t st) {
    if (D.F + D.L <= 0) return hipSuccess;
    lba_update_kernel<<<lba_grid(D.F + D.L), kLbaThreads, 0, st>>>(D);
    return hipGetLastError();
}

hipError_t launch_lba_ctl_trial(const LbaDev& D, hipStream_t st) {
    lba_ctl_trial_kernel<<<1, 64, 0, st>>>(D);
    return hipGetLastError();
}

hipError_t launch_lba_restore(const LbaDev& D, hipStream_t st) {
    if (D.F + D.L <= 0) return hipSuccess;
    lba_restore_kernel<<<lba_grid(D.F + D.L), kLbaThreads, 0, st>>>(D);
    return hipGetLastError();
}

hipError_t launch_lba_classify(const LbaDev& D, int phase, hipStream_t st) {
    if (D.n_edges <= 0) return hipSuccess;
    lba_classify_kernel<<<lba_grid(D.n_edges), kLbaThreads, 0, st>>>(D, phase);
    return hipGetLastError();
}

}  // namespace rsc
