// mpupdate.hip — MapPoint::ComputeDistinctiveDescriptors() and MapPoint::UpdateNormalAndDepth()
// (src/MapPoint.cpp:224-289, :312-353) over a batch of points; see rsc_mpupdate.h for the arithmetic and the quirks
// kept.  Two kernels, one launch each: lists of up to 64 observations take one wave per point (lane i owns row i of
// the distance matrix and observation i of the normal), longer lists one workgroup per point (rows and
// observations strided over its lanes).  The kept descriptors are staged in LDS and every lane reads descriptor j
// at the same time (a broadcast, no bank conflict); a row's median comes from mpu_row_median's bisection, so no
// lane holds more than its own descriptor.  The normal's sum runs on one lane in list order.
#include <hip/hip_runtime.h>
#include "rsc_mpupdate.h"

namespace rsc {

namespace {

constexpr int kMpuWaves = kMpuThreads / 64;
static_assert(kMpuWaveObs == 64, "one lane per observation of a wave-class list");
static_assert(sizeof(ProjDesc) * kMpuMaxObs <= 32768, "the staged descriptors of the longest list fit 32 KB of LDS");

__device__ __forceinline__ int wave_min(int key) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) key = min(key, __shfl_xor(key, m));
    return key;
}

// One point per wave, four points per workgroup.  Every wave of a workgroup reaches the barrier.
__global__ __launch_bounds__(kMpuThreads) void mpupdate_wave_kernel(const MpuProblem Q) {
    __shared__ ProjDesc sd[kMpuWaves][kMpuWaveObs];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slot = blockIdx.x * kMpuWaves + wave;
    const bool active = slot < Q.n_wave;
    const int p = active ? Q.order[slot] : 0;
    const bool with_desc = active && (Q.what & 1);
    int N = 0, my_pos = 0;
    ProjDesc own = {};
    if (with_desc) {
        N = Q.kept_begin[p + 1] - Q.kept_begin[p];  // <= 64: the class holds lists of at most 64 observations
        if (lane < N) {
            my_pos = mpu_kept_pos(Q, p, lane);
            own = mpu_obs_desc(Q, p, my_pos);
            sd[wave][lane] = own;
        }
    }
    __syncthreads();
    if (with_desc) {
        int key = kMpuNoKey;
        if (lane < N) key = mpu_key(mpu_row_median(own, sd[wave], N), lane);
        key = wave_min(key);
        if (N == 0) {
            if (lane == 0) Q.best_obs[p] = -1;
        } else if (lane == mpu_key_row(key)) {
            mpu_store_desc(Q, p, my_pos, own);
        }
    }
    if (active && (Q.what & 2)) {
        const int ob = Q.obs_begin[p], n = Q.obs_begin[p + 1] - ob;  // 1 <= n <= 64
        const float pos[3] = {Q.pos[3 * p], Q.pos[3 * p + 1], Q.pos[3 * p + 2]};
        float u[3] = {0.0f, 0.0f, 0.0f};
        if (lane < n) mpu_unit(pos, Q.kfs[Q.obs_kf[ob + lane]].Ow, u);
        float sum[3] = {0.0f, 0.0f, 0.0f};
        for (int i = 0; i < n; ++i) {  // lane 0's sum is the one kept; every lane runs the shuffles
            sum[0] = sum[0] + __shfl(u[0], i);
            sum[1] = sum[1] + __shfl(u[1], i);
            sum[2] = sum[2] + __shfl(u[2], i);
        }
        if (lane == 0) {
            float normal[3], dmax, dmin;
            mpu_finish(pos, Q.kfs[Q.ref_kf[p]], Q.ref_idx[p], sum, n, normal, dmax, dmin);
            mpu_store_normal(Q, p, normal, dmax, dmin);
        }
    }
}

// One point per workgroup.  The 32 KB of LDS hold, one after the other, the unit vectors of the normal (12 bytes
// per observation), the kept descriptors, and the waves' keys.
__global__ __launch_bounds__(kMpuThreads) void mpupdate_block_kernel(const MpuProblem Q) {
    __shared__ ProjDesc sd[kMpuMaxObs];
    const int tid = threadIdx.x;
    const int p = Q.order[Q.n_wave + blockIdx.x];
    if (Q.what & 2) {
        float* su = reinterpret_cast<float*>(sd);  // [3][kMpuMaxObs]
        const int ob = Q.obs_begin[p], n = Q.obs_begin[p + 1] - ob;  // 64 < n <= 1024
        const float pos[3] = {Q.pos[3 * p], Q.pos[3 * p + 1], Q.pos[3 * p + 2]};
        for (int i = tid; i < n; i += kMpuThreads) {
            float u[3];
            mpu_unit(pos, Q.kfs[Q.obs_kf[ob + i]].Ow, u);
            su[i] = u[0];
            su[kMpuMaxObs + i] = u[1];
            su[2 * kMpuMaxObs + i] = u[2];
        }
        __syncthreads();
        if (tid == 0) {
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
        __syncthreads();  // the unit vectors make room for the descriptors
    }
    if (Q.what & 1) {
        const int N = Q.kept_begin[p + 1] - Q.kept_begin[p];  // <= 1024
        if (N == 0) {
            if (tid == 0) Q.best_obs[p] = -1;
            return;  // the whole workgroup: N is the point's
        }
        for (int r = tid; r < N; r += kMpuThreads) sd[r] = mpu_obs_desc(Q, p, mpu_kept_pos(Q, p, r));
        __syncthreads();
        int key = kMpuNoKey;
        for (int r = tid; r < N; r += kMpuThreads) {
            const ProjDesc own = sd[r];
            key = min(key, mpu_key(mpu_row_median(own, sd, N), r));
        }
        key = wave_min(key);
        __syncthreads();  // every row is done: the descriptors make room for the waves' keys
        int* sk = reinterpret_cast<int*>(sd);
        if ((tid & 63) == 0) sk[tid >> 6] = key;
        __syncthreads();
        if (tid == 0) {
            int best = sk[0];
#pragma unroll
            for (int w = 1; w < kMpuWaves; ++w) best = min(best, sk[w]);
            const int pos = mpu_kept_pos(Q, p, mpu_key_row(best));
            mpu_store_desc(Q, p, pos, mpu_obs_desc(Q, p, pos));  // from the KeyFrame: sd[0] holds the keys now
        }
    }
}

}  // namespace

hipError_t launch_mpupdate(const MpuProblem& Q, hipStream_t st) {
    if (Q.n_wave > 0) {
        mpupdate_wave_kernel<<<(Q.n_wave + kMpuWaves - 1) / kMpuWaves, kMpuThreads, 0, st>>>(Q);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    if (Q.n_block > 0) {
        mpupdate_block_kernel<<<Q.n_block, kMpuThreads, 0, st>>>(Q);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace rsc
