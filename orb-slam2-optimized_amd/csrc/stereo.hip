// stereo.hip — Frame::ComputeStereoMatches() (src/Frame.cpp:538-673) over a batch of frames; see rsc_stereo.h
// for the arithmetic and the quirks kept.  Two kernels, one launch each.
// Match: a workgroup owns kStmTile left keypoints of one frame, a wave kStmPerWave of them.  The right frame's
// (y, u, octave) pass through LDS in chunks of kStmChunk; for each of its left keypoints a wave's lanes test
// the gates on 64 staged right keypoints at a time, only survivors load the 32-byte right descriptor, and every
// lane keeps the smallest key it has seen.  A wave min over the keys is the reference's winner.
// Cut: one workgroup per frame builds the histogram of the accepted distances with integer LDS atomics (the
// counts do not depend on their order), one lane derives the median and thDist, and all sweep the keypoints.
#include <hip/hip_runtime.h>
#include "rsc_stereo.h"

namespace rsc {

namespace {

__device__ __forceinline__ unsigned long long wave_min_key(unsigned long long key) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const unsigned long long o = __shfl_xor(key, m);
        key = o < key ? o : key;
    }
    return key;
}

__global__ __launch_bounds__(kStmThreads) void stereo_match_kernel(const StereoProblem* __restrict__ problems) {
    __shared__ float sy[kStmChunk];
    __shared__ float su[kStmChunk];
    __shared__ int so[kStmChunk];
    const StereoProblem P = problems[blockIdx.y];
    const int tile0 = blockIdx.x * kStmTile;
    if (tile0 >= P.n_left) return;  // the whole workgroup: the grid is sized by the longest frame
    const DevProjFrame& F = *P.left;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int first = tile0 + wave * kStmPerWave;
    const float maxD = stm_max_d(P.mbf, P.mb);
    unsigned long long best[kStmPerWave];
#pragma unroll
    for (int k = 0; k < kStmPerWave; ++k) best[k] = kStmNoKey;
    for (int c0 = 0; c0 < P.n_right; c0 += kStmChunk) {  // P.n_right is the workgroup's: every wave takes each barrier
        const int m = min(kStmChunk, P.n_right - c0);
        __syncthreads();  // the previous chunk has been read
        for (int j = threadIdx.x; j < m; j += kStmThreads) {
            const ProjPt p = P.r_kp[c0 + j];
            sy[j] = p.y;
            su[j] = p.x;
            so[j] = P.r_octave[c0 + j];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kStmPerWave; ++k) {
            const int i = first + k;
            if (i >= P.n_left) break;  // the wave's
            const int level = F.octave[i];
            const StereoLeft L = stm_left(F.kp[i], level, F.scale[level], maxD);
            if (!L.live) continue;
            const ProjDesc dl = F.desc[i];
            for (int j = lane; j < m; j += 64) {
                const float yR = sy[j];
                if (!stm_gate(L, yR, su[j], so[j])) continue;
                const unsigned long long key = stm_key(proj_desc_dist(dl, P.r_desc[c0 + j]), yR, c0 + j);
                best[k] = key < best[k] ? key : best[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kStmPerWave; ++k) {
        const int i = first + k;
        if (i >= P.n_left) break;
        const unsigned long long key = wave_min_key(best[k]);
        if (lane == 0) {
            const int level = F.octave[i];
            stm_finish(P, i, stm_left(F.kp[i], level, F.scale[level], maxD), maxD, key);
        }
    }
}

__global__ __launch_bounds__(kStmCutThreads) void stereo_cut_kernel(const StereoProblem* __restrict__ problems) {
    __shared__ int hist[kStmThOrbDist];
    __shared__ int removed;
    __shared__ StereoOut cut;
    const StereoProblem P = problems[blockIdx.x];
    const int tid = threadIdx.x;
    if (tid < kStmThOrbDist) hist[tid] = 0;
    if (tid == 0) removed = 0;
    __syncthreads();
    for (int i = tid; i < P.n_left; i += kStmCutThreads) {
        const int d = P.best_dist[i];  // -1, or 0 .. 74
        if (d >= 0) atomicAdd(&hist[d], 1);
    }
    __syncthreads();
    if (tid == 0) cut = stm_cut_threshold(hist);
    __syncthreads();
    const StereoOut o = cut;
    int mine = 0;
    for (int i = tid; i < P.n_left; i += kStmCutThreads) {
        float u = P.u_right[i];
        if (stm_cut_removes(o, P.best_dist[i])) {
            u = -1.0f;
            P.u_right[i] = -1.0f;
            P.depth[i] = -1.0f;
            ++mine;
        }
        if (P.view_uright) P.view_uright[i] = u;
    }
    if (mine) atomicAdd(&removed, mine);
    __syncthreads();
    if (tid == 0) {
        StereoOut r = o;
        r.n_removed = removed;
        *P.result = r;
    }
}

}  // namespace

hipError_t launch_stereo(const StereoProblem* problems, int count, int max_left, hipEvent_t mid, hipStream_t st) {
    if (count <= 0) return hipSuccess;
    if (max_left > 0) {
        const dim3 g((max_left + kStmTile - 1) / kStmTile, count);
        stereo_match_kernel<<<g, kStmThreads, 0, st>>>(problems);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    if (mid) (void)hipEventRecord(mid, st);
    stereo_cut_kernel<<<count, kStmCutThreads, 0, st>>>(problems);
    return hipGetLastError();
}

}  // namespace rsc
