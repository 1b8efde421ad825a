// triang.hip — ORBmatcher::SearchForTriangulation (src/ORBmatcher.cpp:489-669) and the pair geometry of
// LocalMapping::CreateNewMapPoints (src/LocalMapping.cpp:262-407).  See rsc_triang.h for the mapping.
#include <hip/hip_runtime.h>
#include "rsc_triang.h"

namespace rsc {
namespace {

constexpr uint32_t kIdx = ~kBowInvalid;

// ORBmatcher::DescriptorDistance (ORBmatcher.cpp:1492-1508): the popcount of the XOR words
__device__ __forceinline__ uint32_t desc_dist(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// ------------------------------------------------------------------------------------------------
// Kernel 0: the items of a problem (one 256-thread workgroup per problem).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTriThreads) void tri_join_kernel(const TriMatchProblem* __restrict__ probs,
                                                              int2* __restrict__ nodeinfo_all) {
    __shared__ int cnt[kTriClasses + 1];
    const TriMatchProblem& P = probs[blockIdx.x];
    const DevBow& A = P.A;
    const DevBow& B = P.B;
    const int tid = threadIdx.x, lane = tid & 63;
    const int nn = A.n_nodes;
    const int nfA = nn ? A.node_begin[nn] : 0;
    // the problem's slice of the node table: kTriMaxFeatures entries per problem
    int2* nodeinfo = nodeinfo_all + (size_t)blockIdx.x * kTriMaxFeatures;
    if (tid <= kTriClasses) cnt[tid] = 0;
    __syncthreads();
    for (int i = tid; i < A.n; i += kTriThreads) {
        P.matches12[i] = -1;
        P.den_zero_slot[i] = 0;
    }
    if (tid < 2) P.counts[tid] = 0;
    // the merge walk of :523-635 visits exactly the node ids both FeatureVectors hold
    int common = 0;
    for (int k = tid; k < nn; k += kTriThreads) {
        const uint32_t id = A.node_id[k];
        int lo = 0, hi = B.n_nodes;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (B.node_id[mid] < id) lo = mid + 1;
            else hi = mid;
        }
        const bool hit = lo < B.n_nodes && B.node_id[lo] == id;
        const int b0 = hit ? B.node_begin[lo] : 0;
        nodeinfo[k] = make_int2(b0, hit ? B.node_begin[lo + 1] - b0 : -1);
        common += hit;
    }
    if (common) atomicAdd(&cnt[kTriClasses], common);
    __threadfence_block();
    __syncthreads();
    // every FeatureVector entry of KeyFrame 1: its node, eligibility (:531-541: has1 carries the MapPoint test
    // and, under bOnlyStereo, the stereo test), its class
    for (int e0 = tid - lane; e0 < nfA; e0 += kTriThreads) {
        const int e = e0 + lane;
        int cls = -1;
        int2 ni = make_int2(0, -1);
        if (e < nfA) {
            int lo = 0, hi = nn - 1;  // the node k with node_begin[k] <= e < node_begin[k + 1]
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (A.node_begin[mid + 1] <= e) lo = mid + 1;
                else hi = mid;
            }
            ni = nodeinfo[lo];
            const int idx1 = (int)(A.feat[e] & kIdx);
            if (ni.y >= 0 && !P.has1[idx1]) cls = tri_class_of(ni.y);
        }
#pragma unroll
        for (int c = 0; c < kTriClasses; ++c) {
            const uint64_t m = __ballot(cls == c);
            if (!m) continue;
            int base = 0;
            if (lane == 0) base = atomicAdd(&cnt[c], (int)__popcll(m));
            base = __shfl(base, 0);
            if (cls == c) {
                const int off = (int)__popcll(m & ((1ull << lane) - 1ull));
                P.items[(size_t)c * nfA + base + off] = make_int4(e, ni.x, ni.y, 0);
            }
        }
    }
    __syncthreads();
    if (tid <= kTriClasses) P.nitems[tid] = cnt[tid];
}

// ------------------------------------------------------------------------------------------------
// Kernel 1: a group of G lanes per item (grid (kTriMatchGroups, problems)).
// ------------------------------------------------------------------------------------------------
template <int G>
__device__ __forceinline__ void match_class(const TriMatchProblem& P, const int4* __restrict__ items, int total) {
    const DevBow& A = P.A;
    const DevBow& B = P.B;
    constexpr int gpb = kTriThreads / G;
    const int gid = blockIdx.x * gpb + (int)threadIdx.x / G, gl = (int)threadIdx.x % G;
    const int S = gridDim.x * gpb;
    for (int base = 0; base < total; base += S) {  // uniform over the workgroup: the shuffles below see all lanes
        const int item = base + gid;
        const bool act = item < total;
        const int4 it = items[act ? item : 0];
        const int e1 = it.x, b0 = it.y, nb = act ? it.z : 0;
        const int idx1 = (int)(A.feat[e1] & kIdx);
        const float2 k1 = P.kp1[idx1];
        const bool stereo1 = P.ur1[idx1] >= 0;  // `>= 0` (:537), not the other matchers' `> 0`
        float a, b, c, den;
        tri_epiline(P.F, k1.x, k1.y, a, b, c, den);
        const bool dz = act && den == 0;  // :552
        const uint4 d0 = A.desc_fv[2 * e1], d1 = A.desc_fv[2 * e1 + 1];
        uint32_t key = kTriNoKey;
        for (int q = gl; q < (dz ? 0 : nb); q += G) {
            const int eb = b0 + q;
            const int idx2 = (int)(B.feat[eb] & kIdx);
            // :567 `vbMatched2[idx2] || pMP2`: vbMatched2 is never set (nothing after :604 writes it), so
            // the term is always false and is not kept; has2 also carries bOnlyStereo's test of :572-574
            if (P.has2[idx2]) continue;
            const bool stereo2 = P.ur2[idx2] >= 0;
            const uint32_t dist = desc_dist(d0, d1, B.desc_fv[2 * eb], B.desc_fv[2 * eb + 1]);
            // :580 `dist > TH_LOW || dist > bestDist`: 50 is kept; the running best is the group's minimum
            if (dist > (uint32_t)kTriThLow) continue;
            const float2 k2 = P.kp2[idx2];
            const float sf2 = P.scale2[P.oct2[idx2]];
            if (tri_candidate_ok(a, b, c, den, P.ex, P.ey, stereo1, stereo2, k2.x, k2.y, sf2))
                key = min(key, tri_key(dist, (uint32_t)q));
        }
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, off));
        if (gl == 0 && act) {
            if (dz) {
                P.den_zero_slot[idx1] = 1;
                P.counts[1] = 1;
            } else if (key != kTriNoKey) {
                P.matches12[idx1] = (int32_t)(B.feat[b0 + (int)tri_key_pos(key)] & kIdx);
            }
        }
    }
}

__global__ __launch_bounds__(kTriThreads) void tri_match_kernel(const TriMatchProblem* __restrict__ probs) {
    const TriMatchProblem& P = probs[blockIdx.y];
    const int nn = P.A.n_nodes;
    const int nfA = nn ? P.A.node_begin[nn] : 0;
    match_class<4>(P, P.items, P.nitems[0]);
    match_class<16>(P, P.items + (size_t)nfA, P.nitems[1]);
    match_class<64>(P, P.items + 2 * (size_t)nfA, P.nitems[2]);
}

// ------------------------------------------------------------------------------------------------
// Kernel 2: den_zero, the orientation mask, the count (one workgroup per problem).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTriThreads) void tri_finish_kernel(const TriMatchProblem* __restrict__ probs,
                                                                int check_ori) {
    __shared__ int hist[32];
    __shared__ int keep[3];
    __shared__ int total;
    const TriMatchProblem& P = probs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63;
    const int n = P.A.n;
    // `return false` (:552-553): no match survives; the slot flags stay for the driver.  Bit 1 of check_ori
    // (the driver's speculation, orientation off): the matches stay too, since the replay may find every
    // den == 0 slot filled by an earlier neighbour and then needs them
    const bool speculative = (check_ori & 2) != 0;
    check_ori &= 1;
    if (P.counts[1] && !speculative) {
        for (int i = tid; i < n; i += kTriThreads) P.matches12[i] = -1;
        return;
    }
    if (tid < 32) hist[tid] = 0;
    if (tid == 0) total = 0;
    __syncthreads();
    if (check_ori) {
        for (int i = tid; i < n; i += kTriThreads) {
            const int v = P.matches12[i];
            if (v < 0) continue;
            const int bin = tri_rot_bin(P.angle1[i], P.angle2[v]);
            if ((unsigned)bin < 30u) atomicAdd(&hist[bin], 1);  // finite angles give 0..12; the reference asserts
        }
        __syncthreads();
        if (tid == 0) {
            const TriMaxima mx = tri_three_maxima([&](int i) { return hist[i]; });
            keep[0] = mx.ind1; keep[1] = mx.ind2; keep[2] = mx.ind3;
        }
        __syncthreads();
    }
    int cnt = 0;
    for (int i = tid; i < n; i += kTriThreads) {
        int v = P.matches12[i];
        if (v >= 0 && check_ori) {
            // each slot sits in one bin's list once, so the per-entry removal of :645-654 is a mask
            const int bin = tri_rot_bin(P.angle1[i], P.angle2[v]);
            if (bin != keep[0] && bin != keep[1] && bin != keep[2]) {
                v = -1;
                P.matches12[i] = -1;
            }
        }
        cnt += v >= 0;
    }
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (lane == 0 && cnt) atomicAdd(&total, cnt);
    __syncthreads();
    if (tid == 0) P.counts[0] = total;
}

// ------------------------------------------------------------------------------------------------
// The pair geometry: one lane per matched pair (grid (pairs / 64, problems)).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void tri_pairs_kernel(const TriPairsProblem* __restrict__ probs) {
    const TriPairsProblem& P = probs[blockIdx.y];
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= P.npairs) return;
    float x3D[3];
    const int32_t st = tri_pair(P.K1, P.K2, P.pairs[2 * i], P.pairs[2 * i + 1], x3D);
    P.status[i] = st;
    P.x3d[3 * i] = x3D[0];
    P.x3d[3 * i + 1] = x3D[1];
    P.x3d[3 * i + 2] = x3D[2];
}

}  // namespace

hipError_t launch_search_for_triangulation(int count, const TriMatchProblem* probs, int2* nodeinfo, int check_ori,
                                           hipStream_t st) {
    tri_join_kernel<<<count, kTriThreads, 0, st>>>(probs, nodeinfo);
    tri_match_kernel<<<dim3(kTriMatchGroups, count), kTriThreads, 0, st>>>(probs);
    tri_finish_kernel<<<count, kTriThreads, 0, st>>>(probs, check_ori);
    return hipGetLastError();
}

hipError_t launch_triangulate_pairs(int count, int max_pairs, const TriPairsProblem* probs, hipStream_t st) {
    if (max_pairs > 0) tri_pairs_kernel<<<dim3((max_pairs + 63) / 64, count), 64, 0, st>>>(probs);
    return hipGetLastError();
}

}  // namespace rsc
