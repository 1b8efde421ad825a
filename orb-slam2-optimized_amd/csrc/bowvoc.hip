// bowvoc.hip — the vocabulary transform (ComputeBoW) kernels; see rsc_bowvoc.h for the mapping.
#include "rsc_bowvoc.h"

namespace rsc {
namespace {

__device__ inline uint32_t hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// Descent of one feature per SG-lane subgroup.  grid = (ceil(max_n / features per workgroup), views).
// Dynamic LDS: lds_nodes * (32 B descriptor) then lds_nodes * (8 B record).
template <int SG>
__global__ __launch_bounds__(kVocDescendThreads) void voc_descend_kernel(DevVoc V, const VocJob* __restrict__ jobs,
                                                                         int nid_level) {
    extern __shared__ uint4 s_mem[];
    constexpr int kPerWg = kVocDescendThreads / SG;
    const VocJob J = jobs[blockIdx.y];
    if ((int)blockIdx.x * kPerWg >= J.n) return;  // whole workgroup: no barrier is passed by a part of it
    uint4* s_desc = s_mem;
    uint2* s_rec = reinterpret_cast<uint2*>(s_mem + 2 * (size_t)V.lds_nodes);
    for (int i = threadIdx.x; i < 2 * V.lds_nodes; i += kVocDescendThreads) s_desc[i] = V.desc[i];
    for (int i = threadIdx.x; i < V.lds_nodes; i += kVocDescendThreads) s_rec[i] = V.rec[i];
    __syncthreads();

    const int sub = threadIdx.x / SG, lane = threadIdx.x % SG;
    const int f = blockIdx.x * kPerWg + sub;
    const bool live = f < J.n;
    const int fr = live ? f : J.n - 1;  // idle subgroups repeat the last feature and store nothing
    const uint4 q0 = J.desc[2 * (size_t)fr], q1 = J.desc[2 * (size_t)fr + 1];

    uint32_t cur = 0, nid = 0;
    bool done = false;
    for (int depth = 1; depth <= V.max_depth; ++depth) {
        uint32_t key = 0xFFFFFFFFu;
        uint32_t begin = 0;
        if (!done) {
            const uint2 r = cur < (uint32_t)V.lds_nodes ? s_rec[cur] : V.rec[cur];
            begin = r.x;
            if (r.y == 0) {
                done = true;
            } else if ((uint32_t)lane < r.y) {
                const uint32_t c = begin + lane;
                uint4 c0, c1;
                if (c < (uint32_t)V.lds_nodes) {
                    c0 = s_desc[2 * c];
                    c1 = s_desc[2 * c + 1];
                } else {
                    c0 = V.desc[2 * (size_t)c];
                    c1 = V.desc[2 * (size_t)c + 1];
                }
                key = (hamming256(q0, q1, c0, c1) << 8) | (uint32_t)lane;
            }
        }
#pragma unroll
        for (int m = SG / 2; m >= 1; m >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)key, m, SG);
            key = o < key ? o : key;
        }
        if (!done) {
            cur = begin + (key & 0xFFu);
            if (depth == nid_level) nid = V.orig[cur];
        }
    }
    if (live && lane == 0) {
        J.f_word[f] = V.word[cur];
        J.f_node[f] = nid;
        J.f_weight[f] = V.weight[cur];
    }
}

// ---- build: one workgroup per view ----

// lane l's value as a wave-uniform operand (two v_readlane_b32; __shfl would go through the LDS crossbar)
__device__ inline double readlane_f64(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// exclusive scan of one int per thread over the workgroup; *total = the sum
__device__ inline int block_exscan(int v, int* s_wave, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();  // s_wave may still be read from the previous scan
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int base = 0, sum = 0;
    for (int w = 0; w < kVocBuildThreads / 64; ++w) {
        const int t = s_wave[w];
        if (w < wave) base += t;
        sum += t;
    }
    *total = sum;
    return base + inc - v;
}

// ascending bitonic sort of the N (a power of two) keys (kw, kf) held in LDS.  Pair i of a step with
// distance j lies in the 2j-aligned block of elements around it, so for j <= 64 a wave (64
// consecutive pairs) only touches its own 128 elements in every such step: those steps need no
// workgroup barrier, only program order within the wave (10 barriers instead of 66 for 2048 keys).
__device__ inline void bitonic_sort(uint32_t* kw, uint16_t* kf, int N) {
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            if (j >= 64) __syncthreads();  // the previous step's pairs crossed waves, or this one's do
            else __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            for (int i = threadIdx.x; i < N / 2; i += kVocBuildThreads) {
                const int lo = 2 * i - (i & (j - 1)), hi = lo + j;  // (i / j) * 2j + i % j, j a power of two
                const uint32_t aw = kw[lo], bw = kw[hi];
                const uint16_t af = kf[lo], bf = kf[hi];
                const bool gt = aw > bw || (aw == bw && af > bf);
                if (gt == ((lo & k) == 0)) {
                    kw[lo] = bw; kw[hi] = aw;
                    kf[lo] = bf; kf[hi] = af;
                }
            }
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(kVocBuildThreads) void voc_build_kernel(const VocJob* __restrict__ jobs) {
    __shared__ uint32_t kw[kVocMaxFeatures];
    __shared__ uint16_t kf[kVocMaxFeatures];
    __shared__ int s_wave[kVocBuildThreads / 64];
    __shared__ double s_norm;
    const VocJob J = jobs[blockIdx.x];
    const int n = J.n, tid = threadIdx.x;
    int N = 64;
    while (N < n) N <<= 1;
    const int per = (N + kVocBuildThreads - 1) / kVocBuildThreads;

    // ---- BowVector: sort (word id, feature); stopped features and the padding go to the end ----
    int live = 0;
    for (int i = tid; i < N; i += kVocBuildThreads) {
        uint32_t w = kVocStoppedKey;
        if (i < n && J.f_weight[i] > 0.0) {
            w = J.f_word[i];
            ++live;
        }
        kw[i] = w;
        kf[i] = (uint16_t)i;
    }
    int m = 0;
    (void)block_exscan(live, s_wave, &m);  // m = features that are not stopped
    bitonic_sort(kw, kf, N);

    const int p0 = min(tid * per, m), p1 = min(p0 + per, m);
    int heads = 0;
    for (int p = p0; p < p1; ++p) heads += (p == 0 || kw[p - 1] != kw[p]) ? 1 : 0;
    int nw = 0;
    int idx = block_exscan(heads, s_wave, &nw);
    for (int p = p0; p < p1; ++p) {
        const uint32_t w = kw[p];
        if (p != 0 && kw[p - 1] == w) continue;
        double s = J.f_weight[kf[p]];  // v.addWeight(id, w): insert, then += in feature order
        for (int q = p + 1; q < m && kw[q] == w; ++q) s += J.f_weight[kf[q]];
        J.word_id[idx] = w;
        J.word_value[idx] = s;
        ++idx;
    }
    __syncthreads();  // the values are read back by other lanes of this workgroup

    // BowVector::normalize(L1): norm += fabs(value) in ascending word id, one ordered chain on wave 0
    // (64 values per coalesced load, then one add per value on the first lane's register)
    if (tid < 64) {
        double norm = 0.0;
        // the loads run two chunks ahead of the chain, which only ever waits for the adds
        double v = tid < nw ? fabs(J.word_value[tid]) : 0.0;
        double v1 = 64 + tid < nw ? fabs(J.word_value[64 + tid]) : 0.0;
        for (int base = 0; base < nw; base += 64) {
            const double v2 = base + 128 + tid < nw ? fabs(J.word_value[base + 128 + tid]) : 0.0;
            if (base + 64 <= nw) {  // a full chunk: 64 adds back to back, no test between them
#pragma unroll
                for (int j = 0; j < 64; ++j) norm += readlane_f64(v, j);
            } else {
#pragma unroll
                for (int j = 0; j < 64; ++j) {
                    const double vj = readlane_f64(v, j);
                    if (base + j < nw) norm += vj;
                }
            }
            v = v1;
            v1 = v2;
        }
        if (tid == 0) s_norm = norm;
    }
    __syncthreads();
    const double norm = s_norm;
    if (norm > 0.0)
        for (int i = tid; i < nw; i += kVocBuildThreads) J.word_value[i] = J.word_value[i] / norm;

    // ---- FeatureVector: sort (node id, feature) ----
    __syncthreads();
    for (int i = tid; i < N; i += kVocBuildThreads) {
        kw[i] = (i < n && J.f_weight[i] > 0.0) ? J.f_node[i] : kVocStoppedKey;
        kf[i] = (uint16_t)i;
    }
    bitonic_sort(kw, kf, N);
    heads = 0;
    for (int p = p0; p < p1; ++p) heads += (p == 0 || kw[p - 1] != kw[p]) ? 1 : 0;
    int nn = 0;
    idx = block_exscan(heads, s_wave, &nn);
    for (int p = p0; p < p1; ++p) {
        J.feat[p] = kf[p];
        if (p == 0 || kw[p - 1] != kw[p]) {
            J.node_id[idx] = kw[p];
            J.node_begin[idx] = p;
            ++idx;
        }
    }
    if (tid == 0) {
        J.node_begin[nn] = m;
        J.counts[0] = nw;
        J.counts[1] = nn;
        J.counts[2] = m;
        J.counts[3] = 0;
    }
}

__global__ __launch_bounds__(256) void voc_gather_kernel(VocGather G, uint32_t invalid_flag) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= G.n || e >= G.counts[2]) return;
    const uint32_t f = G.feat[e];
    G.desc_fv[2 * (size_t)e] = G.desc[2 * (size_t)f];
    G.desc_fv[2 * (size_t)e + 1] = G.desc[2 * (size_t)f + 1];
    if (G.valid && !G.valid[f]) G.feat[e] = f | invalid_flag;
}

}  // namespace

hipError_t launch_voc_transform(const DevVoc& voc, const VocJob* jobs, int count, int max_n, int nid_level, bool wide,
                                hipEvent_t* ev, hipStream_t st) {
    if (count <= 0) return hipSuccess;
    if (ev) (void)hipEventRecord(ev[0], st);
    if (max_n > 0) {
        const int per = kVocDescendThreads / (wide ? 32 : 16);
        const dim3 grid((unsigned)((max_n + per - 1) / per), (unsigned)count);
        const size_t lds = (size_t)voc.lds_nodes * kVocLdsNodeBytes;
        if (wide)
            hipLaunchKernelGGL(voc_descend_kernel<32>, grid, dim3(kVocDescendThreads), lds, st, voc, jobs, nid_level);
        else
            hipLaunchKernelGGL(voc_descend_kernel<16>, grid, dim3(kVocDescendThreads), lds, st, voc, jobs, nid_level);
    }
    if (ev) (void)hipEventRecord(ev[1], st);
    hipLaunchKernelGGL(voc_build_kernel, dim3((unsigned)count), dim3(kVocBuildThreads), 0, st, jobs);
    if (ev) (void)hipEventRecord(ev[2], st);
    return hipGetLastError();
}

hipError_t launch_voc_gather(const VocGather& g, uint32_t invalid_flag, hipStream_t st) {
    if (g.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(voc_gather_kernel, dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, st, g, invalid_flag);
    return hipGetLastError();
}

}  // namespace rsc
