// rsc_projrounds.h — the device side of rsc_projcore.h: the window walk by a subgroup of lanes and the rounds
// loop of the four matcher kernels (frameproj.hip, kfproj.hip, localproj.hip, lastproj.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "rsc_projcore.h"

namespace rsc {

constexpr int kProjSub = 16;          // lanes that walk one window together
// LDS list of the points that walk their window this round (16 KB).  A point whose slot lands at or past the cap
// walks alone inside the pick loop (best() instead of best_coop()): the same decision, so the same fixed point.
// Reached only when more than kProjWalkCap points of one problem have used up their cache in one round, e.g.
// 4,200 identical points over 12 features within 1 px of their projection at distances 3 + 5 k: 4,197 walkers in
// each of the last three of 6 rounds (tests/walk_list_cases.py, which reads the cap from this line; the cases at
// cap, cap + 1 and cap + 101 run in tests/test_gpu_walk_list.py).
constexpr int kProjWalkCap = 4096;
constexpr unsigned long long kProjNoKey = ~0ull;

// proj_walk by kSub lanes, as a fold.  For one column ix the cells iy0..iy1 are contiguous in the CSR (cell =
// ix * 48 + iy) and in visiting order, so the lanes stride over each column's entries and s = visit(s, f, rank)
// gets every feature with its rank in the sequential visit.  The state goes through by value: a visitor that
// updated captured locals behind an if / else kept them in the private segment.
template <int kSub, class State, class Visit>
__device__ __forceinline__ State proj_walk_coop(const DevProjFrame& F, const ProjCells& w, int lane, State s,
                                                Visit visit) {
    const int32_t* cell_begin = F.cell_begin;
    const int32_t* cell_feat = F.cell_feat;
    int rank0 = 0;
    for (int ix = w.x0; ix <= w.x1; ++ix) {
        const int b = cell_begin[ix * kProjGridRows + w.y0], e1 = cell_begin[ix * kProjGridRows + w.y1 + 1];
        for (int e = b + lane; e < e1; e += kSub) s = visit(s, cell_feat[e], rank0 + (e - b));
        rank0 += e1 - b;
    }
    return s;
}

// (distance, rank, feature): distinct per candidate, and ascending as the sequential walk's strict < prefers.
// rank and f are below kProjMaxFeatures, so the two share the low word.
__device__ __forceinline__ unsigned long long proj_coop_key(int dist, int rank, int f) {
    return (unsigned long long)dist << 32 | ((unsigned)rank << 16 | (unsigned)f);
}

// the smallest key of the subgroup, in every lane of it
template <int kSub>
__device__ __forceinline__ unsigned long long proj_min_coop(unsigned long long key) {
#pragma unroll
    for (int s = kSub / 2; s; s >>= 1) {
        const unsigned long long o = __shfl_xor(key, s, kSub);
        key = o < key ? o : key;
    }
    return key;
}

// proj_first_min by kSub lanes: the smallest (distance, rank) key of the subgroup is the first strict minimum
// of the sequential walk.  Every lane of the subgroup returns the decision; lanes with cells < 0 only take
// part in the shuffles.
template <int kSub, class Gate>
__device__ __forceinline__ int proj_first_min_coop(const DevProjFrame& F, int cells, const ProjDesc dMP, int i,
                                                   const int* owner, const Gate& gate, int cutoff, int lane) {
    const ProjDesc* desc = F.desc;
    unsigned long long best = kProjNoKey;
    if (cells >= 0)
        best = proj_walk_coop<kSub>(F, ProjCells(cells), lane, best, [&](unsigned long long k, int f, int rank) {
            if (!gate(f) || owner[f] < i) return k;
            const unsigned long long key = proj_coop_key(proj_desc_dist(dMP, desc[f]), rank, f);
            return key < k ? key : k;
        });
    best = proj_min_coop<kSub>(best);
    if (best == kProjNoKey) return -1;
    return (int)(best >> 32) <= cutoff ? (int)(best & 0xffff) : -1;
}

// proj_first_min_coop for a matcher without claims (every feature free, KfpAllFree: the KeyFrame Fuse of
// rsc_fusekf.h): the gate alone decides what takes part
template <int kSub, class Gate>
__device__ __forceinline__ int proj_first_min_free_coop(const DevProjFrame& F, int cells, const ProjDesc dMP,
                                                        const Gate& gate, int cutoff, int lane) {
    const ProjDesc* desc = F.desc;
    unsigned long long best = kProjNoKey;
    if (cells >= 0)
        best = proj_walk_coop<kSub>(F, ProjCells(cells), lane, best, [&](unsigned long long k, int f, int rank) {
            if (!gate(f)) return k;
            const unsigned long long key = proj_coop_key(proj_desc_dist(dMP, desc[f]), rank, f);
            return key < k ? key : k;
        });
    best = proj_min_coop<kSub>(best);
    if (best == kProjNoKey) return -1;
    return (int)(best >> 32) <= cutoff ? (int)(best & 0xffff) : -1;
}

// The rounds of one workgroup of kThreads lanes (the loop and its bound: rsc_projcore.h).  owner: the LDS
// table over the n_features features; claim: A, -1 on entry; n_eligible: the points with a window.  M is the
// matcher:
//   n_points()          points of the problem
//   entry_occupied(f)   feature f carries kProjOccupied
//   blocks(i)           a claim of point i enters the owner table
//   pick(i, owner)      point i's choice from its cache: the feature, -1 none, -2 walk the window, kProjSkip
//   best(i, owner)      the same decision by walking the window alone
//   kCoopWalk           the points that walk are listed in `walk` (kProjWalkCap ints of LDS) and their windows
//                       walked by kProjSub lanes each: best_coop(i, valid, owner, lane), which every lane of
//                       the subgroup calls; the same decision in all of them.  A full list: best().
// Returns the rounds run; afterwards claim is the fixed point and owner the table of its blocking claims.
template <int kThreads, class M>
__device__ __forceinline__ int proj_rounds(const M m, int* owner, int n_features, int32_t* claim, int n_eligible,
                                           int* walk) {
    __shared__ int changed, n_walk;
    const int tid = threadIdx.x, n = m.n_points();
    const int max_rounds = n_eligible + 1;
    int rounds = 0;
    for (int r = 0; r < max_rounds; ++r) {
        for (int f = tid; f < n_features; f += kThreads) owner[f] = m.entry_occupied(f) ? kProjOccupied : kProjFree;
        if (tid == 0) {
            changed = 0;
            if constexpr (M::kCoopWalk) n_walk = 0;
        }
        __syncthreads();
        for (int i = tid; i < n; i += kThreads) {
            const int a = claim[i];
            if (a >= 0 && m.blocks(i)) atomicMin(&owner[a], i);
        }
        __syncthreads();
        int any = 0;
        for (int i = tid; i < n; i += kThreads) {
            int b = m.pick(i, owner);
            if (b == kProjSkip) continue;
            if (b == -2) {  // the cache is used up and the list was longer: walk the window
                if constexpr (M::kCoopWalk) {
                    const int slot = atomicAdd(&n_walk, 1);
                    if (slot < kProjWalkCap) {
                        walk[slot] = i;
                        continue;
                    }
                }
                b = m.best(i, owner);
            }
            if (b != claim[i]) {
                claim[i] = b;
                any = 1;
            }
        }
        if constexpr (M::kCoopWalk) {
            __syncthreads();
            const int nw = n_walk < kProjWalkCap ? n_walk : kProjWalkCap;
            const int sub = tid / kProjSub, lane = tid % kProjSub;
            for (int base = 0; base < nw; base += kThreads / kProjSub) {  // one trip count for all: shuffles inside
                const int w = base + sub;
                const bool valid = w < nw;
                const int i = valid ? walk[w] : 0;
                const int b = m.best_coop(i, valid, owner, lane);
                if (valid && lane == 0 && b != claim[i]) {
                    claim[i] = b;
                    any = 1;
                }
            }
        }
        if (any) changed = 1;
        ++rounds;
        __syncthreads();
        const int go = changed;
        __syncthreads();
        if (!go) break;
    }
    return rounds;
}

// the points with a window, summed into *n_eligible (LDS, zeroed and followed by a barrier by the caller)
template <int kThreads, class Rec>
__device__ __forceinline__ void proj_count_eligible(const Rec* rec, int n, int* n_eligible) {
    int mine = 0;
    for (int i = threadIdx.x; i < n; i += kThreads) mine += rec[i].cells >= 0;
    if (mine) atomicAdd(n_eligible, mine);
}

}  // namespace rsc
