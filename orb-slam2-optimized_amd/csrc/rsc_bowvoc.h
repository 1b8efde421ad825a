// rsc_bowvoc.h — DBoW2 TemplatedVocabulary::transform(features, BowVector, FeatureVector, levelsup)
// (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1194, :1218-1259; Frame::ComputeBoW /
// KeyFrame::ComputeBoW) on the GPU: device layout shared by the kernels (bowvoc.hip) and the host.
//
// The vocabulary is resident in HBM in breadth-first ("dense") order: the children of a node are one
// contiguous run in child order, and the top levels of the tree are a prefix of every array, so the
// first `lds_nodes` nodes can be staged in LDS by each descent workgroup.
//
// Two kernels per call:
//   voc_descend_kernel<SG> — a subgroup of SG lanes (16, or 32 when a node has more than 16
//       children) per feature, one child per lane: 8 XOR + popcount on the child's 32 bytes, then a
//       min-reduction of (distance << 8 | child index) over the subgroup — exactly "smallest distance,
//       first child on ties" (the strict < of :1244).  Nodes below the cut come from LDS, the others
//       are gathered (one contiguous run of children per subgroup).  Per feature it leaves the word
//       id, the node id at nid_level and the leaf weight (<= 0 or NaN: stopped, :1157).
//   voc_build_kernel — one workgroup per view: bitonic sort of (word id, feature) in LDS, the word
//       values as sequential adds in feature order by the lane at the head of each run
//       (BowVector::addWeight), the L1 norm as one ordered FP64 chain over the words in ascending id
//       (BowVector::normalize), IEEE divisions; then the same sort on (node id, feature) gives the
//       FeatureVector as CSR.  Sort steps whose pair distance is <= 64 stay inside one wave (no
//       workgroup barrier); the chain takes its operands with v_readlane_b32 from values loaded two
//       chunks ahead (DESIGN.md §9 has the measurements behind both).
// Integer popcount and a short FP64 chain: no MFMA.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace rsc {

constexpr int kVocMaxFeatures = 8192;        // features per view (= kBowMaxFeatures)
constexpr int kVocMaxChildren = 32;          // children per node (one lane each in a 32-lane subgroup)
constexpr int kVocDescendThreads = 512;      // 32 (SG = 16) or 16 (SG = 32) features per workgroup
constexpr int kVocBuildThreads = 1024;       // one workgroup per view
constexpr int kVocLdsNodeBytes = 40;         // staged node: 32 B descriptor + (child_begin, n_children)
constexpr int kVocLdsBudgetDefault = 48 * 1024;  // ORBvoc levels 0-3: 1111 nodes = 44440 B
constexpr int kVocLdsBudgetMax = 48 * 1024;
constexpr uint32_t kVocStoppedKey = 0xFFFFFFFFu;  // sort key of a stopped feature / of the padding

// The resident vocabulary (dense = breadth-first index; node 0 is the root).
struct DevVoc {
    const uint4* desc;       // [n_nodes][2] descriptors
    const uint2* rec;        // [n_nodes] (dense index of the first child, number of children)
    const uint32_t* orig;    // [n_nodes] node id in the caller's numbering (the FeatureVector key)
    const uint32_t* word;    // [n_nodes] word id (0 for a node that is not a word)
    const double* weight;    // [n_nodes]
    int n_nodes;
    int lds_nodes;           // nodes [0, lds_nodes) are staged in LDS (whole levels)
    int max_depth;           // deepest leaf: bound of the descent loop
};

// One view of a call.
struct VocJob {
    const uint4* desc;       // [n][2]
    int n;
    uint32_t* f_word;        // [n] per-feature word id          (descent -> build)
    uint32_t* f_node;        // [n] per-feature node id at nid_level
    double* f_weight;        // [n] per-feature leaf weight
    uint32_t* word_id;       // [n] BowVector ids ascending
    double* word_value;      // [n]
    uint32_t* node_id;       // [n] FeatureVector keys ascending
    int32_t* node_begin;     // [n + 1]
    uint32_t* feat;          // [n]
    int32_t* counts;         // [4] n_words, n_nodes, features not stopped, 0
};

// rsc_bow_create_transformed: desc_fv[e] = desc[feat[e]] and the validity flag on feat[e]
struct VocGather {
    const uint4* desc;
    uint4* desc_fv;
    uint32_t* feat;
    const uint8_t* valid;    // may be null
    const int32_t* counts;   // counts[2] = entries
    int n;
};

// nid_level = L - levelsup (<= 0: every node id is 0); wide: 32-lane subgroups; ev (may be null):
// three events recorded before the descent, between the kernels and after the build
hipError_t launch_voc_transform(const DevVoc& voc, const VocJob* jobs, int count, int max_n, int nid_level, bool wide,
                                hipEvent_t* ev, hipStream_t st);
hipError_t launch_voc_gather(const VocGather& g, uint32_t invalid_flag, hipStream_t st);

}  // namespace rsc
