// What the Hungarian matchers and the set criteria share (msda_matcher.hip, msda_criterion*.hip; bound and checked in
// msda_abi.hip): a launch's prediction sets, one step's targets, and the one place the match result buffer is laid out.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msda {

constexpr int kMatchMaxQueries = 1024;  // queries of a frame (one workgroup, one thread per query)
constexpr int kMatchMaxTargets = 16;    // targets of a frame (rows of the solved problem, held per thread)
constexpr int kMatchMaxSets = 16;       // prediction sets per launch (their pointers travel as kernel arguments)
constexpr int kMatchMaxDim = 64;        // keypoint values per target

// Per-set pointers, T = const float (predictions) or float (their gradients).  hand / obj: null without target keypoints;
// AssemblyHands has one keypoint head: its matcher passes it as both, its criterion as hand alone.
template <class T>
struct PredSets {
    T *logits[kMatchMaxSets];
    T *hand[kMatchMaxSets];
    T *obj[kMatchMaxSets];
};

// One step's targets, every frame's flattened: frame f owns rows [offsets[f], offsets[f + 1]).
struct SetTargets {
    const int64_t *labels;      // [n_targets]
    const float *tgt_kp;        // [n_targets, D] or NULL (D = 0)
    const int64_t *offsets;     // [bs + 1]
    long long n_targets;
    const int32_t *is_valid;    // slot k pairs with the k-th valid frame; NULL (AssemblyHands): with frame k
    int t_max;                  // targets of a frame at most: the width W of the match result's index rows
};

// The matcher's int64 result (include/msda.h): query_idx, target_idx [sets, bs, W], count, status [sets, bs], then the
// number of valid frames.  slot = set * bs + frame slot.
struct MatchView {
    long long slots;
    int W;
    __host__ __device__ MatchView(long long sets, int bs, int t_max) : slots(sets * bs), W(t_max) {}
    __host__ __device__ long long query(long long slot, int m) const { return slot * W + m; }
    __host__ __device__ long long target(long long slot, int m) const { return slots * W + slot * W + m; }
    __host__ __device__ long long count(long long slot) const { return 2 * slots * W + slot; }
    __host__ __device__ long long status(long long slot) const { return 2 * slots * W + slots + slot; }
    __host__ __device__ long long nvalid() const { return 2 * slots * W + 2 * slots; }
    __host__ __device__ long long numel() const { return nvalid() + 1; }
};

}  // namespace msda
