// seg_metrics.h -- the confusion-count slot of one vertex and the per-wave LDS histogram of seg_metrics.hip, shared with
// scan_predict.hip.
#pragma once
#include "geot_common.h"
#include "geot_hip.h"

namespace geot {

constexpr int SM_THREADS = 256;
constexpr int SM_WAVES = SM_THREADS / GEOT_WAVE;
constexpr int SM_MAX_SLOTS = GEOT_NTM_MAX_C * (GEOT_NTM_MAX_C + 1) + 1;
constexpr int SM_PEEL = 4;
constexpr int SM_GROUPS = 512;           // workgroups per launch (2 per CU), shared out over the scans

// slot of one vertex: row = label, column = prediction (column c = outside [0, c)); a label outside [0, c) -> the last slot
__device__ __forceinline__ int sm_slot(long long label, long long pred, int c)
{
    if (label < 0 || label >= c) return c * (c + 1);
    return (int)label * (c + 1) + (pred >= 0 && pred < c ? (int)pred : c);
}

// Adds 1 to h[key] for every active lane.  Called by every lane of the wave (the ballots need all of them).
__device__ __forceinline__ void sm_count(unsigned *h, int key, bool active)
{
    const int lane = threadIdx.x & (GEOT_WAVE - 1);
    bool pending = active;
    for (int k = 0; k < SM_PEEL; ++k) {
        const unsigned long long left = __ballot(pending);
        if (left == 0) return;
        const int leader = __ffsll(left) - 1;
        const int lkey = __builtin_amdgcn_readlane(key, leader);
        const bool same = pending && key == lkey;
        const unsigned long long group = __ballot(same);
        if (lane == leader) atomicAdd(&h[lkey], (unsigned)__popcll(group));
        pending = pending && !same;
    }
    if (pending) atomicAdd(&h[key], 1u);
}

} // namespace geot
