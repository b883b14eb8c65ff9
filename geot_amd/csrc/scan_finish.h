// scan_finish.h -- what the whole-scan kernels that keep a vertex-major accumulator share (scan_predict.hip's tile form of
// geot_scan_vote, scan_cover.hip): the arg-max rule over one row of sums and the ordering of a wave's own LDS traffic; and the
// same rule over one column of channel-first logits (scan_decode.hip).
#pragma once
#include "geot_common.h"

namespace geot {

// torch.argmax's rule over one row of c values, serially in one lane: the first NaN if there is one, else the first maximum
__device__ __forceinline__ int sp_argmax_row(const float *row, int c)
{
    float best = row[0];
    int at = 0;
    bool nan = best != best;
    for (int k = 1; k < c; ++k) {
        const float x = row[k];
        if (!nan && (x != x || x > best)) { best = x; at = k; nan = x != x; }
    }
    return at;
}

// the same rule over one column of a channel-first table: value k at col[k * stride] (scan_decode.hip's logits)
__device__ __forceinline__ int sp_argmax_strided(const float *col, size_t stride, int c)
{
    float best = col[0];
    int at = 0;
    bool nan = best != best;
    for (int k = 1; k < c; ++k) {
        const float x = col[(size_t)k * stride];
        if (!nan && (x != x || x > best)) { best = x; at = k; nan = x != x; }
    }
    return at;
}

// Between a wave's LDS writes and its other lanes' reads of them: the hardware keeps one wave's LDS accesses in order, this
// keeps the compiler from moving them across.
__device__ __forceinline__ void sp_wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

} // namespace geot
