// What geot_fixmatch_views (views.hip) and geot_view_program (view_program.hip) share: the assignment of points to threads,
// the NaN-propagating extrema, the element accessors and the workgroup reduction trees.  Both kernels reduce with exactly
// these statements, in this order -- that is what makes a transform list compiled to a view program carry the bits of the
// hard-wired kernel.
#ifndef GEOT_VIEWS_H
#define GEOT_VIEWS_H
#include <hip/hip_runtime.h>

#include "geot_common.h"
#include "geot_hip.h"

namespace geot {

constexpr int VIEW_THREADS = 512, VIEW_WAVES = VIEW_THREADS / GEOT_WAVE, VIEW_PPT = GEOT_VIEW_REG_POINTS / VIEW_THREADS;
constexpr int VIEW_CHUNK = 4;       // rounds per step of the streaming path

__device__ __forceinline__ float nan_min(float a, float b) { return (a != a) ? a : ((b < a || b != b) ? b : a); }
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a) ? a : ((b > a || b != b) ? b : a); }

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);     // butterfly: every lane ends with the same bits
    return v;
}
template <bool IS_MAX>
__device__ __forceinline__ float wave_ext_nan(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float o = __shfl_xor(v, d);
        v = IS_MAX ? nan_max(v, o) : nan_min(v, o);
    }
    return v;
}

// element at a 32-bit BYTE offset from a workgroup-uniform base: one address register per access instead of a 64-bit pair
// (the entry points admit only clouds whose rows stay below 4 GB)
__device__ __forceinline__ float view_ld(const float *base, unsigned bytes) { return *(const float *)((const char *)base + bytes); }
__device__ __forceinline__ void view_st(float *base, unsigned bytes, float v) { *(float *)((char *)base + bytes) = v; }

struct ViewRed {
    double sum[3];
    float mn, mx;
};

// the workgroup's column sums and minimum out of every thread's partials: a butterfly over the wave, the wave results added
// in wave order by every thread.  red_sum / red_min: __shared__, not in use by any other reduction still being read.
__device__ __forceinline__ void view_reduce_sum_min(ViewRed &r, double (&red_sum)[VIEW_WAVES][3], float (&red_min)[VIEW_WAVES],
                                                    int wave, double (&tot)[3], float &low)
{
#pragma unroll
    for (int a = 0; a < 3; ++a) r.sum[a] = wave_sum_f64(r.sum[a]);
    r.mn = wave_ext_nan<false>(r.mn);
    if (lane_id() == 0) {
        red_sum[wave][0] = r.sum[0];
        red_sum[wave][1] = r.sum[1];
        red_sum[wave][2] = r.sum[2];
        red_min[wave] = r.mn;
    }
    __syncthreads();
    tot[0] = tot[1] = tot[2] = 0;
    low = red_min[0];
#pragma unroll
    for (int w = 0; w < VIEW_WAVES; ++w) {
        tot[0] += red_sum[w][0];
        tot[1] += red_sum[w][1];
        tot[2] += red_sum[w][2];
        low = nan_min(low, red_min[w]);
    }
}

// the workgroup's maximum (IS_MAX) or minimum of every thread's partial v
template <bool IS_MAX>
__device__ __forceinline__ float view_reduce_ext(float v, float (&red)[VIEW_WAVES], int wave)
{
    v = wave_ext_nan<IS_MAX>(v);
    if (lane_id() == 0) red[wave] = v;
    __syncthreads();
    float top = red[0];
#pragma unroll
    for (int w = 1; w < VIEW_WAVES; ++w) top = IS_MAX ? nan_max(top, red[w]) : nan_min(top, red[w]);
    return top;
}

} // namespace geot
#endif
