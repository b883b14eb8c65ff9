// FixMatch pseudo-label masks refined by the nearest neighbours' probabilities (geot_pseudo_refine): utils/pseudo_mask.py's
// pseudo_label_refine / _margin / _margin_v1 behind their neighbour search, for all points of a batch in one launch -- no
// workspace, no atomics, no host synchronisation.  See include/geot_hip.h for the rules.
//
// A workgroup takes 64 consecutive points of one cloud.  Per point and class: the point's own probability (coalesced: the
// layout is channel-first), the n neighbours' probabilities of that class (n scattered 4-byte reads of a (B, C, N) array that
// lives in L2 at the step's sizes), the k largest kept in a descending list by compare-exchange in registers (every index
// static: no scratch), the reference's update once per kept value, and the running top two over the classes.
// Two forms of sharing the classes out (GEOT_PSEUDO_REFINE_IMPL=point|split, read at every call; the same bits;
// profiles/pseudo_refine_timing.txt):
//   point  one wave per workgroup, a lane per point walks all C classes;
//   split  four waves per workgroup, wave g walks the classes g, g + 4, ... of the same 64 points, and wave 0 merges the four
//          top-two pairs through LDS: four times the waves and the loads in flight at sizes (32 000 - 48 000 points) that
//          give the point form two or three waves per CU.
#include "geot_common.h"
#include "geot_hip.h"

namespace geot {

constexpr int PR_POINTS = 64;
constexpr int PR_SPLIT = 4;

// torch.topk's and torch.max's order: a NaN ranks above every number
__device__ __forceinline__ bool pr_above(float a, float b) { return a > b || (a != a && b == b); }

__device__ __forceinline__ void pr_top2(float p, float &t1, float &t2)
{
    const bool first = pr_above(p, t1), second = pr_above(p, t2);      // selects, not branches: t1 / t2 stay in registers
    t2 = first ? t1 : (second ? p : t2);
    t1 = first ? p : t1;
}

// KM: the length of the kept list (k <= KM), NM: the neighbour ids held in registers (n <= NM), SPLIT: waves per workgroup
template <int KM, int NM, int SPLIT>
__global__ __launch_bounds__(PR_POINTS *SPLIT) void pseudo_refine_kernel(int c, int npts, int n, int k, int mode, float th,
                                                                         float beta, const float *__restrict__ prob,
                                                                         const int *__restrict__ nbr,
                                                                         const float *__restrict__ e_joint,
                                                                         unsigned char *__restrict__ keep,
                                                                         float *__restrict__ value)
{
    __shared__ float part[SPLIT > 1 ? 2 * (SPLIT - 1) * PR_POINTS : 1];
    const int lane = threadIdx.x % PR_POINTS, g = threadIdx.x / PR_POINTS;
    const int b = blockIdx.y;
    const int i = blockIdx.x * PR_POINTS + lane;
    const bool live = i < npts;
    const float lowest = -__builtin_inff();
    float t1 = lowest, t2 = lowest;
    bool bad = false;
    if (live) {
        const size_t point = (size_t)b * npts + i;
        const int *__restrict__ row = nbr + point * n;
        int id[NM];
#pragma unroll
        for (int j = 0; j < NM; ++j) {
            id[j] = i;
            if (j < n) {
                const int v = row[j];
                if ((unsigned)v < (unsigned)npts)
                    id[j] = v;
                else
                    bad = true;          // never followed: the point's own index stands in, the point is dropped below
            }
        }
        for (int cls = g; cls < c; cls += SPLIT) {
            const float *__restrict__ pc = prob + ((size_t)b * c + cls) * npts;
            float p = pc[i];
            float top[KM];
#pragma unroll
            for (int j = 0; j < KM; ++j) top[j] = lowest;
#pragma unroll
            for (int j = 0; j < NM; ++j) {
                if (j < n) {
                    float v = pc[id[j]];
#pragma unroll
                    for (int s = 0; s < KM; ++s) {          // descending: v sinks to its place, equal values stay both
                        const bool up = pr_above(v, top[s]);
                        const float hi = up ? v : top[s], lo = up ? top[s] : v;
                        top[s] = hi;
                        v = lo;
                    }
                }
            }
            if (mode == GEOT_PSEUDO_MARGIN_V1) {
                const float e = e_joint[cls];
#pragma unroll
                for (int s = 0; s < KM; ++s) {
                    if (s < k) {
                        const float v = top[s];
                        const float ub = (e * p) / v;
                        p = (p + v) - (p * ub);
                    }
                }
            } else {
#pragma unroll
                for (int s = 0; s < KM; ++s) {
                    if (s < k) {
                        const float v = top[s];
                        p = (p + beta * v) - ((p * v) * beta);
                    }
                }
            }
            pr_top2(p, t1, t2);
        }
    }
    if (SPLIT > 1) {
        if (g > 0) {
            part[(2 * (g - 1)) * PR_POINTS + lane] = t1;
            part[(2 * (g - 1) + 1) * PR_POINTS + lane] = t2;
        }
        __syncthreads();
        if (g > 0) return;
#pragma unroll
        for (int w = 0; w < 2 * (SPLIT - 1); ++w) pr_top2(part[w * PR_POINTS + lane], t1, t2);
    }
    if (!live) return;
    float val = mode == GEOT_PSEUDO_MAX ? t1 : t1 - t2;
    if (bad) val = __builtin_nanf("");
    const size_t point = (size_t)b * npts + i;
    keep[point] = val >= th ? 1 : 0;
    if (value) value[point] = val;
}

template <int SPLIT>
static void pr_launch(int b, int c, int npts, int n, int k, int mode, float th, float beta, const float *prob, const int *nbr,
                      const float *e_joint, unsigned char *keep, float *value, hipStream_t s)
{
    const dim3 grid((npts + PR_POINTS - 1) / PR_POINTS, b), block(PR_POINTS * SPLIT);
#define PR_GO(KM, NM)                                                                                                           \
    hipLaunchKernelGGL((pseudo_refine_kernel<KM, NM, SPLIT>), grid, block, 0, s, c, npts, n, k, mode, th, beta, prob, nbr, e_joint, \
                       keep, value)
    if (n <= 4) {
        if (k == 1)
            PR_GO(1, 4);
        else
            PR_GO(4, 4);
    } else if (k == 1) {
        PR_GO(1, 32);
    } else if (k <= 4) {
        PR_GO(4, 32);
    } else {
        PR_GO(32, 32);
    }
#undef PR_GO
}

} // namespace geot

using namespace geot;

GEOT_EXPORT int geot_pseudo_refine(int b, int c, int npts, int n, int k, int mode, float th, float beta, const float *prob,
                                   const int *nbr, const float *e_joint, unsigned char *keep, float *value, void *stream)
{
    if (b < 1 || b > 65535 || c < 1 || c > GEOT_NTM_MAX_C || n < 1 || n > GEOT_PSEUDO_REFINE_MAX_N || k < 1 || k > n)
        return hipErrorInvalidValue;
    if (npts < n + 1 || mode < GEOT_PSEUDO_MAX || mode > GEOT_PSEUDO_MARGIN_V1) return hipErrorInvalidValue;
    if (mode != GEOT_PSEUDO_MAX && c < 2) return hipErrorInvalidValue;
    if (!prob || !nbr || !keep || (mode == GEOT_PSEUDO_MARGIN_V1 && !e_joint)) return hipErrorInvalidValue;
    const char *e = getenv("GEOT_PSEUDO_REFINE_IMPL");      // read at every call; the default is the form that measured faster
    hipStream_t s = (hipStream_t)stream;
    if (e && e[0] == 'p')
        pr_launch<1>(b, c, npts, n, k, mode, th, beta, prob, nbr, e_joint, keep, value, s);
    else
        pr_launch<PR_SPLIT>(b, c, npts, n, k, mode, th, beta, prob, nbr, e_joint, keep, value, s);
    return hipGetLastError();
}
