// The evaluation half of the training loop (examples/segmentation/train.py:716-832: validate, get_pred_whole,
// get_seg_metrics) on the device.  Every value the reference reports -- per-scan accuracy, mIoU and DSC and their jaw and
// whole means -- is a function of a few integer counts per scan, and these two entry points produce them:
//
//   geot_seg_confusion         from given predictions (the get_seg_metrics drop-in)
//   geot_seg_confusion_interp  from the soft-max of the N sampled points, three_nn's neighbours of every vertex and the
//                              vertex labels: get_pred_whole's weights, interpolation and arg-max per vertex in registers,
//                              counted at once -- no (C, M) probabilities and no per-vertex prediction are written
//
// Counting: one LDS histogram per wave, so the waves of a workgroup never contend.  Inside a wave, the lanes that share a
// bin -- most vertices land on the ~C diagonal bins, and neighbouring vertices on the same one -- are counted by a single
// LDS add of their number (up to SM_PEEL distinct bins per wave and pass; lanes left after that add 1 each).  The
// workgroup's histograms are summed and flushed with 64-bit integer atomics: the counts do not depend on the schedule.
// The translation unit is built with -ffp-contract=off, so the weight and interpolation expressions below round exactly
// as get_pred_whole's torch chain and gather_group.hip's three_interpolate_kernel round them.
#include "geot_common.h"
#include "geot_hip.h"
#include "seg_metrics.h"

namespace geot {

// get_pred_whole's prediction for one vertex (train.py:792-797):
//   dist_recip = 1.0 / (dist + 1e-8), dist = sqrt(dist2)   -- torch: (dist + 1e-8).reciprocal() * 1.0, correctly rounded
//   norm = torch.sum(dist_recip, dim=2)                      -- torch's reduction of a 3-long row runs on two lanes:
//                                                              (r0 + r2) + r1, not fp_weights_kernel's (r0 + r1) + r2
//   weight = dist_recip / norm
//   three_interpolate: P[i0] * w0 + P[i1] * w1 + P[i2] * w2, un-contracted (three_interpolate_kernel's expression)
//   argmax over the classes: the first maximum; a NaN counts as larger than everything (the first NaN wins)
__device__ __forceinline__ int sm_interp_argmax(const float *__restrict__ prob, int c, int n, const int *__restrict__ idx3,
                                                const float *__restrict__ d3)
{
    const int i0 = idx3[0], i1 = idx3[1], i2 = idx3[2];
    const float r0 = 1.0f / (sqrtf(d3[0]) + 1e-8f), r1 = 1.0f / (sqrtf(d3[1]) + 1e-8f), r2 = 1.0f / (sqrtf(d3[2]) + 1e-8f);
    const float norm = (r0 + r2) + r1;
    const float w0 = r0 / norm, w1 = r1 / norm, w2 = r2 / norm;
    float best = prob[i0] * w0 + prob[i1] * w1 + prob[i2] * w2;
    int arg = 0;
    for (int l = 1; l < c; ++l) {
        const float *P = prob + (size_t)l * n;
        const float v = P[i0] * w0 + P[i1] * w1 + P[i2] * w2;
        if (best == best && (v != v || v > best)) {
            best = v;
            arg = l;
        }
    }
    return arg;
}

template <bool INTERP>
__global__ __launch_bounds__(SM_THREADS) void seg_confusion_kernel(int b, int c, int n, const long long *__restrict__ offsets,
                                                                   const long long *__restrict__ pred,
                                                                   const float *__restrict__ prob, const int *__restrict__ idx,
                                                                   const float *__restrict__ dist2,
                                                                   const long long *__restrict__ label,
                                                                   unsigned long long *__restrict__ counts)
{
    __shared__ unsigned h[SM_WAVES * SM_MAX_SLOTS];
    const int slots = c * (c + 1) + 1;
    unsigned *hw = h + (threadIdx.x / GEOT_WAVE) * slots;
    for (int s = blockIdx.y; s < b; s += gridDim.y) {
        for (int i = threadIdx.x; i < SM_WAVES * slots; i += SM_THREADS) h[i] = 0;
        __syncthreads();
        const long long lo = offsets[s], hi = offsets[s + 1];
        // `base` is uniform over the workgroup: every lane of a wave reaches sm_count's ballots together
        for (long long base = lo + (long long)blockIdx.x * SM_THREADS; base < hi; base += (long long)gridDim.x * SM_THREADS) {
            const long long v = base + threadIdx.x;
            const bool active = v < hi;
            int key = 0;
            if (active) {
                long long p;
                if constexpr (INTERP)
                    p = sm_interp_argmax(prob + (size_t)s * c * n, c, n, idx + 3 * v, dist2 + 3 * v);
                else
                    p = pred[v];
                key = sm_slot(label[v], p, c);
            }
            sm_count(hw, key, active);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < slots; i += SM_THREADS) {
            unsigned t = 0;
#pragma unroll
            for (int w = 0; w < SM_WAVES; ++w) t += h[w * slots + i];
            if (t) atomicAdd(&counts[(size_t)s * slots + i], (unsigned long long)t);
        }
        __syncthreads();        // every histogram is read before the next scan clears them
    }
}

static hipError_t seg_confusion_launch(int b, int c, int n, const long long *offsets, const long long *pred, const float *prob,
                                       const int *idx, const float *dist2, const long long *label, long long *counts,
                                       hipStream_t s)
{
    const int gy = b < 65535 ? b : 65535;
    const dim3 grid((SM_GROUPS + gy - 1) / gy, gy);
    unsigned long long *out = reinterpret_cast<unsigned long long *>(counts);
    if (prob)
        hipLaunchKernelGGL((seg_confusion_kernel<true>), grid, dim3(SM_THREADS), 0, s, b, c, n, offsets, nullptr, prob, idx, dist2,
                           label, out);
    else
        hipLaunchKernelGGL((seg_confusion_kernel<false>), grid, dim3(SM_THREADS), 0, s, b, c, 0, offsets, pred, nullptr, nullptr,
                           nullptr, label, out);
    return hipGetLastError();
}

} // namespace geot

using namespace geot;

GEOT_EXPORT int geot_seg_confusion(int b, int c, const long long *offsets, const long long *pred, const long long *label,
                                   long long *counts, void *stream)
{
    if (b < 0 || c < 1 || c > GEOT_NTM_MAX_C) return hipErrorInvalidValue;
    if (b == 0) return hipSuccess;
    if (!offsets || !pred || !label || !counts) return hipErrorInvalidValue;
    return seg_confusion_launch(b, c, 0, offsets, pred, nullptr, nullptr, nullptr, label, counts, (hipStream_t)stream);
}

GEOT_EXPORT int geot_seg_confusion_interp(int b, int c, int n, const long long *offsets, const float *prob, const int *idx,
                                          const float *dist2, const long long *label, long long *counts, void *stream)
{
    if (b < 0 || c < 1 || c > GEOT_NTM_MAX_C || n < 0) return hipErrorInvalidValue;
    if (b == 0) return hipSuccess;
    if (n == 0 || !offsets || !prob || !idx || !dist2 || !label || !counts) return hipErrorInvalidValue;
    return seg_confusion_launch(b, c, n, offsets, nullptr, prob, idx, dist2, label, counts, (hipStream_t)stream);
}
