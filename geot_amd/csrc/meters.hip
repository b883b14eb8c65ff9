// The epoch statistics of the FixMatch+NTM loop (examples/segmentation/train.py:599-644 per iteration, :672-699 into the
// meters, :701-715 read out) on the device: two launches per iteration and no host synchronisation, so a replayed
// iteration (geot_amd/graph_step.py) can carry them.  The reference pays ~3 C + 10 host round trips per iteration
// (`.item()`, `if denominator == 0`).
//
//   geot_fixmatch_meters_count     integer counts over the B_u * N unlabelled points (LDS histograms, integer atomics:
//                                  deterministic whatever the schedule)
//   geot_fixmatch_meters_finalize  one workgroup: the iteration's values from the counts, with the reference's arithmetic,
//                                  accumulated into persistent AverageMeter states; zeroes the counts for the next iteration
//
// Arithmetic (the translation unit is built with -ffp-contract=off; the _rn intrinsics make every rounding explicit):
//   fp32-tensor meters   value = fp32 arithmetic on the exact counts (below 2^24 points the reference's fp32 sums of 0/1
//                        are exact); meter sum += fp32(value * n), avg = sum / count as torch forms a CUDA tensor divided by
//                        a Python int (see fdiv_by_int)
//   Python-float meters  per-class value = double(fp32 ratio) * 100 in double; loss value = double(fp32 loss);
//                        meter sum += value * n, avg = sum / count, in double
#include "geot_common.h"
#include "geot_hip.h"

namespace geot {

constexpr int FM_THREADS = 256;
constexpr int FM_FIN_THREADS = 64;
// counter layout (ints): see include/geot_hip.h
constexpr int FM_M = 0, FM_TG = 1, FM_SG = 2, FM_MTG = 3, FM_FG = 4, FM_FG_M = 5, FM_FG_MTG = 6, FM_BAD = 7, FM_CLS = 8;
// fp32 meters, in this order: th_percentage, mean_pseudo_label_acc, teacher_acc, student_acc, over_th_wobg, over_acc_wobg
constexpr int FM_F32 = 6;
// double scalar meters: loss, loss_l, loss_u, feat, identity, 3d
constexpr int FM_LOSS = 6;

// torch: a CUDA tensor divided by a Python number is multiplied by the fp32 reciprocal of that number
// (the div_true kernel's CPU-scalar path); a tensor divided by a tensor is a correctly rounded fp32 division
__device__ __forceinline__ float fdiv_by_int(float a, long long d) { return __fmul_rn(a, __fdiv_rn(1.0f, (float)d)); }

__global__ __launch_bounds__(FM_THREADS) void fm_count_kernel(int b, int n, int c, float threshold,
                                                              const long long *__restrict__ pseudo,
                                                              const float *__restrict__ conf,
                                                              const long long *__restrict__ gt,
                                                              const float *__restrict__ prob, int *__restrict__ counts)
{
    __shared__ int h[FM_CLS + 4 * GEOT_NTM_MAX_C];
    const int bins = FM_CLS + 4 * c;
    for (int i = threadIdx.x; i < bins; i += blockDim.x) h[i] = 0;
    __syncthreads();
    int acc[FM_CLS] = {0, 0, 0, 0, 0, 0, 0, 0};
    const long long total = (long long)b * n;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long long)gridDim.x * blockDim.x) {
        const long long bi = p / n, i = p - bi * n;
        const long long t = pseudo[p], g = gt[p];
        const bool m = conf[p] >= threshold;            // NaN confidence: not confident (torch.ge)
        // the student's label: torch.max over C -- the first maximum, a NaN counted as larger than everything
        const float *col = prob + bi * c * n + i;
        float best = col[0];
        int s = 0;
        for (int cc = 1; cc < c; ++cc) {
            const float v = col[(long long)cc * n];
            if (best == best && (v != v || v > best)) {
                best = v;
                s = cc;
            }
        }
        const bool tg = t == g, fg = t > 0;
        acc[FM_M] += m;
        acc[FM_TG] += tg;
        acc[FM_SG] += (long long)s == g;
        acc[FM_MTG] += m && tg;
        acc[FM_FG] += fg;
        acc[FM_FG_M] += fg && m;
        acc[FM_FG_MTG] += fg && m && tg;
        const bool t_in = t >= 0 && t < c, g_in = g >= 0 && g < c;
        acc[FM_BAD] += !t_in + !g_in;
        if (t_in) {
            atomicAdd(&h[FM_CLS + 2 * c + t], 1);                 // [t = c]
            if (m) {
                atomicAdd(&h[FM_CLS + t], 1);                     // m [t = c]
                if (tg) atomicAdd(&h[FM_CLS + c + t], 1);         // m [t = c][g = c]
            }
        }
        if (g_in) atomicAdd(&h[FM_CLS + 3 * c + g], 1);           // [g = c]
    }
    for (int k = 0; k < FM_CLS; ++k)
        if (acc[k]) atomicAdd(&h[k], acc[k]);
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += blockDim.x)
        if (h[i]) atomicAdd(&counts[i], h[i]);
}

// AverageMeter.update(val, n) for a meter whose values are fp32 CUDA tensors: sum += val * n (fp32), avg = sum / count
__device__ __forceinline__ void meter_f32(float *m, int k, float val, long long n, long long count)
{
    float *v = m, *s = m + FM_F32, *a = m + 2 * FM_F32;
    v[k] = val;
    s[k] = __fadd_rn(s[k], __fmul_rn(val, (float)n));
    a[k] = fdiv_by_int(s[k], count);
}

// ... for a meter whose values are Python floats: the same in double
__device__ __forceinline__ void meter_f64(double *v, double *s, double *a, int k, double val, long long n, long long count)
{
    v[k] = val;
    s[k] = __dadd_rn(s[k], __dmul_rn(val, (double)n));
    a[k] = __ddiv_rn(s[k], (double)count);
}

// (ratio).item() * 100 with the reference's `0 if denominator == 0` guard
__device__ __forceinline__ double class_ratio(int num, int den)
{
    return den == 0 ? 0.0 : __dmul_rn((double)__fdiv_rn((float)num, (float)den), 100.0);
}

__global__ __launch_bounds__(FM_FIN_THREADS) void fm_finalize_kernel(int b, int n, int c, int n_l, int n_u,
                                                                     const float *__restrict__ loss, const float *__restrict__ sup,
                                                                     const float *__restrict__ unsup,
                                                                     const float *__restrict__ threed,
                                                                     const float *__restrict__ feat,
                                                                     const float *__restrict__ identity,
                                                                     const float *__restrict__ ema_corr, int *__restrict__ counts,
                                                                     float *__restrict__ mf32, double *__restrict__ mf64,
                                                                     long long *__restrict__ mi64, float *__restrict__ ema_corr_out)
{
    const int tid = threadIdx.x;
    // counts of meters already updated, before this iteration
    const long long cnt_all = mi64[0] + n_l + n_u, cnt_l = mi64[1] + n_l, cnt_u = mi64[2] + n_u;
    if (tid < c) {
        const int *h = counts + FM_CLS;
        const int mt = h[tid], mtg = h[c + tid], tt = h[2 * c + tid], gg = h[3 * c + tid];
        double *v = mf64 + 3 * FM_LOSS, *s = v + 3 * c, *a = s + 3 * c;
        meter_f64(v, s, a, tid, class_ratio(mtg, mt), n_u, cnt_u);            // pseudo_label_acc_classwise
        meter_f64(v, s, a, c + tid, class_ratio(mt, tt), n_u, cnt_u);         // th_meter_u_classwise
        meter_f64(v, s, a, 2 * c + tid, class_ratio(mtg, gg), n_u, cnt_u);    // th_meter_u_classwise_recall
    }
    if (tid == FM_FIN_THREADS - 1) {
        const long long bn = (long long)b * n;
        const float m = (float)counts[FM_M], fg = (float)counts[FM_FG], fg_m = (float)counts[FM_FG_M];
        const float over_th = __fmul_rn(fdiv_by_int(m, bn), 100.0f);
        const float pl_acc = counts[FM_M] == 0 ? 0.0f : __fmul_rn(__fdiv_rn((float)counts[FM_MTG], m), 100.0f);
        const float t_acc = fdiv_by_int((float)counts[FM_TG], bn);
        const float s_acc = fdiv_by_int((float)counts[FM_SG], bn);
        const float th_wobg = __fmul_rn(__fdiv_rn(fg_m, fg), 100.0f);          // unguarded: 0 / 0 = NaN, as in the reference
        const float acc_wobg = counts[FM_FG_M] == 0 ? 0.0f : __fmul_rn(__fdiv_rn((float)counts[FM_FG_MTG], fg_m), 100.0f);
        meter_f32(mf32, 0, over_th, n_u, cnt_u);
        meter_f32(mf32, 1, pl_acc, n_u, cnt_u);
        meter_f32(mf32, 2, t_acc, n_u, cnt_u);
        meter_f32(mf32, 3, s_acc, n_u, cnt_u);
        meter_f32(mf32, 4, th_wobg, n_u, cnt_u);
        meter_f32(mf32, 5, acc_wobg, n_u, cnt_u);
        double *v = mf64, *s = v + FM_LOSS, *a = s + FM_LOSS;
        meter_f64(v, s, a, 0, (double)*loss, n_l + n_u, cnt_all);
        meter_f64(v, s, a, 1, (double)*sup, n_l, cnt_l);
        meter_f64(v, s, a, 2, (double)*unsup, n_u, cnt_u);
        // NULL: the switch is off and the reference meters torch.tensor([0.]).item() (train.py:560-568, 678-679)
        meter_f64(v, s, a, 3, feat ? (double)*feat : 0.0, n_u, cnt_u);
        meter_f64(v, s, a, 4, identity ? (double)*identity : 0.0, n_u, cnt_u);
        meter_f64(v, s, a, 5, (double)*threed, n_u, cnt_u);
        mi64[3] += counts[FM_BAD];
        mi64[4] += 1;
    }
    if (ema_corr != nullptr)
        for (int i = tid; i < c * c; i += FM_FIN_THREADS) ema_corr_out[i] = ema_corr[i];
    __syncthreads();                                                            // every read of the counts is done
    if (tid == 0) {
        mi64[0] = cnt_all;
        mi64[1] = cnt_l;
        mi64[2] = cnt_u;
    }
    for (int i = tid; i < FM_CLS + 4 * c; i += FM_FIN_THREADS) counts[i] = 0;
}

} // namespace geot

using namespace geot;

GEOT_EXPORT int geot_fixmatch_meters_count(int b, int n, int c, float threshold, const long long *pseudo, const float *conf,
                                           const long long *gt, const float *prob, int *counts, void *stream)
{
    if (b < 1 || n < 1 || c < 1 || c > GEOT_NTM_MAX_C || (long long)b * n >= (1LL << 24) || !pseudo || !conf || !gt || !prob ||
        !counts)
        return hipErrorInvalidValue;
    const long long total = (long long)b * n;
    const int grid = (int)((total + FM_THREADS - 1) / FM_THREADS < 1024 ? (total + FM_THREADS - 1) / FM_THREADS : 1024);
    hipLaunchKernelGGL(fm_count_kernel, dim3(grid), dim3(FM_THREADS), 0, (hipStream_t)stream, b, n, c, threshold, pseudo, conf,
                       gt, prob, counts);
    return hipGetLastError();
}

GEOT_EXPORT int geot_fixmatch_meters_finalize(int b, int n, int c, int n_l, int n_u, const float *loss, const float *sup,
                                              const float *unsup, const float *threed, const float *ema_corr, int *counts,
                                              float *meters_f32, double *meters_f64, long long *meters_i64, float *ema_corr_out,
                                              void *stream)
{
    if (b < 1 || n < 1 || c < 1 || c > GEOT_NTM_MAX_C || n_l < 0 || n_u < 0 || !loss || !sup || !unsup || !threed || !counts ||
        !meters_f32 || !meters_f64 || !meters_i64 || (ema_corr && !ema_corr_out))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(fm_finalize_kernel, dim3(1), dim3(FM_FIN_THREADS), 0, (hipStream_t)stream, b, n, c, n_l, n_u, loss, sup,
                       unsup, threed, nullptr, nullptr, ema_corr, counts, meters_f32, meters_f64, meters_i64, ema_corr_out);
    return hipGetLastError();
}

GEOT_EXPORT int geot_fixmatch_meters_finalize6(int b, int n, int c, int n_l, int n_u, const float *loss, const float *sup,
                                               const float *unsup, const float *threed, const float *feat,
                                               const float *identity, const float *ema_corr, int *counts, float *meters_f32,
                                               double *meters_f64, long long *meters_i64, float *ema_corr_out, void *stream)
{
    if (b < 1 || n < 1 || c < 1 || c > GEOT_NTM_MAX_C || n_l < 0 || n_u < 0 || !loss || !sup || !unsup || !threed || !counts ||
        !meters_f32 || !meters_f64 || !meters_i64 || (ema_corr && !ema_corr_out))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(fm_finalize_kernel, dim3(1), dim3(FM_FIN_THREADS), 0, (hipStream_t)stream, b, n, c, n_l, n_u, loss, sup,
                       unsup, threed, feat, identity, ema_corr, counts, meters_f32, meters_f64, meters_i64, ema_corr_out);
    return hipGetLastError();
}
