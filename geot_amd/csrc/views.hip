// The FixMatch views of a sampled scan (geot_fixmatch_views): what the reference's transform lists do per item on CPU workers
// (openpoints/transforms/point_transformer_gpu.py; cfgs/tooth_semi/transformer_finetune_fixmatch_ntm.yaml datatransforms):
//
//   labelled   PointCloudScaling, PointCloudCenterAndNormalize
//   weak       PointCloudCenterAndNormalize
//   strong     PointCloudScaling_s, PointCloudCenterAndNormalize, PointCloudRotation_s, PointCloudTranslation_s
//
// one view = one job = one workgroup of 512 threads; all jobs of a batch are one launch.  A batch has B_l + 2 B_u jobs (6 at
// the configured sizes), so the launch is latency-bound by construction: what counts is that a job reads its cloud once,
// keeps it in registers through the three phases (sums + minimum, maximum norm, output) and that nothing returns to the
// host in between.  Thread t holds points t, t + 512, ...: up to VIEW_PPT = 48 of them (m <= 24 576), 144 VGPRs of the 256
// a 512-thread workgroup leaves each thread (at 1024 threads and 128 registers the 72 held values spilled).  Larger clouds
// take the PPT = 0 instantiation, which re-reads the cloud in every phase, VIEW_CHUNK rounds at a time -- the same
// assignment of points to threads and the same reduction trees, hence the same bits.  Loads are unconditional (the index
// is clamped to the last point, the surplus is masked out of the sums and never stored), so a thread's loads are all in
// flight together instead of one per branch.
// (A point is 12 bytes: a wave's dwordx3 loads cover 768 contiguous bytes; no cache line is fetched twice.)
//
// Arithmetic: every statement is one fp32 operation (the translation unit is built with -ffp-contract=off; nothing here is
// an explicit fma) except the mean: fp64 partial sums per thread in index order, a butterfly over the wave, the 8 wave sums
// added in wave order, one division, one rounding.  min / max propagate NaN like torch.min / torch.max.
#include "views.h"

namespace geot {

struct ViewJob {         // GEOT_VIEW_JOB_WORDS words, include/geot_hip.h
    int src_row, out_row, flags, reserved0;
    float s[3], R[9], t[3], reserved1;
};
static_assert(sizeof(ViewJob) == GEOT_VIEW_JOB_WORDS * 4, "job record layout");

// q[c] = r * s for rounds k0 .. k0 + N - 1 of this thread (one multiply per element)
template <int N>
__device__ __forceinline__ void view_load(const float *__restrict__ src, int m, int tid, int k0, const ViewJob &jb, float (&q)[N][3])
{
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const unsigned i = min((unsigned)(tid + (k0 + c) * VIEW_THREADS), (unsigned)(m - 1));
        q[c][0] = view_ld(src, 12u * i) * jb.s[0];
        q[c][1] = view_ld(src, 12u * i + 4u) * jb.s[1];
        q[c][2] = view_ld(src, 12u * i + 8u) * jb.s[2];
    }
}

// phase 1: x = q (channel-first), column sums, minimum of the gravity column
template <int N, int G>
__device__ __forceinline__ void view_phase1(int m, int tid, int k0, const float (&q)[N][3], float *__restrict__ out_x, ViewRed &r)
{
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const int i = tid + (k0 + c) * VIEW_THREADS;
        const bool live = i < m;
        const float gq = q[c][G];
        const double s0 = r.sum[0] + (double)q[c][0], s1 = r.sum[1] + (double)q[c][1], s2 = r.sum[2] + (double)q[c][2];
        const float lo = nan_min(r.mn, gq);
        r.sum[0] = live ? s0 : r.sum[0];
        r.sum[1] = live ? s1 : r.sum[1];
        r.sum[2] = live ? s2 : r.sum[2];
        r.mn = live ? lo : r.mn;
        if (live) {
            view_st(out_x, 4u * (unsigned)i, q[c][0]);
            view_st(out_x, 4u * ((unsigned)m + (unsigned)i), q[c][1]);
            view_st(out_x, 4u * (2u * (unsigned)m + (unsigned)i), q[c][2]);
        }
        __builtin_amdgcn_sched_barrier(0);       // one point at a time: the scheduler otherwise interleaves all and spills
    }
}

// phase 2: heights, and the largest norm of the centred cloud
template <int N, int G>
__device__ __forceinline__ void view_phase2(int m, int tid, int k0, const float (&q)[N][3], float low, float cx, float cy,
                                            float cz, float *__restrict__ out_h, ViewRed &r)
{
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const int i = tid + (k0 + c) * VIEW_THREADS;
        const bool live = i < m;
        const float gq = q[c][G];
        const float a = q[c][0] - cx, b = q[c][1] - cy, d = q[c][2] - cz;
        const float hi = nan_max(r.mx, sqrtf((a * a + b * b) + d * d));
        r.mx = live ? hi : r.mx;
        if (live) view_st(out_h, 4u * (unsigned)i, gq - low);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// phase 3: pos = (q - mean) / mx, then the strong view's rotation and shift
template <int N>
__device__ __forceinline__ void view_phase3(int m, int tid, int k0, const ViewJob &jb, const float (&q)[N][3], float cx, float cy,
                                            float cz, float top, float *__restrict__ out_pos)
{
    const bool rotate = jb.flags & 1, shift = jb.flags & 2;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const int i = tid + (k0 + c) * VIEW_THREADS;
        float p0 = (q[c][0] - cx) / top, p1 = (q[c][1] - cy) / top, p2 = (q[c][2] - cz) / top;
        if (rotate) {
            const float r0 = (p0 * jb.R[0] + p1 * jb.R[1]) + p2 * jb.R[2];
            const float r1 = (p0 * jb.R[3] + p1 * jb.R[4]) + p2 * jb.R[5];
            const float r2 = (p0 * jb.R[6] + p1 * jb.R[7]) + p2 * jb.R[8];
            p0 = r0;
            p1 = r1;
            p2 = r2;
        }
        if (shift) {
            p0 = p0 + jb.t[0];
            p1 = p1 + jb.t[1];
            p2 = p2 + jb.t[2];
        }
        if (i < m) {
            view_st(out_pos, 12u * (unsigned)i, p0);
            view_st(out_pos, 12u * (unsigned)i + 4u, p1);
            view_st(out_pos, 12u * (unsigned)i + 8u, p2);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int PPT, int G>      // G: the gravity column (a run-time choice among q[c][0..2] would put the array in scratch)
__global__ __launch_bounds__(VIEW_THREADS) void fm_views_kernel(int m, int n_rows, int n_out,
                                                                 const float *__restrict__ raw,
                                                                 const ViewJob *__restrict__ jobs, float *__restrict__ pos,
                                                                 float *__restrict__ x, float *__restrict__ heights,
                                                                 float *__restrict__ view_center, float *__restrict__ view_scale)
{
    __shared__ double red_sum[VIEW_WAVES][3];
    __shared__ float red_min[VIEW_WAVES], red_max[VIEW_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, job = blockIdx.x;
    const ViewJob jb = jobs[job];
    if (jb.src_row < 0 || jb.src_row >= n_rows || jb.out_row < 0 || jb.out_row >= n_out) {     // (uniform over the workgroup)
        if (tid < 3) view_center[job * 3 + tid] = NAN;
        if (tid == 3) view_scale[job] = NAN;
        return;
    }
    const float *src = raw + (size_t)jb.src_row * m * 3;
    float *out_pos = pos + (size_t)jb.out_row * m * 3;
    float *out_x = x + (size_t)jb.out_row * m * 3;
    float *out_h = heights + (size_t)jb.out_row * m;
    constexpr bool HOLD = PPT > 0;
    const int rounds = HOLD ? PPT : (m + VIEW_THREADS - 1) / VIEW_THREADS;
    float held[HOLD ? PPT : 1][3];

    ViewRed r = {{0, 0, 0}, INFINITY, 0.f};
    if constexpr (HOLD) {
        view_load<PPT>(src, m, tid, 0, jb, held);
        view_phase1<PPT, G>(m, tid, 0, held, out_x, r);
    } else {
        for (int k0 = 0; k0 < rounds; k0 += VIEW_CHUNK) {
            float q[VIEW_CHUNK][3];
            view_load<VIEW_CHUNK>(src, m, tid, k0, jb, q);
            view_phase1<VIEW_CHUNK, G>(m, tid, k0, q, out_x, r);
        }
    }
    double tot[3];
    float low;
    view_reduce_sum_min(r, red_sum, red_min, wave, tot, low);
    const float cx = (float)(tot[0] / (double)m), cy = (float)(tot[1] / (double)m), cz = (float)(tot[2] / (double)m);

    if constexpr (HOLD) {
        view_phase2<PPT, G>(m, tid, 0, held, low, cx, cy, cz, out_h, r);
    } else {
        for (int k0 = 0; k0 < rounds; k0 += VIEW_CHUNK) {
            float q[VIEW_CHUNK][3];
            view_load<VIEW_CHUNK>(src, m, tid, k0, jb, q);
            view_phase2<VIEW_CHUNK, G>(m, tid, k0, q, low, cx, cy, cz, out_h, r);
        }
    }
    const float top = view_reduce_ext<true>(r.mx, red_max, wave);
    if (tid == 0) {
        view_center[job * 3] = cx;
        view_center[job * 3 + 1] = cy;
        view_center[job * 3 + 2] = cz;
        view_scale[job] = top;
    }

    if constexpr (HOLD) {
        view_phase3<PPT>(m, tid, 0, jb, held, cx, cy, cz, top, out_pos);
    } else {
        for (int k0 = 0; k0 < rounds; k0 += VIEW_CHUNK) {
            float q[VIEW_CHUNK][3];
            view_load<VIEW_CHUNK>(src, m, tid, k0, jb, q);
            view_phase3<VIEW_CHUNK>(m, tid, k0, jb, q, cx, cy, cz, top, out_pos);
        }
    }
}

} // namespace geot

using namespace geot;

GEOT_EXPORT int geot_fixmatch_views(int j, int m, int n_rows, int n_out, int gravity_dim, const float *raw, const void *jobs,
                                    float *pos, float *x, float *heights, float *view_center, float *view_scale, void *stream)
{
    if (j < 1 || m < 1 || n_rows < 1 || n_out < 1 || gravity_dim < 0 || gravity_dim > 2) return hipErrorInvalidValue;
    if ((long long)m * 12 > 0xffffffffLL) return hipErrorInvalidValue;     // 32-bit byte offsets inside a row
    if (!raw || !jobs || !pos || !x || !heights || !view_center || !view_scale) return hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const ViewJob *jb = (const ViewJob *)jobs;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(j), dim3(VIEW_THREADS), 0, s, m, n_rows, n_out, raw, jb, pos, x, heights, view_center,
                           view_scale);
    };
    const bool hold = m <= GEOT_VIEW_REG_POINTS;
    if (gravity_dim == 0) hold ? launch(fm_views_kernel<VIEW_PPT, 0>) : launch(fm_views_kernel<0, 0>);
    else if (gravity_dim == 1) hold ? launch(fm_views_kernel<VIEW_PPT, 1>) : launch(fm_views_kernel<0, 1>);
    else hold ? launch(fm_views_kernel<VIEW_PPT, 2>) : launch(fm_views_kernel<0, 2>);
    return hipGetLastError();
}
