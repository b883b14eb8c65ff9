// The random draws of a batch's transform lists on the GPU (geot_view_draw): what ViewProgram.draw does per item on the host
// with three global generators -- a handful of scalars per view, and for the jittering and per-point colour dropping
// transforms one (m, 3) normal or (m,) uniform row per item, multiplied, clamped and uploaded -- in ONE launch in front of
// geot_view_program, which then reads its job table, noise rows and mask rows from device buffers this kernel filled.
//
// Per job the host compiles, with nothing random in it, a TEMPLATE record (a geot_view_program job whose op list is the
// list's worst case: both flips, the zeroing, the masked store) and a PLAN (which quantities the list draws, their constant
// bounds, which op of the template each one lands in).  The kernel copies the template, overwrites the drawn fields -- an
// un-taken FLIP or ZERO becomes SCALE by (1, 1, 1), a bit-exact no-op; STORE_X's mode follows the drop draw -- and fills the
// job's noise and mask rows.  Philox4x32-10 (philox.h), key = seed, counter = (element, tag, draw id lo, draw id hi); the
// tag (view_draw.h vd_tag) names the slot's view, the step's place in the list and the quantity.  No state, no atomics, no
// workspace: grid (ceil(m / 256), jobs), thread i of a job draws point i of every noise and mask row of that job, and the
// first block's thread k draws step k's scalars (view_draw.h vd_draw_step, vd_draw_point).  The arithmetic is view_draw.h's: one rounded fp32 operation per statement
// (-ffp-contract=off), no math-library call; tests/_view_draw_ref.py restates it in numpy.
#include <hip/hip_runtime.h>

#include "geot_common.h"
#include "view_draw.h"

namespace geot {

typedef unsigned long long u64;
constexpr int VD_THREADS = 256;

__global__ __launch_bounds__(VD_THREADS) void view_draw_kernel(int m, int n_noise, int n_mask, const VdJob *__restrict__ tmpl,
                                                              const VdPlan *__restrict__ plans, u64 seed, u64 draw_base,
                                                              VdJob *__restrict__ jobs, float *__restrict__ noise,
                                                              float *__restrict__ mask)
{
    const int j = blockIdx.y, tid = threadIdx.x;
    const VdJob &tj = tmpl[j];
    const VdPlan &pl = plans[j];
    if (!vd_plan_ok(pl, tj, n_noise, n_mask)) return;              // (uniform over the job's blocks) a bad plan writes nothing
    const u64 d = draw_base + (u64)pl.slot;
    const VdKey key = {(uint32_t)d, (uint32_t)(d >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), pl.view};

    if (blockIdx.x == 0) {
        const int *src = (const int *)&tj;
        int *dst = (int *)&jobs[j];
        for (int w = tid; w < GEOT_VIEW_PROGRAM_JOB_WORDS; w += VD_THREADS) dst[w] = src[w];
        __syncthreads();
        if (tid < pl.n_steps) vd_draw_step(pl, pl.step[tid], key, jobs[j]);
    }

    const uint32_t i = blockIdx.x * VD_THREADS + tid;
    if (i < (uint32_t)m) vd_draw_point(pl, tj, key, i, m, noise, mask);
}

} // namespace geot

using namespace geot;

GEOT_EXPORT int geot_view_draw(int j, int m, int n_noise, int n_mask, const void *tmpl_host, const void *plans_host,
                               const void *tmpl, const void *plans, unsigned long long seed, unsigned long long draw_base,
                               void *jobs, float *noise, float *mask, void *stream)
{
    if (j < 1 || j > 65535 || m < 1 || n_noise < 0 || n_mask < 0) return hipErrorInvalidValue;
    if ((long long)m * 12 > 0xffffffffLL) return hipErrorInvalidValue;             // geot_view_program's bound on a row
    if (!tmpl_host || !plans_host || !tmpl || !plans || !jobs) return hipErrorInvalidValue;
    if ((n_noise > 0 && !noise) || (n_mask > 0 && !mask)) return hipErrorInvalidValue;
    const VdJob *th = (const VdJob *)tmpl_host;
    const VdPlan *ph = (const VdPlan *)plans_host;
    for (int i = 0; i < j; ++i)
        if (!vd_plan_ok(ph[i], th[i], n_noise, n_mask)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(view_draw_kernel, dim3(((unsigned)m + VD_THREADS - 1) / VD_THREADS, (unsigned)j), dim3(VD_THREADS), 0,
                       (hipStream_t)stream, m, n_noise, n_mask, (const VdJob *)tmpl, (const VdPlan *)plans, seed, draw_base,
                       (VdJob *)jobs, noise, mask);
    return hipGetLastError();
}
