// A transform list as a per-view program (geot_view_program): the reference builds a training item by running a list of
// transform classes over it on a CPU worker (openpoints/transforms/point_transformer_gpu.py); the host compiles such a list,
// with the item's random draws, into at most GEOT_VIEW_MAX_OPS fixed-size ops (geot_amd/openpoints/dataset/view_program.py)
// and this kernel interprets them.
//
// Launch shape of views.hip: one view = one job = one workgroup of 512 threads, all jobs of a batch in one launch, nothing
// returns to the host.  Thread t holds points t, t + 512, ... in registers across ALL ops (up to VIEW_PPT = 48 points, m <=
// GEOT_VIEW_REG_POINTS); the op loop is uniform over the workgroup and the op's parameters are scalar loads.  Larger clouds
// take the PPT = 0 instantiation: an op reads the cloud from where the previous op left it -- the job's own pos output row --
// VIEW_CHUNK rounds at a time and writes it back there.  A thread only ever re-reads what it wrote itself (same assignment
// of points to threads), so no barrier separates the ops, and the reduction trees see the same partials: same bits.
//
// Arithmetic: the contract of views.hip.  Every statement is one fp32 operation (-ffp-contract=off), the mean is fp64
// partial sums in the shared fixed tree (views.h), min / max propagate NaN.  The three configured lists compile to
// SCALE, STORE_X, CENTER_NORM, ROTATE, TRANSLATE, which are statement for statement what fm_views_kernel executes.
#include <vector>

#include "views.h"

namespace geot {

enum VpKind {
    VP_SCALE = 1,            // p *= f[0..2]
    VP_CENTER_NORM = 2,      // arg: bit 0 centring, bit 1 normalising, bits 2-3 gravity column; writes heights
    VP_XYZ_ALIGN = 3,        // arg: gravity column.  p -= mean; p[g] -= min(p[g])
    VP_TRANSLATE = 4,        // p += f[0..2]
    VP_SCALE_TRANSLATE = 5,  // p = p * f[0..2] + f[3..5]   (two roundings)
    VP_JITTER = 6,           // arg: noise row of the job.  p += noise
    VP_SCALE_JITTER = 7,     // arg: noise row of the job.  p = p * f[0..2] + noise
    VP_ROTATE = 8,           // p_k = (p0 f[3k] + p1 f[3k+1]) + p2 f[3k+2]
    VP_FLIP = 9,             // arg: axis.  p[axis] = max(all coordinates) - p[axis]
    VP_ZERO = 10,            // p = 0
    VP_MASK = 11,            // arg: mask row of the job.  p *= mask
    VP_STORE_X = 12,         // arg: bits 0-1 mode (0 x = p, 1 x = 0, 2 x = p * mask), bits 2.. mask row of the job
    VP_KINDS = 13
};

struct VpOp {
    int kind, arg;
    float f[12];
};
struct VpJob {           // GEOT_VIEW_PROGRAM_JOB_WORDS words, include/geot_hip.h
    int src_row, out_row, n_ops, noise_row, mask_row, reserved[3];
    VpOp op[GEOT_VIEW_MAX_OPS];
};
static_assert(sizeof(VpJob) == GEOT_VIEW_PROGRAM_JOB_WORDS * 4, "job record layout");

// is this job safe to run?  The same test on the host (the entry point) and in the kernel (uniform over the workgroup).
__host__ __device__ inline bool vp_job_ok(const VpJob &jb, int n_rows, int n_out, int n_noise, int n_mask, bool have_heights)
{
    if (jb.src_row < 0 || jb.src_row >= n_rows || jb.out_row < 0 || jb.out_row >= n_out) return false;
    if (jb.n_ops < 0 || jb.n_ops > GEOT_VIEW_MAX_OPS) return false;
    for (int o = 0; o < jb.n_ops; ++o) {
        const int kind = jb.op[o].kind, arg = jb.op[o].arg;
        if (kind < 1 || kind >= VP_KINDS) return false;
        if (kind == VP_CENTER_NORM && (arg < 0 || (arg >> 2) > 2 || !have_heights)) return false;
        if ((kind == VP_XYZ_ALIGN || kind == VP_FLIP) && (arg < 0 || arg > 2)) return false;
        if (kind == VP_JITTER || kind == VP_SCALE_JITTER) {
            if (arg < 0 || jb.noise_row < 0 || (long long)jb.noise_row + arg >= n_noise) return false;
        }
        if (kind == VP_MASK) {
            if (arg < 0 || jb.mask_row < 0 || (long long)jb.mask_row + arg >= n_mask) return false;
        }
        if (kind == VP_STORE_X) {
            const int mode = arg & 3, row = arg >> 2;
            if (arg < 0 || mode > 2) return false;
            if (mode == 2 && (jb.mask_row < 0 || (long long)jb.mask_row + row >= n_mask)) return false;
        }
    }
    return true;
}

struct VpCtx {
    int m, tid;
    const float *cur;        // where the streaming path finds the cloud: the source row, then the job's pos row
    float *out_pos;
};

// f(p, i, live) over this thread's points: the register copy (PPT > 0), or chunks of the cloud in memory, written back to the
// job's pos row when WRITE.  The index handed to f is clamped to the last point, so that f's own loads (noise, masks: rows
// nobody writes) stay unconditional as in views.hip; `live` masks the surplus out of sums and stores.
template <int PPT, bool WRITE, typename F>
__device__ __forceinline__ void vp_each(VpCtx &c, float (&held)[PPT > 0 ? PPT : 1][3], F f)
{
    if constexpr (PPT > 0) {
        // the thread's index, opaque per pass: otherwise the 48 point indices, their byte offsets and their `live` masks are
        // common subexpressions of all passes and loop invariants of the op loop, and are kept in registers beside the cloud
        int tid = c.tid;
        asm volatile("" : "+v"(tid));
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int i = tid + k * VIEW_THREADS;
            f(held[k], (unsigned)min(i, c.m - 1), i < c.m);
            __builtin_amdgcn_sched_barrier(0);       // one point at a time (views.hip)
        }
    } else {
        const int rounds = (c.m + VIEW_THREADS - 1) / VIEW_THREADS;
        for (int k0 = 0; k0 < rounds; k0 += VIEW_CHUNK) {
            float q[VIEW_CHUNK][3];
#pragma unroll
            for (int k = 0; k < VIEW_CHUNK; ++k) {
                // a slot past the end loads nothing (the register form clamps instead: it only ever loads from the source
                // row, which nobody writes; here the last point may be being rewritten by its owner in this very pass)
                const unsigned i = (unsigned)(c.tid + (k0 + k) * VIEW_THREADS);
                q[k][0] = q[k][1] = q[k][2] = 0.f;
                if (i < (unsigned)c.m) {
                    q[k][0] = view_ld(c.cur, 12u * i);
                    q[k][1] = view_ld(c.cur, 12u * i + 4u);
                    q[k][2] = view_ld(c.cur, 12u * i + 8u);
                }
            }
#pragma unroll
            for (int k = 0; k < VIEW_CHUNK; ++k) {
                const int i = c.tid + (k0 + k) * VIEW_THREADS;
                const bool live = i < c.m;
                f(q[k], (unsigned)min(i, c.m - 1), live);
                if (WRITE && live) {
                    view_st(c.out_pos, 12u * (unsigned)i, q[k][0]);
                    view_st(c.out_pos, 12u * (unsigned)i + 4u, q[k][1]);
                    view_st(c.out_pos, 12u * (unsigned)i + 8u, q[k][2]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (WRITE) c.cur = c.out_pos;
    }
}

// a value in a register of its own.  The compiler merges a point's three loads (and stores) into one 96-bit access, whose
// operand is a register TUPLE -- allocated even-aligned, four registers for three -- and without this copy the register
// copy of the cloud is carried as 48 such tuples through every op, which no longer fits beside the ops' temporaries.
__device__ __forceinline__ float vp_own(float v)
{
    float r;
    asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "v"(v));
    return r;
}

// column g of a point by selection: a run-time index into p would put the register copy in scratch
__device__ __forceinline__ float vp_col(const float (&p)[3], int g) { return g == 0 ? p[0] : (g == 1 ? p[1] : p[2]); }

// One op kind of the interpreter: a diamond of its own whose other side leaves the cloud untouched.  `kind` is made opaque
// in front of every test, so that the tests are not threaded into one multi-way branch: at the join of a 12-way branch the
// register copy of the cloud exists once per incoming edge as far as the register allocator is concerned, and spills.
#define VP_WHEN(cond)                                                                                                          \
    asm volatile("" : "+s"(kind));                                                                                             \
    if (cond)

template <int PPT>
__global__ __launch_bounds__(VIEW_THREADS) void view_program_kernel(int m, int n_rows, int n_out, int n_noise, int n_mask,
                                                                     const float *__restrict__ raw,
                                                                     const VpJob *__restrict__ jobs,
                                                                     const float *__restrict__ noise,
                                                                     const float *__restrict__ mask, float *__restrict__ pos,
                                                                     float *__restrict__ x, float *__restrict__ heights,
                                                                     float *__restrict__ view_center, float *__restrict__ view_scale)
{
    __shared__ double red_sum[VIEW_WAVES][3];
    __shared__ float red_min[VIEW_WAVES], red_ext[VIEW_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, job = blockIdx.x;
    const VpJob &jb = jobs[job];
    if (!vp_job_ok(jb, n_rows, n_out, n_noise, n_mask, heights != nullptr)) {     // (uniform over the workgroup)
        if (tid < 3) view_center[job * 3 + tid] = NAN;
        if (tid == 3) view_scale[job] = NAN;
        return;
    }
    float *out_x = x + (size_t)jb.out_row * m * 3;
    float *out_h = heights ? heights + (size_t)jb.out_row * m : nullptr;
    VpCtx c = {m, tid, raw + (size_t)jb.src_row * m * 3, pos + (size_t)jb.out_row * m * 3};
    float held[PPT > 0 ? PPT : 1][3];
    if constexpr (PPT > 0) {
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const unsigned i = min((unsigned)(tid + k * VIEW_THREADS), (unsigned)(m - 1));
            held[k][0] = vp_own(view_ld(c.cur, 12u * i));
            held[k][1] = vp_own(view_ld(c.cur, 12u * i + 4u));
            held[k][2] = vp_own(view_ld(c.cur, 12u * i + 8u));
        }
    }
    float cx = 0.f, cy = 0.f, cz = 0.f, top = 1.f;       // what view_center / view_scale report: the last centring op's

    // the column sums and the minimum of column g, reduced over the workgroup
    auto sum_min = [&](int g, double (&tot)[3], float &low) {
        ViewRed r = {{0, 0, 0}, INFINITY, 0.f};
        vp_each<PPT, false>(c, held, [&](float (&p)[3], unsigned, bool live) {
            const double s0 = r.sum[0] + (double)p[0], s1 = r.sum[1] + (double)p[1], s2 = r.sum[2] + (double)p[2];
            const float lo = nan_min(r.mn, vp_col(p, g));
            r.sum[0] = live ? s0 : r.sum[0];
            r.sum[1] = live ? s1 : r.sum[1];
            r.sum[2] = live ? s2 : r.sum[2];
            r.mn = live ? lo : r.mn;
        });
        __syncthreads();                         // the arrays may still be being read from the previous reduction
        view_reduce_sum_min(r, red_sum, red_min, wave, tot, low);
    };

    const int n_ops = jb.n_ops;
    for (int o = 0; o < n_ops; ++o) {
        const VpOp &op = jb.op[o];
        int kind = op.kind;
        const int arg = op.arg;
        VP_WHEN(kind == VP_SCALE) {
            const float s0 = op.f[0], s1 = op.f[1], s2 = op.f[2];
            vp_each<PPT, true>(c, held, [&](float (&p)[3], unsigned, bool) {
                p[0] = p[0] * s0;
                p[1] = p[1] * s1;
                p[2] = p[2] * s2;
            });
        }
        VP_WHEN(kind == VP_TRANSLATE) {
            const float t0 = op.f[0], t1 = op.f[1], t2 = op.f[2];
            vp_each<PPT, true>(c, held, [&](float (&p)[3], unsigned, bool) {
                p[0] = p[0] + t0;
                p[1] = p[1] + t1;
                p[2] = p[2] + t2;
            });
        }
        VP_WHEN(kind == VP_SCALE_TRANSLATE) {
            const float s0 = op.f[0], s1 = op.f[1], s2 = op.f[2], t0 = op.f[3], t1 = op.f[4], t2 = op.f[5];
            vp_each<PPT, true>(c, held, [&](float (&p)[3], unsigned, bool) {
                p[0] = p[0] * s0 + t0;
                p[1] = p[1] * s1 + t1;
                p[2] = p[2] * s2 + t2;
            });
        }
        VP_WHEN(kind == VP_JITTER || kind == VP_SCALE_JITTER) {
            const float *nz = noise + (size_t)(jb.noise_row + arg) * m * 3;
            const bool scale = kind == VP_SCALE_JITTER;
            const float s0 = op.f[0], s1 = op.f[1], s2 = op.f[2];
            vp_each<PPT, true>(c, held, [&](float (&p)[3], unsigned i, bool) {
                const float n0 = view_ld(nz, 12u * i), n1 = view_ld(nz, 12u * i + 4u), n2 = view_ld(nz, 12u * i + 8u);
                p[0] = (scale ? p[0] * s0 : p[0]) + n0;
                p[1] = (scale ? p[1] * s1 : p[1]) + n1;
                p[2] = (scale ? p[2] * s2 : p[2]) + n2;
            });
        }
        VP_WHEN(kind == VP_ROTATE) {
            float R[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = op.f[k];
            vp_each<PPT, true>(c, held, [&](float (&p)[3], unsigned, bool) {
                const float r0 = (p[0] * R[0] + p[1] * R[1]) + p[2] * R[2];
                const float r1 = (p[0] * R[3] + p[1] * R[4]) + p[2] * R[5];
                const float r2 = (p[0] * R[6] + p[1] * R[7]) + p[2] * R[8];
                p[0] = r0;
                p[1] = r1;
                p[2] = r2;
            });
        }
        VP_WHEN(kind == VP_ZERO) {
            vp_each<PPT, true>(c, held, [&](float (&p)[3], unsigned, bool) { p[0] = p[1] = p[2] = 0.f; });
        }
        VP_WHEN(kind == VP_MASK) {
            const float *mk = mask + (size_t)(jb.mask_row + arg) * m;
            vp_each<PPT, true>(c, held, [&](float (&p)[3], unsigned i, bool) {
                const float k = view_ld(mk, 4u * i);
                p[0] = p[0] * k;
                p[1] = p[1] * k;
                p[2] = p[2] * k;
            });
        }
        VP_WHEN(kind == VP_STORE_X) {
            const int mode = arg & 3;
            const float *mk = mode == 2 ? mask + (size_t)(jb.mask_row + (arg >> 2)) * m : raw;      // (raw: never read)
            vp_each<PPT, false>(c, held, [&](float (&p)[3], unsigned i, bool live) {
                const float k = mode == 2 ? view_ld(mk, 4u * i) : 1.f;
                const float x0 = mode == 0 ? p[0] : (mode == 1 ? 0.f : p[0] * k);
                const float x1 = mode == 0 ? p[1] : (mode == 1 ? 0.f : p[1] * k);
                const float x2 = mode == 0 ? p[2] : (mode == 1 ? 0.f : p[2] * k);
                if (live) {
                    view_st(out_x, 4u * i, x0);
                    view_st(out_x, 4u * ((unsigned)m + i), x1);
                    view_st(out_x, 4u * (2u * (unsigned)m + i), x2);
                }
            });
        }
        VP_WHEN(kind == VP_FLIP) {
            float mx = -INFINITY;
            vp_each<PPT, false>(c, held, [&](float (&p)[3], unsigned, bool live) {
                const float hi = nan_max(nan_max(nan_max(mx, p[0]), p[1]), p[2]);
                mx = live ? hi : mx;
            });
            __syncthreads();                     // red_ext may still be being read from the previous reduction
            const float all = view_reduce_ext<true>(mx, red_ext, wave);
            vp_each<PPT, true>(c, held, [&](float (&p)[3], unsigned, bool) {
                p[0] = arg == 0 ? all - p[0] : p[0];
                p[1] = arg == 1 ? all - p[1] : p[1];
                p[2] = arg == 2 ? all - p[2] : p[2];
            });
        }
        VP_WHEN(kind == VP_XYZ_ALIGN) {
            // p -= mean, then the gravity column's minimum of the centred cloud leaves that column
            double tot[3];
            float low;
            sum_min(arg, tot, low);
            cx = (float)(tot[0] / (double)m);
            cy = (float)(tot[1] / (double)m);
            cz = (float)(tot[2] / (double)m);
            top = 1.f;
            float mn = INFINITY;
            vp_each<PPT, true>(c, held, [&](float (&p)[3], unsigned, bool live) {
                p[0] = p[0] - cx;
                p[1] = p[1] - cy;
                p[2] = p[2] - cz;
                const float lo = nan_min(mn, vp_col(p, arg));
                mn = live ? lo : mn;
            });
            __syncthreads();
            const float floor_ = view_reduce_ext<false>(mn, red_ext, wave);
            vp_each<PPT, true>(c, held, [&](float (&p)[3], unsigned, bool) {
                p[0] = arg == 0 ? p[0] - floor_ : p[0];
                p[1] = arg == 1 ? p[1] - floor_ : p[1];
                p[2] = arg == 2 ? p[2] - floor_ : p[2];
            });
        }
        VP_WHEN(kind == VP_CENTER_NORM) {
            const bool centre = arg & 1, normalise = arg & 2;
            const int g = arg >> 2;
            double tot[3];
            float low;
            sum_min(g, tot, low);
            // without centring the "mean" taken off is +0: p - 0 is p, bit for bit, and the pass stays free of branches
            cx = centre ? (float)(tot[0] / (double)m) : 0.f;
            cy = centre ? (float)(tot[1] / (double)m) : 0.f;
            cz = centre ? (float)(tot[2] / (double)m) : 0.f;
            top = 1.f;
            // heights of the un-centred cloud, the centred cloud and its largest norm
            float mx = 0.f;
            vp_each<PPT, true>(c, held, [&](float (&p)[3], unsigned i, bool live) {
                const float gq = vp_col(p, g);
                p[0] = p[0] - cx;
                p[1] = p[1] - cy;
                p[2] = p[2] - cz;
                const float hi = nan_max(mx, sqrtf((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]));
                mx = live ? hi : mx;
                if (live) view_st(out_h, 4u * i, gq - low);
            });
            if (normalise) {
                __syncthreads();
                top = view_reduce_ext<true>(mx, red_ext, wave);
                vp_each<PPT, true>(c, held, [&](float (&p)[3], unsigned, bool) {
                    p[0] = p[0] / top;
                    p[1] = p[1] / top;
                    p[2] = p[2] / top;
                });
            }
        }
    }

    if constexpr (PPT > 0) {
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int i = tid + k * VIEW_THREADS;
            if (i < m) {
                view_st(c.out_pos, 12u * (unsigned)i, vp_own(held[k][0]));
                view_st(c.out_pos, 12u * (unsigned)i + 4u, vp_own(held[k][1]));
                view_st(c.out_pos, 12u * (unsigned)i + 8u, vp_own(held[k][2]));
            }
        }
    } else if (c.cur != c.out_pos) {             // no op wrote the cloud: pos is the source row
        vp_each<PPT, true>(c, held, [&](float (&)[3], unsigned, bool) {});
    }
    if (tid == 0) {
        view_center[job * 3] = cx;
        view_center[job * 3 + 1] = cy;
        view_center[job * 3 + 2] = cz;
        view_scale[job] = top;
    }
}

#undef VP_WHEN

} // namespace geot

using namespace geot;

GEOT_EXPORT int geot_view_program(int j, int m, int n_rows, int n_out, int n_noise, int n_mask, const float *raw,
                                  const void *jobs_host, const void *jobs, const float *noise, const float *mask, float *pos,
                                  float *x, float *heights, float *view_center, float *view_scale, void *stream)
{
    if (j < 1 || j > 65535 || m < 1 || n_rows < 1 || n_out < 1 || n_noise < 0 || n_mask < 0) return hipErrorInvalidValue;
    if ((long long)m * 12 > 0xffffffffLL) return hipErrorInvalidValue;     // 32-bit byte offsets inside a row
    if (!raw || !jobs_host || !jobs || !pos || !x || !view_center || !view_scale) return hipErrorInvalidValue;
    if ((n_noise > 0 && !noise) || (n_mask > 0 && !mask)) return hipErrorInvalidValue;
    // the records, read on the host: every row, op count and op kind in range, each output row named once
    const VpJob *host = (const VpJob *)jobs_host;
    std::vector<bool> taken((size_t)n_out, false);
    for (int i = 0; i < j; ++i) {
        if (!vp_job_ok(host[i], n_rows, n_out, n_noise, n_mask, heights != nullptr)) return hipErrorInvalidValue;
        if (taken[(size_t)host[i].out_row]) return hipErrorInvalidValue;
        taken[(size_t)host[i].out_row] = true;
    }
    hipStream_t s = (hipStream_t)stream;
    const VpJob *jb = (const VpJob *)jobs;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(j), dim3(VIEW_THREADS), 0, s, m, n_rows, n_out, n_noise, n_mask, raw, jb, noise, mask,
                           pos, x, heights, view_center, view_scale);
    };
    if (m <= GEOT_VIEW_REG_POINTS) launch(view_program_kernel<VIEW_PPT>);
    else launch(view_program_kernel<0>);
    return hipGetLastError();
}
