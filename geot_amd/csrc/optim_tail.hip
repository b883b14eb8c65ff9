// The tail of a training iteration behind its backward as one multi-tensor pass (include/geot_hip.h "ABI 25"): the global
// gradient norm of torch.nn.utils.clip_grad_norm_ (norm_type 2, error_if_nonfinite=False), torch.optim.AdamW's update and
// the exponential moving average that makes a mean teacher follow its student -- two sweeps over a list of tensor records.
//
//   geot_optim_tail_norm    sweep 1: every workgroup sums the squares of its OT_BLOCK gradient elements and stores the sum in
//                           a slot of its own (no float atomics, every slot written: nothing to clear)
//   geot_optim_tail_finish  one workgroup: the slots summed in a fixed order in double -> total_norm, coef; the step counters
//                           of the records it is handed go up by one
//   geot_optim_tail_update  sweep 2: g' = coef g, AdamW, t = d t + (1 - d) p_new, every parameter read once
//
// With step_per_update = k > 1 (ABI 27) the gradients of k calls are summed before one update, gated on a counter in device
// memory, so that every call issues the same launches and one captured graph serves every call of a window:
//
//   geot_optim_tail_accumulate  sweep 1': acc = acc + g in a flat fp32 accumulator (one writer per element), and the sum of the
//                               squares of the NEW accumulator values per workgroup, partitioned and ordered as sweep 1 does
//   geot_optim_tail_acc_finish  one workgroup: raises the window counter; on call k of a window it does what
//                               geot_optim_tail_finish does and resets the counter, otherwise nothing else
//   geot_optim_tail_acc_update  sweep 2 with the accumulated value in the place of g, which it then zeroes; its workgroups
//                               return at once on a call that is no update
//
// The records travel BY VALUE in the kernel arguments, OT_CAP per launch (gradient addresses are new every iteration, and
// under graph capture an upload would be a memcpy node): the entry points read a host table and issue ceil(T / OT_CAP)
// launches per sweep.  A workgroup finds its record by a scan of the launch's first-block indices (uniform, scalar loads).
// Which records take the dwordx4 path, how many workgroups each gets and how many launches a sweep takes is decided by one
// function, ot_plan, which geot_optim_tail_plan exposes.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "geot_common.h"
#include "geot_hip.h"

namespace geot {

constexpr int OT_THREADS = 256;
constexpr int OT_BLOCK = GEOT_OPTIM_TAIL_BLOCK_ELEMS;
constexpr int OT_CAP = GEOT_OPTIM_TAIL_CAP;
constexpr int OT_STEP_CAP = GEOT_OPTIM_TAIL_STEP_CAP;
constexpr int OT_PER_THREAD = OT_BLOCK / OT_THREADS;      // 16 elements, as 4 quads on the vector path
static_assert(OT_BLOCK % (OT_THREADS * 4) == 0, "a block is whole quads per thread");

struct OtRec {                       // = one host record, GEOT_OPTIM_TAIL_REC_WORDS 32-bit words
    float *p;
    const float *g;
    float *m;
    float *v;
    float *t;
    long long n;
    int first_block;                 // filled by the launcher: the record's first workgroup within its launch
    int group;
    int flags;                       // GEOT_OPTIM_TAIL_VECTOR is the launcher's to set (from ot_plan)
    int step;                        // index of the record's step counter
};
static_assert(sizeof(OtRec) == 4 * GEOT_OPTIM_TAIL_REC_WORDS, "record layout");

struct OtGroup {                     // = one host group record, GEOT_OPTIM_TAIL_GROUP_WORDS words
    double beta1, beta2;
    float eps, weight_decay, lr;
    int pad;
    const float *lr_ptr;             // non-NULL: the learning rate is read from this device float
};
static_assert(sizeof(OtGroup) == 4 * GEOT_OPTIM_TAIL_GROUP_WORDS, "group layout");

struct OtTable { OtRec r[OT_CAP]; };
struct OtGroups { OtGroup g[GEOT_OPTIM_TAIL_MAX_GROUPS]; };
struct OtSteps { int idx[OT_STEP_CAP]; };
static_assert(sizeof(OtTable) + sizeof(OtGroups) + 64 <= 4096 && sizeof(OtSteps) + 64 <= 4096, "kernel arguments fit 4 KB");

// ---- the plan: the one place that decides paths, workgroups and launches ------------------------------------------------------
struct OtPlan {
    std::vector<long long> blocks;   // workgroups of each record (both sweeps)
    std::vector<int> vec;            // 1: dwordx4 path
    long long update_launches = 0, norm_launches = 0, update_blocks = 0, slots = 0;
};

static inline bool ot_adamw_record(int flags) { return !(flags & (GEOT_OPTIM_TAIL_EMA_ONLY | GEOT_OPTIM_TAIL_INT64)); }
static inline bool ot_in_norm(int flags) { return ot_adamw_record(flags) && (flags & GEOT_OPTIM_TAIL_CLIPPED); }

static bool ot_plan(int t, const long long *counts, const int *aligned, const int *flags, OtPlan &plan)
{
    if (t < 0) return false;
    plan.blocks.assign((size_t)t, 0);
    plan.vec.assign((size_t)t, 0);
    long long in_launch = 0, norm_in_launch = 0;
    int norm_records = 0;
    for (int i = 0; i < t; ++i) {
        if (counts[i] < 0) return false;
        const long long nb = (counts[i] + OT_BLOCK - 1) / OT_BLOCK;
        plan.blocks[(size_t)i] = nb;
        plan.vec[(size_t)i] = (aligned[i] && !(flags[i] & GEOT_OPTIM_TAIL_INT64)) ? 1 : 0;
        plan.update_blocks += nb;
        in_launch += nb;
        if (i % OT_CAP == OT_CAP - 1 || i == t - 1) {       // a launch of OT_CAP records ends here; an empty one is not issued
            plan.update_launches += in_launch > 0;
            in_launch = 0;
        }
        if (ot_in_norm(flags[i])) {
            plan.slots += nb;
            norm_in_launch += nb;
            if (++norm_records % OT_CAP == 0) {
                plan.norm_launches += norm_in_launch > 0;
                norm_in_launch = 0;
            }
        }
    }
    plan.norm_launches += norm_in_launch > 0;
    return true;
}

// ---- device side -----------------------------------------------------------------------------------------------------------
// The record of workgroup `b`: the last one whose first block is not behind b (records without elements share their
// successor's first block and are passed over).
__device__ inline int ot_find(const OtTable &tab, int count, int b)
{
    int at = 0;
    for (int i = 1; i < count; ++i)
        if (tab.r[i].first_block <= b) at = i;
    return at;
}

__device__ inline float ot_block_sum(float acc, float *lds)
{
    for (int off = GEOT_WAVE / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, GEOT_WAVE);
    const int lane = threadIdx.x % GEOT_WAVE, wave = threadIdx.x / GEOT_WAVE;
    if (lane == 0) lds[wave] = acc;
    __syncthreads();
    float total = 0.f;
    if (threadIdx.x == 0)
        for (int w = 0; w < OT_THREADS / GEOT_WAVE; ++w) total += lds[w];
    return total;                    // (thread 0's)
}

__global__ __launch_bounds__(OT_THREADS) void ot_norm_kernel(const OtTable tab, int count, float *__restrict__ slots)
{
    __shared__ float lds[OT_THREADS / GEOT_WAVE];
    const int b = blockIdx.x, tid = threadIdx.x;
    const OtRec &r = tab.r[ot_find(tab, count, b)];
    const long long n = r.n, base = (long long)(b - r.first_block) * OT_BLOCK;
    const float *__restrict__ g = r.g;
    float acc = 0.f;
    if (r.flags & GEOT_OPTIM_TAIL_VECTOR) {
#pragma unroll
        for (int it = 0; it < OT_PER_THREAD / 4; ++it) {
            const long long e = base + ((long long)it * OT_THREADS + tid) * 4;
            if (e + 3 < n) {
                const float4 q = *reinterpret_cast<const float4 *>(g + e);
                acc += q.x * q.x;
                acc += q.y * q.y;
                acc += q.z * q.z;
                acc += q.w * q.w;
            } else {
                for (int k = 0; k < 4; ++k)
                    if (e + k < n) acc += g[e + k] * g[e + k];
            }
        }
    } else {
#pragma unroll 4
        for (int it = 0; it < OT_PER_THREAD; ++it) {
            const long long e = base + (long long)it * OT_THREADS + tid;
            if (e < n) acc += g[e] * g[e];
        }
    }
    const float total = ot_block_sum(acc, lds);
    if (tid == 0) slots[b] = total;
}

// scalars[0] = total_norm, scalars[1] = coef.  mode 0: leave the scalars alone (a further launch of step counters);
// 1: clip -- the slots in a fixed order in double; 2: no clip -- total_norm 0, coef 1.
__global__ __launch_bounds__(OT_THREADS) void ot_finish_kernel(const OtSteps st, int n_steps, int mode, long long n_slots,
                                                                const float *__restrict__ slots, float max_norm,
                                                                float *__restrict__ steps, float *__restrict__ scalars)
{
    __shared__ double lds[OT_THREADS];
    const int tid = threadIdx.x;
    for (int i = tid; i < n_steps; i += OT_THREADS) steps[st.idx[i]] += 1.0f;      // (distinct indices: one writer each)
    if (mode == 2 && tid == 0) {
        scalars[0] = 0.f;
        scalars[1] = 1.f;
    }
    if (mode != 1) return;
    double acc = 0.0;
    for (long long i = tid; i < n_slots; i += OT_THREADS) acc += (double)slots[i];
    lds[tid] = acc;
    __syncthreads();
    for (int half = OT_THREADS / 2; half > 0; half >>= 1) {
        if (tid < half) lds[tid] += lds[tid + half];
        __syncthreads();
    }
    if (tid == 0) {
        const float total = (float)sqrt(lds[0]);
        const float x = max_norm / (total + 1e-6f);
        scalars[0] = total;
        scalars[1] = x < 1.0f ? x : (x != x ? x : 1.0f);       // min(1, x) that lets a NaN through, as torch.clamp(max=1) does
    }
}

// ---- step_per_update > 1: the gated window ------------------------------------------------------------------------------------
struct OtSlotBase { int s[OT_CAP]; };                    // a record's first norm slot; -1: it is not part of the norm
static_assert(sizeof(OtTable) + sizeof(OtSlotBase) + 64 <= 4096, "kernel arguments fit 4 KB");

// acc = acc + g over the launch's records (g null: the record got no gradient in this call, its sum stands), and per workgroup
// of a clipped record the sum of the squares of the new values: ot_norm_kernel's partition, its order within a thread and
// within the workgroup, so that the slots hold what ot_norm_kernel gives for the summed gradient.
__global__ __launch_bounds__(OT_THREADS) void ot_acc_kernel(const OtTable tab, const OtSlotBase sb, int count,
                                                             float *__restrict__ acc, const long long *__restrict__ offs,
                                                             long long n_acc, float *__restrict__ slots)
{
    __shared__ float lds[OT_THREADS / GEOT_WAVE];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int at = ot_find(tab, count, b);
    const OtRec &r = tab.r[at];
    const long long n = r.n, base = (long long)(b - r.first_block) * OT_BLOCK;
    const long long off = offs[r.step];
    if (off < 0 || (off & 3) || off + n > n_acc) return;   // (uniform; the host builds the table: never taken)
    float *__restrict__ a = acc + off;
    const float *__restrict__ g = r.g;
    const bool add = g != nullptr;
    float sum = 0.f;
    if (r.flags & GEOT_OPTIM_TAIL_VECTOR) {
#pragma unroll
        for (int it = 0; it < OT_PER_THREAD / 4; ++it) {
            const long long e = base + ((long long)it * OT_THREADS + tid) * 4;
            if (e + 3 < n) {
                float4 q = *reinterpret_cast<float4 *>(a + e);
                if (add) {
                    const float4 gq = *reinterpret_cast<const float4 *>(g + e);
                    q.x = q.x + gq.x;
                    q.y = q.y + gq.y;
                    q.z = q.z + gq.z;
                    q.w = q.w + gq.w;
                    *reinterpret_cast<float4 *>(a + e) = q;
                }
                sum += q.x * q.x;
                sum += q.y * q.y;
                sum += q.z * q.z;
                sum += q.w * q.w;
            } else {
                for (int k = 0; k < 4; ++k) {
                    if (e + k < n) {
                        float x = a[e + k];
                        if (add) {
                            x = x + g[e + k];
                            a[e + k] = x;
                        }
                        sum += x * x;
                    }
                }
            }
        }
    } else {
#pragma unroll 4
        for (int it = 0; it < OT_PER_THREAD; ++it) {
            const long long e = base + (long long)it * OT_THREADS + tid;
            if (e < n) {
                float x = a[e];
                if (add) {
                    x = x + g[e];
                    a[e] = x;
                }
                sum += x * x;
            }
        }
    }
    const int s0 = sb.s[at];
    if (s0 < 0) return;                                  // (uniform)
    const float total = ot_block_sum(sum, lds);
    if (tid == 0) slots[s0 + (b - r.first_block)] = total;
}

// ot_finish_kernel behind the window counter.  gate[0]: calls of the open window, gate[1]: 1 when this call updates.  mode 1 / 2
// (the first launch of a call): the counter goes up; at k it returns to 0 and the flag is set, otherwise the flag is cleared
// and nothing else is written.  mode 0 (a further launch of step counters) follows the flag.
__global__ __launch_bounds__(OT_THREADS) void ot_acc_finish_kernel(const OtSteps st, int n_steps, int mode, long long n_slots,
                                                                    const float *__restrict__ slots, float max_norm,
                                                                    float *__restrict__ steps, float *__restrict__ scalars,
                                                                    int *__restrict__ gate, int k)
{
    __shared__ double lds[OT_THREADS];
    __shared__ int update;
    const int tid = threadIdx.x;
    if (tid == 0) {                                      // (the only thread that touches the gate)
        if (mode == 0) {
            update = gate[1];
        } else {
            const int w = gate[0] + 1;
            update = w >= k ? 1 : 0;
            gate[0] = update ? 0 : w;
            gate[1] = update;
        }
    }
    __syncthreads();
    if (!update) return;
    for (int i = tid; i < n_steps; i += OT_THREADS) steps[st.idx[i]] += 1.0f;
    if (mode == 2 && tid == 0) {
        scalars[0] = 0.f;
        scalars[1] = 1.f;
    }
    if (mode != 1) return;
    double acc = 0.0;
    for (long long i = tid; i < n_slots; i += OT_THREADS) acc += (double)slots[i];
    lds[tid] = acc;
    __syncthreads();
    for (int half = OT_THREADS / 2; half > 0; half >>= 1) {
        if (tid < half) lds[tid] += lds[tid + half];
        __syncthreads();
    }
    if (tid == 0) {
        const float total = (float)sqrt(lds[0]);
        const float x = max_norm / (total + 1e-6f);
        scalars[0] = total;
        scalars[1] = x < 1.0f ? x : (x != x ? x : 1.0f);
    }
}

struct OtConst {                     // what a record's elements share
    float coef, lrwd, omb1, b2, omb2, bc2_sqrt, eps, step_size, d, omd;
    bool teacher;
};

// One element, fp32, un-contracted, in this order:
//   g' = coef g                                   (clipped records; otherwise g' = g)
//   p1 = p - (lr wd) p
//   m' = m + (1 - b1) (g' - m)
//   v' = b2 v + ((1 - b2) g') g'
//   p' = p1 - ((lr / bc1) m') / (sqrt(v') / sqrt(bc2) + eps)
//   t' = d t + (1 - d) p'
// 1 - b1, 1 - b2, bc1 = 1 - b1^step, bc2 = 1 - b2^step, lr / bc1 and sqrt(bc2) are formed in double and rounded once.
__device__ inline void ot_adamw(float &p, float g, float &m, float &v, float &t, const OtConst &c, bool clipped)
{
    if (clipped) g = c.coef * g;
    const float p1 = p - c.lrwd * p;
    m = m + c.omb1 * (g - m);
    v = c.b2 * v + (c.omb2 * g) * g;
    const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
    p = p1 - (c.step_size * m) / denom;
    if (c.teacher) t = c.d * t + c.omd * p;
}

// The accumulator of a gated tail: a flat buffer, the record with step index s at acc[offs[s]...]; gate[0] is the window
// counter, gate[1] the flag "this call updates" the finish stage has just written.
struct OtAcc {
    float *acc;
    const long long *offs;
    long long n_acc;
    const int *gate;
};

// ACC: the gradient is the record's stretch of the accumulator, zeroed once it is read; nothing happens unless gate[1] is set.
template <bool ACC>
__device__ __forceinline__ void ot_update_body(const OtTable &tab, const OtGroups &groups, int count,
                                               const float *__restrict__ scalars, const float *__restrict__ steps,
                                               double decay, const OtAcc &ac)
{
    __shared__ float shared[2];
    if (ACC && ac.gate[1] == 0) return;                  // (uniform: a call inside a window)
    const int b = blockIdx.x, tid = threadIdx.x;
    const OtRec &r = tab.r[ot_find(tab, count, b)];
    const long long n = r.n, base = (long long)(b - r.first_block) * OT_BLOCK;
    const int flags = r.flags;
    if (flags & GEOT_OPTIM_TAIL_INT64) {                 // an integer buffer: the teacher's takes the student's value
        const long long *__restrict__ src = reinterpret_cast<const long long *>(r.p);
        long long *__restrict__ dst = reinterpret_cast<long long *>(r.t);
        for (int it = 0; it < OT_PER_THREAD; ++it) {
            const long long e = base + (long long)it * OT_THREADS + tid;
            if (e < n) dst[e] = src[e];
        }
        return;
    }
    OtConst c;
    c.d = (float)decay;
    c.omd = (float)(1.0 - decay);
    c.teacher = r.t != nullptr;
    const bool vec = flags & GEOT_OPTIM_TAIL_VECTOR;
    if (flags & GEOT_OPTIM_TAIL_EMA_ONLY) {              // a buffer, or a parameter without a gradient: t = d t + (1 - d) p
        const float *__restrict__ p = r.p;
        float *__restrict__ t = r.t;
        if (vec) {
#pragma unroll
            for (int it = 0; it < OT_PER_THREAD / 4; ++it) {
                const long long e = base + ((long long)it * OT_THREADS + tid) * 4;
                if (e + 3 < n) {
                    const float4 pq = *reinterpret_cast<const float4 *>(p + e);
                    float4 tq = *reinterpret_cast<float4 *>(t + e);
                    tq.x = c.d * tq.x + c.omd * pq.x;
                    tq.y = c.d * tq.y + c.omd * pq.y;
                    tq.z = c.d * tq.z + c.omd * pq.z;
                    tq.w = c.d * tq.w + c.omd * pq.w;
                    *reinterpret_cast<float4 *>(t + e) = tq;
                } else {
                    for (int k = 0; k < 4; ++k)
                        if (e + k < n) t[e + k] = c.d * t[e + k] + c.omd * p[e + k];
                }
            }
        } else {
            for (int it = 0; it < OT_PER_THREAD; ++it) {
                const long long e = base + (long long)it * OT_THREADS + tid;
                if (e < n) t[e] = c.d * t[e] + c.omd * p[e];
            }
        }
        return;
    }
    const OtGroup &gr = groups.g[r.group];
    if (tid == 0) {                                      // the two powers once per workgroup, in double
        const double step = (double)steps[r.step];
        const double lr = gr.lr_ptr ? (double)*gr.lr_ptr : (double)gr.lr;
        shared[0] = (float)(lr / (1.0 - pow(gr.beta1, step)));
        shared[1] = (float)sqrt(1.0 - pow(gr.beta2, step));
    }
    __syncthreads();
    const float lr = gr.lr_ptr ? *gr.lr_ptr : gr.lr;
    const bool clipped = flags & GEOT_OPTIM_TAIL_CLIPPED;
    c.coef = clipped ? scalars[1] : 1.0f;
    c.lrwd = lr * gr.weight_decay;
    c.omb1 = (float)(1.0 - gr.beta1);
    c.b2 = (float)gr.beta2;
    c.omb2 = (float)(1.0 - gr.beta2);
    c.eps = gr.eps;
    c.step_size = shared[0];
    c.bc2_sqrt = shared[1];
    float *__restrict__ p = r.p;
    // k = 1: read only (gradients are dropped right after the tail); ACC: the accumulator, read and zeroed by this thread
    float *ga = nullptr;
    if (ACC) {
        const long long off = ac.offs[r.step];
        if (off < 0 || (off & 3) || off + n > ac.n_acc) return;      // (uniform; the host builds the table: never taken)
        ga = ac.acc + off;
    }
    const float *__restrict__ g = ACC ? nullptr : r.g;
    float *__restrict__ m = r.m;
    float *__restrict__ v = r.v;
    float *t = r.t;
    if (vec) {
#pragma unroll
        for (int it = 0; it < OT_PER_THREAD / 4; ++it) {
            const long long e = base + ((long long)it * OT_THREADS + tid) * 4;
            if (e + 3 < n) {
                float4 pq = *reinterpret_cast<float4 *>(p + e);
                const float4 gq = *reinterpret_cast<const float4 *>((ACC ? ga : g) + e);
                float4 mq = *reinterpret_cast<float4 *>(m + e);
                float4 vq = *reinterpret_cast<float4 *>(v + e);
                float4 tq = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c.teacher) tq = *reinterpret_cast<float4 *>(t + e);
                ot_adamw(pq.x, gq.x, mq.x, vq.x, tq.x, c, clipped);
                ot_adamw(pq.y, gq.y, mq.y, vq.y, tq.y, c, clipped);
                ot_adamw(pq.z, gq.z, mq.z, vq.z, tq.z, c, clipped);
                ot_adamw(pq.w, gq.w, mq.w, vq.w, tq.w, c, clipped);
                *reinterpret_cast<float4 *>(p + e) = pq;
                *reinterpret_cast<float4 *>(m + e) = mq;
                *reinterpret_cast<float4 *>(v + e) = vq;
                if (c.teacher) *reinterpret_cast<float4 *>(t + e) = tq;
                if (ACC) *reinterpret_cast<float4 *>(ga + e) = make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                for (int k = 0; k < 4; ++k) {
                    if (e + k < n) {
                        float tt = c.teacher ? t[e + k] : 0.f;
                        ot_adamw(p[e + k], ACC ? ga[e + k] : g[e + k], m[e + k], v[e + k], tt, c, clipped);
                        if (c.teacher) t[e + k] = tt;
                        if (ACC) ga[e + k] = 0.f;
                    }
                }
            }
        }
    } else {
        for (int it = 0; it < OT_PER_THREAD; ++it) {
            const long long e = base + (long long)it * OT_THREADS + tid;
            if (e < n) {
                float tt = c.teacher ? t[e] : 0.f;
                ot_adamw(p[e], ACC ? ga[e] : g[e], m[e], v[e], tt, c, clipped);
                if (c.teacher) t[e] = tt;
                if (ACC) ga[e] = 0.f;
            }
        }
    }
}

__global__ __launch_bounds__(OT_THREADS) void ot_update_kernel(const OtTable tab, const OtGroups groups, int count,
                                                                const float *__restrict__ scalars,
                                                                const float *__restrict__ steps, double decay)
{
    ot_update_body<false>(tab, groups, count, scalars, steps, decay, OtAcc{});
}

__global__ __launch_bounds__(OT_THREADS) void ot_acc_update_kernel(const OtTable tab, const OtGroups groups, int count,
                                                                    const float *__restrict__ scalars,
                                                                    const float *__restrict__ steps, double decay, const OtAcc ac)
{
    ot_update_body<true>(tab, groups, count, scalars, steps, decay, ac);
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static inline bool ot_aligned16(const void *q) { return q == nullptr || (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }

// The table as the launches take it: checked, with the plan's paths set.  false: a record is malformed.
static bool ot_prepare(int t, const void *records_host, int n_groups, int n_steps, std::vector<OtRec> &recs, OtPlan &plan,
                       bool need_g = true)
{
    if (t < 0 || (t > 0 && !records_host)) return false;
    const OtRec *host = static_cast<const OtRec *>(records_host);
    recs.assign(host, host + t);
    std::vector<long long> counts((size_t)t);
    std::vector<int> aligned((size_t)t), flags((size_t)t);
    for (int i = 0; i < t; ++i) {
        const OtRec &r = recs[(size_t)i];
        if (r.n < 0) return false;
        const bool held = r.n > 0;                       // (an empty tensor has no address)
        if (r.flags & (GEOT_OPTIM_TAIL_EMA_ONLY | GEOT_OPTIM_TAIL_INT64)) {
            if (held && (!r.p || !r.t)) return false;
        } else if ((held && (!r.p || (need_g && !r.g) || !r.m || !r.v)) || r.group < 0 || r.group >= n_groups || r.step < 0 ||
                   r.step >= n_steps) {
            return false;
        }
        counts[(size_t)i] = r.n;
        flags[(size_t)i] = r.flags;
        aligned[(size_t)i] = ot_aligned16(r.p) && ot_aligned16(r.g) && ot_aligned16(r.m) && ot_aligned16(r.v) && ot_aligned16(r.t);
    }
    if (!ot_plan(t, counts.data(), aligned.data(), flags.data(), plan)) return false;
    for (int i = 0; i < t; ++i)
        recs[(size_t)i].flags = (recs[(size_t)i].flags & ~GEOT_OPTIM_TAIL_VECTOR) | (plan.vec[(size_t)i] ? GEOT_OPTIM_TAIL_VECTOR : 0);
    return true;
}

// Launches of at most OT_CAP of the chosen records each; issue(table, count, blocks, first slot of the launch).
template <class Issue>
static int ot_sweep(const std::vector<OtRec> &recs, const OtPlan &plan, bool norm_only, Issue issue)
{
    OtTable tab;
    int count = 0;
    long long blocks = 0, slot0 = 0;
    auto flush = [&]() -> int {
        if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
        if (blocks > 0) issue(tab, count, (int)blocks, slot0);
        slot0 += blocks;
        count = 0;
        blocks = 0;
        return hipSuccess;
    };
    for (size_t i = 0; i < recs.size(); ++i) {
        if (norm_only && !ot_in_norm(recs[i].flags)) continue;
        tab.r[count] = recs[i];
        tab.r[count].first_block = (int)blocks;
        blocks += plan.blocks[i];
        if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
        const bool chunk_end = norm_only ? count + 1 == OT_CAP : (i % OT_CAP == OT_CAP - 1);
        ++count;
        if (chunk_end)
            if (int err = flush()) return err;
    }
    return flush();
}

} // namespace geot

using namespace geot;

GEOT_EXPORT int geot_optim_tail_plan(int t, const long long *counts, const int *aligned, const int *flags, long long *out,
                                     int n_out)
{
    if (t < 0 || !out || n_out < 4 + 2 * (long long)t || (t > 0 && (!counts || !aligned || !flags))) return 0;
    OtPlan plan;
    if (!ot_plan(t, counts, aligned, flags, plan)) return 0;
    out[0] = plan.update_launches;
    out[1] = plan.norm_launches;
    out[2] = plan.update_blocks;
    out[3] = plan.slots;
    for (int i = 0; i < t; ++i) {
        out[4 + i] = plan.blocks[(size_t)i];
        out[4 + t + i] = plan.vec[(size_t)i];
    }
    return 1;
}

GEOT_EXPORT int geot_optim_tail_norm(int t, const void *records_host, float *slots, long long n_slots, void *stream)
{
    std::vector<OtRec> recs;
    OtPlan plan;
    if (!ot_prepare(t, records_host, GEOT_OPTIM_TAIL_MAX_GROUPS, 0x7fffffff, recs, plan)) return hipErrorInvalidValue;
    if (plan.slots > n_slots || (plan.slots > 0 && !slots)) return hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const int err = ot_sweep(recs, plan, true, [&](const OtTable &tab, int count, int blocks, long long slot0) {
        hipLaunchKernelGGL(ot_norm_kernel, dim3(blocks), dim3(OT_THREADS), 0, s, tab, count, slots + slot0);
    });
    return err ? err : hipGetLastError();
}

GEOT_EXPORT int geot_optim_tail_finish(int t, const void *records_host, int clip, long long n_slots, const float *slots,
                                       float max_norm, float *steps, int n_steps, float *scalars, void *stream)
{
    if (t < 0 || (t > 0 && !records_host) || !scalars || n_steps < 0 || n_slots < 0) return hipErrorInvalidValue;
    if (clip && n_slots > 0 && !slots) return hipErrorInvalidValue;
    const OtRec *host = static_cast<const OtRec *>(records_host);
    std::vector<int> idx;
    std::vector<bool> seen((size_t)n_steps, false);
    for (int i = 0; i < t; ++i) {
        if (!ot_adamw_record(host[i].flags)) continue;
        const int k = host[i].step;
        if (!steps || k < 0 || k >= n_steps || seen[(size_t)k]) return hipErrorInvalidValue;      // one writer per counter
        seen[(size_t)k] = true;
        idx.push_back(k);
    }
    hipStream_t s = (hipStream_t)stream;
    size_t at = 0;
    int mode = clip ? 1 : 2;
    do {
        OtSteps st;
        const int cnt = (int)((idx.size() - at < (size_t)OT_STEP_CAP) ? idx.size() - at : (size_t)OT_STEP_CAP);
        for (int i = 0; i < cnt; ++i) st.idx[i] = idx[at + (size_t)i];
        hipLaunchKernelGGL(ot_finish_kernel, dim3(1), dim3(OT_THREADS), 0, s, st, cnt, mode, n_slots, slots, max_norm, steps,
                           scalars);
        at += (size_t)cnt;
        mode = 0;
    } while (at < idx.size());
    return hipGetLastError();
}

GEOT_EXPORT int geot_optim_tail_update(int t, const void *records_host, int n_groups, const void *groups_host,
                                       const float *scalars, const float *steps, int n_steps, double ema_decay, void *stream)
{
    if (n_groups < 0 || n_groups > GEOT_OPTIM_TAIL_MAX_GROUPS || (n_groups > 0 && !groups_host) || !scalars) return hipErrorInvalidValue;
    if (!(ema_decay >= 0.0 && ema_decay < 1.0)) return hipErrorInvalidValue;
    std::vector<OtRec> recs;
    OtPlan plan;
    if (!ot_prepare(t, records_host, n_groups, n_steps, recs, plan)) return hipErrorInvalidValue;
    for (const OtRec &r : recs)
        if (ot_adamw_record(r.flags) && !steps) return hipErrorInvalidValue;
    OtGroups groups = {};
    for (int i = 0; i < n_groups; ++i) groups.g[i] = static_cast<const OtGroup *>(groups_host)[i];
    hipStream_t s = (hipStream_t)stream;
    const int err = ot_sweep(recs, plan, false, [&](const OtTable &tab, int count, int blocks, long long) {
        hipLaunchKernelGGL(ot_update_kernel, dim3(blocks), dim3(OT_THREADS), 0, s, tab, groups, count, scalars, steps, ema_decay);
    });
    return err ? err : hipGetLastError();
}

// ---- step_per_update > 1 ---------------------------------------------------------------------------------------------------
namespace geot {

// The launches of the gated tail for these records.  The accumulate sweep takes the records that are neither EMA-only nor
// integer, OT_CAP per launch in table order (a launch without an element is not issued); the gated update sweep is ot_plan's
// update sweep; the finish stage takes one launch per OT_STEP_CAP of the accumulate sweep's records, and at least one.
struct OtAccPlan {
    long long acc_launches = 0, acc_blocks = 0, finish_launches = 1;
};

static void ot_acc_plan(int t, const int *flags, const OtPlan &plan, OtAccPlan &ap)
{
    long long in_launch = 0, records = 0;
    for (int i = 0; i < t; ++i) {
        if (!ot_adamw_record(flags[i])) continue;
        ap.acc_blocks += plan.blocks[(size_t)i];
        in_launch += plan.blocks[(size_t)i];
        if (++records % OT_CAP == 0) {
            ap.acc_launches += in_launch > 0;
            in_launch = 0;
        }
    }
    ap.acc_launches += in_launch > 0;
    ap.finish_launches = records > OT_STEP_CAP ? (records + OT_STEP_CAP - 1) / OT_STEP_CAP : 1;
}

} // namespace geot

GEOT_EXPORT int geot_optim_tail_acc_plan(int t, const long long *counts, const int *aligned, const int *flags, long long *out,
                                         int n_out)
{
    if (t < 0 || !out || n_out < 6 || (t > 0 && (!counts || !aligned || !flags))) return 0;
    OtPlan plan;
    if (!ot_plan(t, counts, aligned, flags, plan)) return 0;
    OtAccPlan ap;
    ot_acc_plan(t, flags, plan, ap);
    out[0] = ap.acc_launches;
    out[1] = ap.finish_launches;
    out[2] = plan.update_launches;
    out[3] = ap.acc_blocks;
    out[4] = plan.update_blocks;
    out[5] = plan.slots;
    return 1;
}

GEOT_EXPORT int geot_optim_tail_accumulate(int t, const void *records_host, float *acc, const long long *acc_offsets,
                                           long long n_acc, int n_steps, float *slots, long long n_slots, void *stream)
{
    if (!acc || !acc_offsets || n_acc < 0 || n_steps < 0 || n_slots < 0) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(acc) & 15u) return hipErrorInvalidValue;
    std::vector<OtRec> recs;
    OtPlan plan;
    if (!ot_prepare(t, records_host, GEOT_OPTIM_TAIL_MAX_GROUPS, n_steps, recs, plan, false)) return hipErrorInvalidValue;
    if (plan.slots > n_slots || (plan.slots > 0 && !slots) || plan.slots > 0x7fffffffLL) return hipErrorInvalidValue;
    std::vector<int> flags((size_t)t);
    for (int i = 0; i < t; ++i) {
        flags[(size_t)i] = recs[(size_t)i].flags;
        if (ot_adamw_record(recs[(size_t)i].flags) && recs[(size_t)i].n > n_acc) return hipErrorInvalidValue;
    }
    OtAccPlan ap;
    ot_acc_plan(t, flags.data(), plan, ap);
    if (ap.acc_blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    OtTable tab;
    OtSlotBase sb;
    int count = 0;
    long long blocks = 0, slot = 0, issued = 0;
    auto flush = [&]() {
        if (blocks > 0) {
            hipLaunchKernelGGL(ot_acc_kernel, dim3((unsigned)blocks), dim3(OT_THREADS), 0, s, tab, sb, count, acc, acc_offsets,
                               n_acc, slots);
            ++issued;
        }
        count = 0;
        blocks = 0;
    };
    for (int i = 0; i < t; ++i) {
        const OtRec &r = recs[(size_t)i];
        if (!ot_adamw_record(r.flags)) continue;
        tab.r[count] = r;
        tab.r[count].first_block = (int)blocks;
        sb.s[count] = ot_in_norm(r.flags) ? (int)slot : -1;
        if (ot_in_norm(r.flags)) slot += plan.blocks[(size_t)i];
        blocks += plan.blocks[(size_t)i];
        if (++count == OT_CAP) flush();
    }
    flush();
    if (issued != ap.acc_launches) return hipErrorUnknown;      // (the plan and the sweep are one rule)
    return hipGetLastError();
}

GEOT_EXPORT int geot_optim_tail_acc_finish(int t, const void *records_host, int clip, long long n_slots, const float *slots,
                                           float max_norm, float *steps, int n_steps, float *scalars, int *gate, int k,
                                           void *stream)
{
    if (t < 0 || (t > 0 && !records_host) || !scalars || !gate || k < 1 || n_steps < 0 || n_slots < 0) return hipErrorInvalidValue;
    if (clip && n_slots > 0 && !slots) return hipErrorInvalidValue;
    const OtRec *host = static_cast<const OtRec *>(records_host);
    std::vector<int> idx;
    std::vector<bool> seen((size_t)n_steps, false);
    for (int i = 0; i < t; ++i) {
        if (!ot_adamw_record(host[i].flags)) continue;
        const int c = host[i].step;
        if (!steps || c < 0 || c >= n_steps || seen[(size_t)c]) return hipErrorInvalidValue;      // one writer per counter
        seen[(size_t)c] = true;
        idx.push_back(c);
    }
    hipStream_t s = (hipStream_t)stream;
    size_t at = 0;
    int mode = clip ? 1 : 2;
    do {
        OtSteps st;
        const int cnt = (int)((idx.size() - at < (size_t)OT_STEP_CAP) ? idx.size() - at : (size_t)OT_STEP_CAP);
        for (int i = 0; i < cnt; ++i) st.idx[i] = idx[at + (size_t)i];
        hipLaunchKernelGGL(ot_acc_finish_kernel, dim3(1), dim3(OT_THREADS), 0, s, st, cnt, mode, n_slots, slots, max_norm,
                           steps, scalars, gate, k);
        at += (size_t)cnt;
        mode = 0;
    } while (at < idx.size());
    return hipGetLastError();
}

GEOT_EXPORT int geot_optim_tail_acc_update(int t, const void *records_host, int n_groups, const void *groups_host,
                                           const float *scalars, const float *steps, int n_steps, double ema_decay, float *acc,
                                           const long long *acc_offsets, long long n_acc, const int *gate, void *stream)
{
    if (n_groups < 0 || n_groups > GEOT_OPTIM_TAIL_MAX_GROUPS || (n_groups > 0 && !groups_host) || !scalars) return hipErrorInvalidValue;
    if (!(ema_decay >= 0.0 && ema_decay < 1.0)) return hipErrorInvalidValue;
    if (!acc || !acc_offsets || n_acc < 0 || !gate || (reinterpret_cast<uintptr_t>(acc) & 15u)) return hipErrorInvalidValue;
    std::vector<OtRec> recs;
    OtPlan plan;
    if (!ot_prepare(t, records_host, n_groups, n_steps, recs, plan, false)) return hipErrorInvalidValue;
    for (const OtRec &r : recs)
        if (ot_adamw_record(r.flags) && (!steps || r.n > n_acc)) return hipErrorInvalidValue;
    OtGroups groups = {};
    for (int i = 0; i < n_groups; ++i) groups.g[i] = static_cast<const OtGroup *>(groups_host)[i];
    const OtAcc ac = {acc, acc_offsets, n_acc, gate};
    hipStream_t s = (hipStream_t)stream;
    const int err = ot_sweep(recs, plan, false, [&](const OtTable &tab, int count, int blocks, long long) {
        hipLaunchKernelGGL(ot_acc_update_kernel, dim3(blocks), dim3(OT_THREADS), 0, s, tab, groups, count, scalars, steps,
                           ema_decay, ac);
    });
    return err ? err : hipGetLastError();
}
