// max_conv.hip -- the backward of  out = max over a group's n points of (W x)  without the dense gradient of W x.
//
// The patch encoder (Encoder._forward_channels_first) runs two 1x1 convolutions y = W x, W (Co, Ci), x (Ci, L = G n), whose
// output feeds nothing but the max over every group's n columns.  The gradient of y then has ONE non-zero per (output
// channel, group): dout (Co, G) at column arg (Co, G).  Written out dense it is 31/32 zeros at n = 32, and the two library
// GEMMs behind it (W^T dy, dy x^T) multiply those zeros.  The two kernels here take the sparse form as it is:
//
//   dgrad   dx[c, g n + j] = sum over the o with arg[o, g] == j of dout[o, g] W[o, c]      (ascending o, fmaf)
//   wgrad   dW[o, c]       = sum over g of dout[o, g] x[c, g n + arg[o, g]]                (ascending g inside a chunk of
//                            groups in fp32 fmaf, the chunks added in ascending order in fp64, rounded once)
//
// No float atomics, no memset / memcpy, nothing read from dx or ws: the same bits on every call and on every device (the
// launch geometry is a function of the shapes alone).
#include "geot_common.h"
#include "geot_hip.h"

using namespace geot;

// ---- dgrad ----------------------------------------------------------------------------------------------------------
// A workgroup of 8 waves keeps a slab of cs input channels of W in LDS, (Co, cs + 4) floats, and walks a run of consecutive
// groups, 8 at a time: their dout / arg columns are staged as (Co, 8) tiles (the columns of one group are G elements apart
// in memory: fetched per group they would cost a cache line per element).  Then every wave takes one group:
//   1. mask[j][o / 32] |= 1 << (o % 32) for the group's Co channels (integer LDS atomics: the result has no order);
//   2. bstart = exclusive scan of the masks' bit counts over the slots j;
//   3. channel o goes to position bstart[j] + (set bits of mask[j] below o): a counting sort by slot, stable in o, as
//      (o, dout) pairs;
//   4. a lane owns 4 input channels and 4 slots: it adds its four lists, 4 fmaf per (pair, W float4) read, and stores the
//      four float4s -- the lanes of one channel row cover the group's n floats, 128 contiguous bytes at n = 32, and the
//      next group continues the row.  Slots no channel selected keep their initial +0.
constexpr int MD_THREADS = 512;
constexpr int MD_WAVES = MD_THREADS / 64;
constexpr int MD_R = 8;                     // groups staged per step
constexpr int MD_LDS_MAX = 160 * 1024;

struct MdPlan {
    int cs, run, nact;
    size_t lds;
};
// slab width, groups per workgroup and the number of waves that take groups, from the shapes alone
static inline bool md_plan(int co, int ci, int g, int n, MdPlan *p)
{
    int cs = co <= 256 ? 32 : (co <= 512 ? 16 : 8);
    while (cs > 4 && cs / 2 >= ci) cs /= 2;
    const int cw = (co + 31) >> 5;
    const size_t fixed = (size_t)co * (cs + 4) * 4 + (size_t)co * MD_R * 4 + (size_t)co * MD_R;
    const size_t per_wave = (size_t)co * 8 + (size_t)n * cw * 4 + (size_t)((n + 2) & ~1) * 4;
    if (fixed + per_wave > (size_t)MD_LDS_MAX) return false;
    size_t nact = ((size_t)MD_LDS_MAX - fixed) / per_wave;
    if (nact > MD_WAVES) nact = MD_WAVES;
    const int slabs = (ci + cs - 1) / cs;
    int run = 64;
    while (run > MD_R && (long long)slabs * ((g + run - 1) / run) < 1024) run >>= 1;
    p->cs = cs;
    p->run = run;
    p->nact = (int)nact;
    p->lds = fixed + nact * per_wave;
    return true;
}

__global__ __launch_bounds__(MD_THREADS) void maxconv_dgrad_kernel(int co, int ci, int G, int n, int cs, int run, int nact,
                                                                   const float *__restrict__ W, const float *__restrict__ dout,
                                                                   const uint8_t *__restrict__ arg, float *__restrict__ dx)
{
    extern __shared__ __align__(16) unsigned char md_smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wst = cs + 4, cq = cs >> 2, cw = (co + 31) >> 5;
    float *Wl = reinterpret_cast<float *>(md_smem);                         // (co, cs + 4)
    float *dt = Wl + (size_t)co * wst;                                      // (co, MD_R)
    uint8_t *at = reinterpret_cast<uint8_t *>(dt + (size_t)co * MD_R);      // (co, MD_R)
    const size_t per_wave = (size_t)co * 8 + (size_t)n * cw * 4 + (size_t)((n + 2) & ~1) * 4;
    unsigned char *mine = at + (size_t)co * MD_R + (size_t)(wave < nact ? wave : 0) * per_wave;
    int2 *list = reinterpret_cast<int2 *>(mine);                            // co (o, dout bits) pairs, sorted by slot
    uint32_t *mask = reinterpret_cast<uint32_t *>(list + co);               // (n, cw)
    int *bstart = reinterpret_cast<int *>(mask + (size_t)n * cw);           // n + 1

    const int c0 = blockIdx.x * cs;
    const int g0 = blockIdx.y * run;
    const int gend = min(G, g0 + run);
    const long long L = (long long)G * n;

    for (int idx = tid; idx < co * cq; idx += MD_THREADS) {
        const int o = idx / cq, q4 = idx - o * cq;
        const int c = c0 + 4 * q4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < ci) v = *reinterpret_cast<const float4 *>(W + (size_t)o * ci + c);
        *reinterpret_cast<float4 *>(Wl + (size_t)o * wst + 4 * q4) = v;
    }
    const int cqi = lane % cq, tq = lane / cq, tqn = 64 / cq;
    const bool c_live = c0 + 4 * cqi < ci;

    for (int gs = g0; gs < gend; gs += MD_R) {
        __syncthreads();                                         // the tiles' readers of the step before are through
        for (int idx = tid; idx < co * MD_R; idx += MD_THREADS) {
            const int o = idx / MD_R, gl = idx % MD_R;
            if (gs + gl < gend) {
                dt[idx] = dout[(long long)o * G + gs + gl];
                at[idx] = arg[(long long)o * G + gs + gl];
            }
        }
        for (int pass = 0; pass * nact < MD_R; ++pass) {
            const int gl = pass * nact + wave;
            const int g = gs + gl;
            const bool active = wave < nact && gl < MD_R && g < gend;
            if (active)
                for (int i = lane; i < n * cw; i += 64) mask[i] = 0u;
            __syncthreads();
            if (active)
                for (int o = lane; o < co; o += 64) {
                    const int a = at[o * MD_R + gl];
                    if (a < n) atomicOr(&mask[a * cw + (o >> 5)], 1u << (o & 31));
                }
            __syncthreads();
            if (active) {
                int carry = 0;
                for (int jb = 0; jb < n; jb += 64) {
                    const int j = jb + lane;
                    int cnt = 0;
                    if (j < n)
                        for (int k = 0; k < cw; ++k) cnt += __popc(mask[j * cw + k]);
                    int inc = cnt;
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const int t = __shfl_up(inc, d);
                        if (lane >= d) inc += t;
                    }
                    if (j < n) bstart[j] = carry + inc - cnt;
                    carry += __shfl(inc, 63);
                }
                if (lane == 0) bstart[n] = carry;
            }
            __syncthreads();
            if (active)
                for (int o = lane; o < co; o += 64) {
                    const int a = at[o * MD_R + gl];
                    if (a < n) {
                        const uint32_t *m = mask + a * cw;
                        int pos = bstart[a] + __popc(m[o >> 5] & ((1u << (o & 31)) - 1u));
                        for (int k = 0; k < (o >> 5); ++k) pos += __popc(m[k]);
                        list[pos] = make_int2(o, __float_as_int(dt[o * MD_R + gl]));
                    }
                }
            __syncthreads();
            if (active && c_live)
                for (int q = tq; q < (n >> 2); q += tqn) {
                    float acc[4][4];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[u][i] = 0.f;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int pe = bstart[4 * q + u + 1];
                        for (int p = bstart[4 * q + u]; p < pe; ++p) {
                            const int2 ent = list[p];
                            const float d = __int_as_float(ent.y);
                            const float4 w = *reinterpret_cast<const float4 *>(Wl + (size_t)ent.x * wst + 4 * cqi);
                            acc[u][0] = fmaf(d, w.x, acc[u][0]);
                            acc[u][1] = fmaf(d, w.y, acc[u][1]);
                            acc[u][2] = fmaf(d, w.z, acc[u][2]);
                            acc[u][3] = fmaf(d, w.w, acc[u][3]);
                        }
                    }
                    float *dst = dx + (long long)(c0 + 4 * cqi) * L + (long long)g * n + 4 * q;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        *reinterpret_cast<float4 *>(dst + i * L) = make_float4(acc[0][i], acc[1][i], acc[2][i], acc[3][i]);
                }
        }
    }
}

// ---- wgrad ----------------------------------------------------------------------------------------------------------
// A workgroup of 16 waves owns 256 output channels x a slab of 128 input channels x one chunk of groups, its (256, 128)
// sums in registers: a wave 16 output channels, a lane the input channels lane and lane + 64 of the slab.  x is therefore
// read once per 256 output channels, the small dout / arg once per slab.  The chunk's groups stream through LDS up to 4 at
// a time, slot-major: xt[(group, slot)][channel], rows of 129 floats, so the 32 lanes of a half-wave (one slot, consecutive
// channels) read 32 banks and the fill (8 float4s of 4 channel rows per half-wave) writes 32 banks.  A wave's (slot, dout)
// pairs of a step sit one per lane (16 channels x 4 groups) and are broadcast with v_readlane: the inner step is one
// address add, two LDS reads and two fmaf.  Partial sums go to ws (chunks, Co, Ci); the finish kernel adds the chunks.
constexpr int MW_THREADS = 1024;
constexpr int MW_OPW = 16;                  // output channels per wave
constexpr int MW_OBLK = 16 * MW_OPW;        // per workgroup
constexpr int MW_CS = 128;                  // input channels per workgroup
constexpr int MW_S = MW_CS + 1;             // LDS row stride (floats)
constexpr int MW_GT = 4;                    // groups per step at most

static inline int mw_step_groups(int n)
{
    int gt = 128 / n;
    return gt < 1 ? 1 : (gt > MW_GT ? MW_GT : gt);
}
// The chunks of groups, from g alone: 32 groups each up to 2048 groups (a few dozen groups already make several chunks, the
// last one ragged), 64 balanced chunks beyond (the workload's 4096 groups: 64 each; ws stays at 64 Co Ci floats).  The count
// never falls as g grows.  GEOT_MAXCONV_CHUNK=<groups> (read on every call) pins the chunk size: tests reach the one-group
// and other odd chunks with it.  size == 0: chunk k is groups [k g / count, (k + 1) g / count).
struct MwChunks {
    int count, size;
};
static inline MwChunks mw_chunks(int g)
{
    if (const char *e = getenv("GEOT_MAXCONV_CHUNK"))
        if (atoi(e) > 0) return {(g + atoi(e) - 1) / atoi(e), atoi(e)};
    if (g <= 2048) return {(g + 31) / 32, 32};
    return {64, 0};
}

__global__ __launch_bounds__(MW_THREADS) void maxconv_wgrad_kernel(int co, int ci, int G, int n, int chunk, int gt,
                                                                   const float *__restrict__ x, const float *__restrict__ dout,
                                                                   const uint8_t *__restrict__ arg, float *__restrict__ ws)
{
    extern __shared__ __align__(16) float mw_xt[];               // (gt n, MW_S)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c0 = blockIdx.x * MW_CS;
    const int ob = blockIdx.z * MW_OBLK + wave * MW_OPW;
    const int g_begin = chunk > 0 ? (int)blockIdx.y * chunk : (int)((long long)blockIdx.y * G / gridDim.y);
    const int g_end = chunk > 0 ? min(G, g_begin + chunk) : (int)((long long)(blockIdx.y + 1) * G / gridDim.y);
    const long long L = (long long)G * n;

    float acc[MW_OPW][2];
#pragma unroll
    for (int i = 0; i < MW_OPW; ++i) acc[i][0] = acc[i][1] = 0.f;

    for (int g = g_begin; g < g_end; g += gt) {
        const int cnt = min(gt, g_end - g);
        int jv = 0;
        float dv = 0.f;
        {
            const int o = ob + (lane & 15), gl = lane >> 4;
            if (o < co && gl < cnt) {
                jv = min((int)arg[(long long)o * G + g + gl], n - 1);
                dv = dout[(long long)o * G + g + gl];
            }
        }
        __syncthreads();                                         // the step before has read its tile
        const int quads = cnt * n >> 2;                          // float4s of a channel row in this step
        const int total = MW_CS * 8 * ((quads + 7) >> 3);
#pragma unroll 4
        for (int idx = tid; idx < total; idx += MW_THREADS) {
            const int f4 = (idx & 7) + 8 * (idx / (8 * MW_CS));
            const int cc = (idx >> 3) & (MW_CS - 1);
            if (f4 < quads) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c0 + cc < ci) v = *reinterpret_cast<const float4 *>(x + (long long)(c0 + cc) * L + (long long)g * n + 4 * f4);
                float *d = mw_xt + (size_t)(4 * f4) * MW_S + cc;
                d[0] = v.x;
                d[MW_S] = v.y;
                d[2 * MW_S] = v.z;
                d[3 * MW_S] = v.w;
            }
        }
        __syncthreads();
        if (ob < co) {
#pragma unroll
            for (int gl = 0; gl < MW_GT; ++gl) {
                if (gl < cnt) {
#pragma unroll
                    for (int i = 0; i < MW_OPW; ++i) {
                        const int j = __builtin_amdgcn_readlane(jv, gl * 16 + i);
                        const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dv), gl * 16 + i));
                        const float *p = mw_xt + (size_t)(gl * n + j) * MW_S + lane;
                        acc[i][0] = fmaf(d, p[0], acc[i][0]);
                        acc[i][1] = fmaf(d, p[64], acc[i][1]);
                    }
                }
            }
        }
    }
    const int c = c0 + lane;
#pragma unroll
    for (int i = 0; i < MW_OPW; ++i) {
        const int o = ob + i;
        if (o < co) {
            float *dst = ws + ((size_t)blockIdx.y * co + o) * ci + c;
            if (c < ci) dst[0] = acc[i][0];
            if (c + 64 < ci) dst[64] = acc[i][1];
        }
    }
}

// dW = the chunks' partial sums added in ascending chunk order in fp64, rounded once
__global__ __launch_bounds__(256) void maxconv_wgrad_finish_kernel(int quads, int chunks, const float4 *__restrict__ ws,
                                                                   float4 *__restrict__ dW)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= quads) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int k = 0; k < chunks; ++k) {
        const float4 v = ws[(size_t)k * quads + e];
        s0 += (double)v.x;
        s1 += (double)v.y;
        s2 += (double)v.z;
        s3 += (double)v.w;
    }
    dW[e] = make_float4((float)s0, (float)s1, (float)s2, (float)s3);
}

// ---- entry points -----------------------------------------------------------------------------------------------------
static inline bool maxconv_shape_ok(int co, int ci, int g, int n)
{
    return co >= 1 && co <= 1024 && ci >= 4 && (ci & 3) == 0 && g >= 1 && n >= 4 && n <= 256 && (n & 3) == 0
           && (long long)g * n <= 0x7fffffffLL && (long long)co * g <= 0x7fffffffLL;
}
static inline bool aligned16(const void *p) { return p && (((uintptr_t)p) & 15) == 0; }

GEOT_EXPORT int geot_maxconv_dgrad(int co, int ci, int g, int n, const float *W, const float *dout, const unsigned char *arg,
                                   float *dx, void *stream)
{
    MdPlan p;
    if (!maxconv_shape_ok(co, ci, g, n) || !aligned16(W) || !aligned16(dx) || !dout || !arg) return hipErrorNotSupported;
    if (!md_plan(co, ci, g, n, &p)) return hipErrorNotSupported;
    const long long gy = (g + p.run - 1) / p.run;
    if (gy > 65535) return hipErrorNotSupported;
    hipError_t e = allow_big_lds((const void *)maxconv_dgrad_kernel, p.lds, MD_LDS_MAX);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(maxconv_dgrad_kernel, dim3((unsigned)((ci + p.cs - 1) / p.cs), (unsigned)gy), dim3(MD_THREADS), p.lds,
                       (hipStream_t)stream, co, ci, g, n, p.cs, p.run, p.nact, W, dout, arg, dx);
    return hipGetLastError();
}

GEOT_EXPORT long long geot_maxconv_ws_floats(int co, int ci, int g, int n)
{
    if (!maxconv_shape_ok(co, ci, g, n)) return -1;
    return (long long)mw_chunks(g).count * co * ci;
}

GEOT_EXPORT int geot_maxconv_wgrad(int co, int ci, int g, int n, const float *x, const float *dout, const unsigned char *arg,
                                   float *ws, float *dW, void *stream)
{
    if (!maxconv_shape_ok(co, ci, g, n) || !aligned16(x) || !aligned16(ws) || !aligned16(dW) || !dout || !arg)
        return hipErrorNotSupported;
    const MwChunks ch = mw_chunks(g);
    const int chunk = ch.size, chunks = ch.count;
    if (chunks > 65535) return hipErrorNotSupported;
    const int gt = mw_step_groups(n);
    const size_t lds = (size_t)gt * n * MW_S * sizeof(float);
    hipError_t e = allow_big_lds((const void *)maxconv_wgrad_kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(maxconv_wgrad_kernel, dim3((unsigned)((ci + MW_CS - 1) / MW_CS), (unsigned)chunks, (unsigned)((co + MW_OBLK - 1) / MW_OBLK)),
                       dim3(MW_THREADS), lds, (hipStream_t)stream, co, ci, g, n, chunk, gt, x, dout, arg, ws);
    const int quads = co * ci / 4;
    hipLaunchKernelGGL(maxconv_wgrad_finish_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, quads,
                       chunks, (const float4 *)ws, (float4 *)dW);
    return hipGetLastError();
}
