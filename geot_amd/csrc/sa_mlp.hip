// sa_mlp.hip -- fused SetAbstraction body for gfx950 (MI355X):
//   neighbourhood gather + centre subtraction + concat + shared MLP (1x1 conv stack with
//   folded BatchNorm + ReLU) + max over nsample, in one kernel.
//
// Replaces the reference chain (behaviour, not code)
//   QueryAndGroup.forward        pointnet2/pointnet2_utils.py:343-358  (2x grouping_operation, cat)
//   SharedMLP                    pointnet2/pytorch_utils.py:8-33       (Conv2d 1x1 + BN + ReLU)
//   F.max_pool2d over nsample    pointnet2/pointnet2_modules.py:360-363
// which materialises (B, 3+C, npoint, nsample) and every (B, C_l, npoint, nsample)
// activation in HBM.  Here the only HBM traffic is the gathered inputs and the
// (B, C_out, npoint) result; this is the one genuinely dense contraction on the hot
// path, so it runs on the matrix cores: v_mfma_f32_32x32x2_f32 (exact fp32, fp32
// accumulate -- bit-for-bit an fmaf chain, so parity with an fp32 reference holds to
// rounding-order level).
//
// Mapping: one wave owns 32 consecutive rows (row = group*nsample + sample) through all
// layers; activations stay in a wave-private LDS tile [32][K+1] (odd stride => the
// A-fragment read, lane -> (row = lane&31, k = lane>>5), is bank-conflict free), weights
// for all layers sit in LDS as W^T [K][C] (B-fragment read is lane-contiguous).  No
// cross-wave synchronisation after the initial weight load.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <type_traits>

#include "geot_common.h"
#include "geot_hip.h"

namespace geot {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int SA_WAVES = 12;  // at most (3 per SIMD); the launcher uses 8 or 4 when the activation tiles do not fit the LDS
constexpr int SA_MAX_LAYERS = 4;

struct SaDesc {
    int nlayers;
    int kp[SA_MAX_LAYERS];   // padded input width of layer l (even)
    int cp[SA_MAX_LAYERS];   // padded output width of layer l (32, 64, 128 or 256)
    int woff[SA_MAX_LAYERS]; // float offset of W^T [kp][cp] in the parameter block
    int boff[SA_MAX_LAYERS]; // float offset of bias [cp]
    int w[SA_MAX_LAYERS];    // unpadded output width of layer l (the columns past it are stored as 0)
    int relu_mask;           // bit l = ReLU after layer l
    int total;               // floats in the parameter block
    int act_stride;          // floats per activation row (widest STORED activation + 1, odd; the last layer is pooled from registers)
};

// max that propagates NaN like torch.relu / torch.max (fmaxf returns the other operand): llvm.maximum, one
// v_maximum3_f32 on gfx950.  It also orders -0 below +0, so any order of the same maxima gives the same bits.
__device__ __forceinline__ float sa_max(float a, float b) { return __builtin_elementwise_maximum(a, b); }

template <int NCT>
__device__ __forceinline__ void sa_layer(const float *__restrict__ W, const float *__restrict__ bias,
                                         int kp, int cp, bool relu, float *__restrict__ act,
                                         int act_stride, f32x16 (&acc)[NCT])
{
    const int lane = lane_id(), r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        float bv = bias[ct * 32 + r];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[ct][e] = bv;
    }
    const float *arow = act + r * act_stride + h;
    const float *wrow = W + h * cp + r;
    for (int k0 = 0; k0 < kp; k0 += 2) {
        float a = arow[k0];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            float b = wrow[k0 * cp + ct * 32];
            acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[ct], 0, 0, 0);
        }
    }
    if (relu) {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ct][e] = sa_max(acc[ct][e], 0.f);
    }
}

// D layout of the 32x32 tile: col = lane&31, row = (e&3) + 8*(e>>2) + 4*(lane>>5).
// Columns at or past the layer's width w are stored as 0: their weights and bias are 0, but 0 * inf is NaN, and the
// next layer's (zero) weights would carry that NaN into every real column where the composed module has none.
template <int NCT>
__device__ __forceinline__ void sa_store_act(const f32x16 (&acc)[NCT], float *__restrict__ act, int act_stride, int w)
{
    const int lane = lane_id(), c = lane & 31, h = lane >> 5;
    const bool padded = w < NCT * 32;   // uniform over the wave
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const bool live = ct * 32 + c < w;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            int row = (e & 3) + 8 * (e >> 2) + 4 * h;
            act[row * act_stride + ct * 32 + c] = (!padded || live) ? acc[ct][e] : 0.f;
        }
    }
}

// Max over the rows of each group inside the tile, merged into pool[g_local][col].
// gpt = groups per tile (1 when nsample >= 32, else 32 / nsample in {2, 4}).
template <int NCT>
__device__ __forceinline__ void sa_pool(const f32x16 (&acc)[NCT], float *__restrict__ pool, int cp, int gpt)
{
    const int lane = lane_id(), c = lane & 31;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        float m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = sa_max(sa_max(acc[ct][4 * j], acc[ct][4 * j + 1]), sa_max(acc[ct][4 * j + 2], acc[ct][4 * j + 3]));
            m[j] = sa_max(v, __shfl_xor(v, 32));
        }
        if (lane < 32) {
            if (gpt == 1) {
                float v = sa_max(sa_max(m[0], m[1]), sa_max(m[2], m[3]));
                pool[ct * 32 + c] = sa_max(pool[ct * 32 + c], v);
            } else if (gpt == 2) {
                pool[ct * 32 + c] = sa_max(pool[ct * 32 + c], sa_max(m[0], m[1]));
                pool[cp + ct * 32 + c] = sa_max(pool[cp + ct * 32 + c], sa_max(m[2], m[3]));
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) pool[j * cp + ct * 32 + c] = sa_max(pool[j * cp + ct * 32 + c], m[j]);
            }
        }
    }
}

// nsample == 32: the tile IS the group, so the max over its 32 rows is final -- it stays in registers (no LDS
// pool): after the cross-half max both half-waves hold every column's result, half h keeps column tiles
// 2p + h, i.e. o[p] = column p*64 + h*32 + (lane & 31).
template <int NCT>
__device__ __forceinline__ void sa_pool_direct(const f32x16 (&acc)[NCT], float (&o)[4])
{
    const int h = lane_id() >> 5;
    float val[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        float v = acc[ct][0];
#pragma unroll
        for (int e = 1; e < 16; ++e) v = sa_max(v, acc[ct][e]);
        val[ct] = sa_max(v, __shfl_xor(v, 32));
    }
#pragma unroll
    for (int p2 = 0; p2 < 4; ++p2) {
        if (2 * p2 < NCT) {
            const float lo = val[2 * p2], hi = val[(2 * p2 + 1 < NCT) ? 2 * p2 + 1 : 2 * p2];
            o[p2] = h ? hi : lo;
        }
    }
}

// out[b, col, group] <- the register-pooled values of group g (column map: sa_pool_direct).  NP = padded width / 64
// store instructions, every lane active (the fast path requires c_out == padded width): no branch, so the
// compiler can count them when it places the s_waitcnt of the loads issued just before.
template <int NP>
__device__ __forceinline__ void sa_write_direct(const float (&o)[4], int g, int npoint, int c_out, float *__restrict__ out)
{
    const int lane = lane_id(), c = lane & 31, h = lane >> 5;
    const int bi = g / npoint, gi = g - bi * npoint;
    float *dst = out + ((size_t)bi * c_out + h * 32 + c) * npoint + gi;
#pragma unroll
    for (int p2 = 0; p2 < NP; ++p2) dst[(size_t)p2 * 64 * npoint] = o[p2];
}

// layer-0 operands of one tile row, in registers between the global loads and the LDS writes
struct SaRow {
    float p[3], q[3], f[4];
};

template <int NCT>
__device__ __forceinline__ void sa_run_layer(const SaDesc &d, int l, const float *__restrict__ P,
                                             float *__restrict__ act, float *__restrict__ pool, int gpt,
                                             bool direct, float (&o)[4])
{
    f32x16 acc[NCT];
    sa_layer<NCT>(P + d.woff[l], P + d.boff[l], d.kp[l], d.cp[l], (d.relu_mask >> l) & 1, act, d.act_stride, acc);
    if (l + 1 < d.nlayers) sa_store_act<NCT>(acc, act, d.act_stride, d.w[l]);
    else if (direct) sa_pool_direct<NCT>(acc, o);
    else sa_pool<NCT>(acc, pool, d.cp[l], gpt);
}

// MAXW = widest layer / 32 the variant supports: the 8-tile (256-wide) accumulators cost 128 VGPRs, which caps
// the occupancy at 2 waves per SIMD; networks up to 128 wide use the lean variant and run 3.
template <int MAXW>
__global__ __launch_bounds__(MAXW >= 8 ? 512 : SA_WAVES * 64) void sa_group_mlp_max_kernel(
    SaDesc d, int b, int n, int npoint, int nsample, int c_feat, int c_out,
    const float *__restrict__ xyz, const float *__restrict__ new_xyz,
    const float *__restrict__ features, const int *__restrict__ idx, float xyz_scale,
    const float *__restrict__ params, float *__restrict__ out, int fast_np, int run_len)
{
    extern __shared__ float sa_lds[];
    float *P = sa_lds;
    const int wave = threadIdx.x >> 6, lane = lane_id();
    const int cp_last = d.cp[d.nlayers - 1];
    const int gpt = nsample >= 32 ? 1 : 32 / nsample;  // groups per 32-row tile
    float *act = sa_lds + d.total + wave * (32 * d.act_stride + gpt * cp_last);
    float *pool = act + 32 * d.act_stride;
    const int nwaves = blockDim.x >> 6;

    const int tpg = nsample >= 32 ? nsample / 32 : 1;  // tiles per group
    const long long ngroups = (long long)b * npoint;
    const long long nunits = (ngroups + gpt - 1) / gpt;
    const int k_in = 3 + c_feat;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (fast_np) {
        // ---- nsample == 32, c_feat <= 8, no padded output columns, < 2^31 groups: the tile IS the group.  Pooled in
        // registers; software-pipelined so that the global loads of the NEXT group's rows are in flight before
        // this group's 128 scattered 4-byte stores are issued: vmcnt retires in order, and a gather issued behind
        // the stores would wait for their acknowledgement (the stores alone cost 12 % of the launch that way).
        const int r = lane & 31, h = lane >> 5;
        float *arow = act + r * d.act_stride;
        // a workgroup owns a contiguous run of groups and its waves walk it together: the 4-byte stores of one
        // output column then land next to each other in the SAME L2 within a few tiles and leave it as whole lines
        // (interleaving the groups over workgroups scattered every line over all eight L2s: partial-sector writes)
        auto load = [&](SaRow &R, int g) {
            const int bi = g / npoint;
            const int a = idx[(size_t)g * 32 + r];
            const float *pp = xyz + ((size_t)bi * n + a) * 3, *q = new_xyz + (size_t)g * 3;
#pragma unroll
            for (int x = 0; x < 3; ++x) { R.p[x] = pp[x]; R.q[x] = q[x]; }
            const float *f = features + (size_t)bi * c_feat * n + a;
#pragma unroll
            for (int j = 0; j < 4; ++j) R.f[j] = (h + 2 * j < c_feat) ? f[(size_t)(h + 2 * j) * n] : 0.f;
        };
        auto commit = [&](const SaRow &R) {
            if (h == 0) {
#pragma unroll
                for (int x = 0; x < 3; ++x) arow[x] = (R.p[x] - R.q[x]) * xyz_scale;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (h + 2 * j < c_feat) arow[3 + h + 2 * j] = R.f[j];
            for (int ch = k_in + h; ch < d.kp[0]; ch += 2) arow[ch] = 0.f;
        };
        // A wave walks RUNS of 8 consecutive groups and keeps their pooled columns in registers (hist): a lane then
        // owns, per column, 8 consecutive floats of out[b, col, :] = one aligned 32-byte sector, written as two
        // dwordx4 stores -- 4x fewer, 4x larger write requests than one 4-byte store per (group, column) (the
        // scattered 4-byte stores were request-rate-bound in the L2: 16 % of the launch).  The stores are
        // issued straight-line before the LDS writes of the rows loaded just before them (wait = vmcnt(2 NP)).
        float hist[8][4];
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int p2 = 0; p2 < 4; ++p2) hist[j][p2] = 0.f;
        auto store_run = [&](int g0, auto np_tag) {
            constexpr int NP = decltype(np_tag)::value;
            const int bi = g0 / npoint, gi0 = g0 - bi * npoint;
            float *dst = out + ((size_t)bi * c_out + h * 32 + (lane & 31)) * npoint + gi0;
#pragma unroll
            for (int p2 = 0; p2 < NP; ++p2) {
                typedef float f32x4 __attribute__((ext_vector_type(4)));
                f32x4 lo = {hist[0][p2], hist[1][p2], hist[2][p2], hist[3][p2]};
                f32x4 hi = {hist[4][p2], hist[5][p2], hist[6][p2], hist[7][p2]};
                f32x4 *d4 = reinterpret_cast<f32x4 *>(dst + (size_t)p2 * 64 * npoint);
                d4[0] = lo;
                d4[1] = hi;
            }
        };
        // run length 1 (few groups per wave: keep every wave busy): the newest entry, 4-byte stores
        auto store_one = [&](int g, auto np_tag) {
            constexpr int NP = decltype(np_tag)::value;
            const int bi = g / npoint, gi = g - bi * npoint;
            float *dst = out + ((size_t)bi * c_out + h * 32 + (lane & 31)) * npoint + gi;
#pragma unroll
            for (int p2 = 0; p2 < NP; ++p2) dst[(size_t)p2 * 64 * npoint] = hist[7][p2];
        };
        auto store_then_commit = [&](int g0, bool do_store, const SaRow *Rn) {
            if (!do_store) { if (Rn) commit(*Rn); }
            else if (run_len == 8) {
                if (fast_np == 1) { store_run(g0, std::integral_constant<int, 1>()); if (Rn) commit(*Rn); }
                else if (fast_np == 2) { store_run(g0, std::integral_constant<int, 2>()); if (Rn) commit(*Rn); }
                else { store_run(g0, std::integral_constant<int, 4>()); if (Rn) commit(*Rn); }
            } else {
                if (fast_np == 1) { store_one(g0, std::integral_constant<int, 1>()); if (Rn) commit(*Rn); }
                else if (fast_np == 2) { store_one(g0, std::integral_constant<int, 2>()); if (Rn) commit(*Rn); }
                else { store_one(g0, std::integral_constant<int, 4>()); if (Rn) commit(*Rn); }
            }
        };
        // runs: a workgroup owns a contiguous range of runs (one L2 sees all of a line's sectors), wave w takes
        // runs first + w, first + w + nwaves, ...
        const int nruns = (int)(ngroups / run_len);      // run_len == 8 requires npoint % 8 == 0
        const int rchunk = (nruns + gridDim.x - 1) / gridDim.x;
        const int rend = min((int)(blockIdx.x + 1) * rchunk, nruns);
        int run = blockIdx.x * rchunk + wave, j = 0;
        SaRow R;
        if (run < rend) load(R, run * run_len);   // the first rows travel while the weights are staged
        for (int i = threadIdx.x; i < d.total; i += blockDim.x) P[i] = params[i];
        __syncthreads();
        if (run < rend) commit(R);
        while (run < rend) {
            for (int l = 0; l < d.nlayers; ++l) {
                const int w32 = d.cp[l] >> 5;
                if (w32 == 1) sa_run_layer<1>(d, l, P, act, pool, 1, true, o);
                else if (w32 == 2) sa_run_layer<2>(d, l, P, act, pool, 1, true, o);
                else if (MAXW >= 8 && w32 == 8) sa_run_layer<(MAXW >= 8 ? 8 : 4)>(d, l, P, act, pool, 1, true, o);
                else sa_run_layer<4>(d, l, P, act, pool, 1, true, o);
            }
#pragma unroll
            for (int jj = 0; jj < 7; ++jj)
#pragma unroll
                for (int p2 = 0; p2 < 4; ++p2) hist[jj][p2] = hist[jj + 1][p2];
#pragma unroll
            for (int p2 = 0; p2 < 4; ++p2) hist[7][p2] = o[p2];
            const bool full = j == run_len - 1;
            const int g0 = run * run_len;
            const int nrun = full ? run + nwaves : run, nj = full ? 0 : j + 1;
            if (nrun < rend) {
                load(R, nrun * run_len + nj);
                store_then_commit(g0, full, &R);
            } else {
                store_then_commit(g0, full, nullptr);
            }
            run = nrun;
            j = nj;
        }
        return;
    }
    for (int i = threadIdx.x; i < d.total; i += blockDim.x) P[i] = params[i];
    __syncthreads();
    const long long uchunk = (nunits + gridDim.x - 1) / gridDim.x, uend = min((long long)(blockIdx.x + 1) * uchunk, nunits);
    for (long long u = (long long)blockIdx.x * uchunk + wave; u < uend; u += nwaves) {   // contiguous run per workgroup
        for (int i = lane; i < gpt * cp_last; i += 64) pool[i] = -INFINITY;
        for (int t = 0; t < tpg; ++t) {
            // ---- layer-0 input: row r of the tile <- (xyz[idx]-centre)*scale, features[:, idx]
            {
                const int r = lane & 31, h = lane >> 5;
                long long g = u * gpt + (nsample >= 32 ? 0 : r / nsample);
                int s = nsample >= 32 ? t * 32 + r : r % nsample;
                float *arow = act + r * d.act_stride;
                if (g < ngroups) {
                    int bi = (int)(g / npoint);
                    int a = idx[g * nsample + s];
                    if (h == 0) {
                        const float *p = xyz + ((size_t)bi * n + a) * 3, *q = new_xyz + g * 3;
                        arow[0] = (p[0] - q[0]) * xyz_scale;
                        arow[1] = (p[1] - q[1]) * xyz_scale;
                        arow[2] = (p[2] - q[2]) * xyz_scale;
                    }
                    const float *f = features + (size_t)bi * c_feat * n + a;
                    for (int ch = h; ch < c_feat; ch += 2) arow[3 + ch] = f[(size_t)ch * n];
                    for (int ch = k_in + h; ch < d.kp[0]; ch += 2) arow[ch] = 0.f;
                } else {
                    for (int ch = h; ch < d.kp[0]; ch += 2) arow[ch] = 0.f;
                }
            }
            for (int l = 0; l < d.nlayers; ++l) {
                const int w32 = d.cp[l] >> 5;
                if (w32 == 1) sa_run_layer<1>(d, l, P, act, pool, gpt, false, o);
                else if (w32 == 2) sa_run_layer<2>(d, l, P, act, pool, gpt, false, o);
                else if (MAXW >= 8 && w32 == 8) sa_run_layer<(MAXW >= 8 ? 8 : 4)>(d, l, P, act, pool, gpt, false, o);
                else sa_run_layer<4>(d, l, P, act, pool, gpt, false, o);
            }
        }
        // ---- pooled result -> out[b, col, group]
        for (int i = lane; i < gpt * c_out; i += 64) {
            int gl = i / c_out, col = i - gl * c_out;
            long long g = u * gpt + gl;
            if (g < ngroups) {
                int bi = (int)(g / npoint);
                int gi = (int)(g - (long long)bi * npoint);
                out[((size_t)bi * c_out + col) * npoint + gi] = pool[gl * cp_last + col];
            }
        }
    }
}

static inline int pad_cols(int c) { return c <= 32 ? 32 : c <= 64 ? 64 : c <= 128 ? 128 : 256; }

// Every launch decision of geot_sa_group_mlp_max, in one place: the launcher and the host-only query geot_sa_plan
// both read it, so the query cannot drift from the dispatch.  cus = the device's CU count (the persistent grid's cap);
// out_aligned16 = the output starts on a 16-byte boundary (the run-of-8 stores are dwordx4).  The GEOT_SA_FAST /
// GEOT_SA_RUN overrides are the launcher's, not the plan's.  ok says whether the kernel takes the shape.
struct SaPlan {
    bool ok, wide;
    int waves, gpt, tpg, fast_np, run_len;
    long long lds, blocks, nunits;
    SaDesc d;
};
static SaPlan sa_plan(int b, int npoint, int nsample, int c_feat, int nlayers, const int *widths, int cus,
                      bool out_aligned16)
{
    SaPlan p = {};
    if (b < 0 || npoint < 0 || c_feat < 0 || nlayers < 1 || nlayers > SA_MAX_LAYERS || !widths || cus < 1) return p;
    if (!(nsample == 8 || nsample == 16 || (nsample >= 32 && nsample % 32 == 0))) return p;
    for (int l = 0; l < nlayers; ++l)
        if (widths[l] < 1 || widths[l] > 256) return p;
    // the descriptor; sizes in 64 bits until the LDS bound has capped them
    SaDesc &d = p.d;
    long long kp = (3LL + c_feat + 1) & ~1LL, off = 0, maxw = kp;
    long long kps[SA_MAX_LAYERS], offs[2 * SA_MAX_LAYERS];
    for (int l = 0; l < nlayers; ++l) {
        const int cp = pad_cols(widths[l]);
        kps[l] = kp; offs[2 * l] = off; off += kp * cp; offs[2 * l + 1] = off; off += cp;
        if (l + 1 < nlayers && cp > maxw) maxw = cp; // the last layer's output never goes to the activation tile
        kp = cp;
    }
    p.gpt = nsample >= 32 ? 1 : 32 / nsample;          // groups per 32-row tile
    p.tpg = nsample >= 32 ? nsample / 32 : 1;          // tiles per group
    for (int l = 0; l < nlayers; ++l) p.wide = p.wide || pad_cols(widths[l]) > 128;
    // As many waves per workgroup (= per CU: the weights + activation tiles fill its LDS) as fit next to the
    // weights, up to 3 per SIMD: one wave's gather, LDS round trips and accumulator hand-offs between layers
    // then overlap with the others' MFMA chains.
    const long long per_wave = 32 * (maxw + 1) + (long long)p.gpt * pad_cols(widths[nlayers - 1]);
    p.waves = p.wide ? 8 : SA_WAVES;
    while (p.waves > 4 && (off + p.waves * per_wave) * (long long)sizeof(float) > 160 * 1024) p.waves -= 4;
    p.lds = (off + p.waves * per_wave) * (long long)sizeof(float);
    if (p.lds > 160 * 1024) return p;
    d.nlayers = nlayers;
    for (int l = 0; l < nlayers; ++l) {
        d.kp[l] = (int)kps[l]; d.cp[l] = pad_cols(widths[l]); d.w[l] = widths[l];
        d.woff[l] = (int)offs[2 * l]; d.boff[l] = (int)offs[2 * l + 1];
    }
    d.total = (int)off;
    d.act_stride = (int)maxw + 1;
    p.nunits = ((long long)b * npoint + p.gpt - 1) / p.gpt;
    // persistent workgroups: one per CU (the weights + activation tiles fill its LDS), each looping over its
    // share of the tiles, so the 52 KB of weights are staged once per CU and not once per 8 tiles
    p.blocks = std::min((p.nunits + p.waves - 1) / p.waves, (long long)cus);
    // register-pooled, software-pipelined path (see the kernel): one 32-row tile per group, few feature channels,
    // no padded output columns
    const int c_last = widths[nlayers - 1];
    const long long ngroups = (long long)b * npoint;
    if (nsample == 32 && c_feat <= 8 && c_last == d.cp[nlayers - 1] && c_last >= 64 && ngroups < 0x7fffffffLL &&
        ngroups * 32 < 0x7fffffffLL * 4)
        p.fast_np = c_last / 64;
    // runs of 8 consecutive groups per wave (sector-sized output stores) once every wave still gets >= 2 runs
    p.run_len = (p.fast_np && npoint % 8 == 0 && out_aligned16 && p.nunits >= 16 * p.blocks * p.waves) ? 8 : 1;
    p.ok = true;
    return p;
}

} // namespace geot

using namespace geot;

GEOT_EXPORT int geot_sa_param_floats(int c_feat, int nlayers, const int *widths)
{
    if (nlayers < 1 || nlayers > SA_MAX_LAYERS || c_feat < 0) return -1;
    long long total = 0, kp = (3LL + c_feat + 1) & ~1LL;
    for (int l = 0; l < nlayers; ++l) {
        if (widths[l] < 1 || widths[l] > 256) return -1;
        int cp = pad_cols(widths[l]);
        total += kp * cp + cp;
        kp = cp;
    }
    return total > 0x7fffffffLL ? -1 : (int)total;
}

GEOT_EXPORT int geot_sa_plan(int b, int npoint, int nsample, int c_feat, int nlayers, const int *widths, int cus,
                             int out_aligned16, long long *out, int n_out)
{
    const SaPlan p = sa_plan(b, npoint, nsample, c_feat, nlayers, widths, cus, out_aligned16 != 0);
    if (p.ok && out) {
        const SaDesc &d = p.d;
        long long v[11 + 4 * SA_MAX_LAYERS] = {p.wide, p.waves, p.lds, p.blocks, p.gpt, p.tpg, p.fast_np, p.run_len,
                                               p.nunits, d.total, d.act_stride};
        for (int l = 0; l < d.nlayers; ++l) {
            v[11 + l] = d.kp[l];
            v[11 + SA_MAX_LAYERS + l] = d.cp[l];
            v[11 + 2 * SA_MAX_LAYERS + l] = d.woff[l];
            v[11 + 3 * SA_MAX_LAYERS + l] = d.boff[l];
        }
        for (int i = 0; i < n_out && i < 11 + 4 * SA_MAX_LAYERS; ++i) out[i] = v[i];
    }
    return p.ok ? 1 : 0;
}

GEOT_EXPORT int geot_sa_group_mlp_max(int b, int n, int npoint, int nsample, int c_feat,
                                      const float *xyz, const float *new_xyz, const float *features,
                                      const int *idx, float xyz_scale, int nlayers, const int *widths,
                                      int relu_mask, const float *params, float *out, void *stream)
{
    if (b < 0 || n < 0 || npoint < 0 || nlayers < 1 || nlayers > SA_MAX_LAYERS || c_feat < 0)
        return hipErrorInvalidValue;
    if (!(nsample == 8 || nsample == 16 || (nsample >= 32 && nsample % 32 == 0))) return hipErrorInvalidValue;
    if (b == 0 || npoint == 0) return hipSuccess;      // nothing to read: the arrays may be NULL
    if (c_feat > 0 && !features) return hipErrorInvalidValue;
    SaPlan p = sa_plan(b, npoint, nsample, c_feat, nlayers, widths, device_cus(), ((uintptr_t)out & 15) == 0);
    if (!p.ok) return hipErrorInvalidValue;
    p.d.relu_mask = relu_mask;
    {   // > 64 KB of dynamic LDS is opt-in, per device and per kernel: raised once (geot_common.h allow_big_lds)
        hipError_t e = p.wide ? allow_big_lds((const void *)sa_group_mlp_max_kernel<8>, p.lds)
                              : allow_big_lds((const void *)sa_group_mlp_max_kernel<4>, p.lds);
        if (e != hipSuccess) return e;
    }
    int fast_np = p.fast_np, run_len = p.run_len;
    if (const char *fe = getenv("GEOT_SA_FAST")) fast_np = atoi(fe) ? fast_np : 0;
    if (!fast_np) run_len = 1;
    if (const char *re = getenv("GEOT_SA_RUN")) run_len = (atoi(re) == 8 && npoint % 8 == 0 && ((uintptr_t)out & 15) == 0) ? 8 : 1;
    if (p.wide)
        hipLaunchKernelGGL(sa_group_mlp_max_kernel<8>, dim3((unsigned)p.blocks), dim3(p.waves * 64), p.lds, (hipStream_t)stream,
                           p.d, b, n, npoint, nsample, c_feat, widths[nlayers - 1], xyz, new_xyz, features, idx, xyz_scale,
                           params, out, fast_np, run_len);
    else
        hipLaunchKernelGGL(sa_group_mlp_max_kernel<4>, dim3((unsigned)p.blocks), dim3(p.waves * 64), p.lds, (hipStream_t)stream,
                           p.d, b, n, npoint, nsample, c_feat, widths[nlayers - 1], xyz, new_xyz, features, idx, xyz_scale,
                           params, out, fast_np, run_len);
    return hipGetLastError();
}
