// The teacher-student point contrastive loss of utils/cluster_contrastloss.py (nativeContrastLoss_t, :1188-1408) in a form
// with fixed shapes, counts kept on the device and no host round trip -- safe to capture.  include/geot_hip.h states the
// arithmetic; this file is four entry points:
//
//   geot_contrast_select     ordered compaction of the points over the threshold per cloud, the draw of at most S of them,
//                            the packed anchor list, its inverse map and the rows the bank will take        (2 launches)
//   geot_contrast_loss       gather + normalise the A selected rows of both tensors, ONE streaming pass per anchor over
//                            the A positives and the 4S bank rows (two running maxima, their sums and W_a together: the
//                            backward needs neither the bank nor a second sweep), merge, fixed-tree mean     (4 launches)
//   geot_contrast_loss_grad  upstream scale, normalisation backward, dense gradient (zeros included)          (2 launches)
//   geot_contrast_enqueue    the bank rows and the pointer                                                    (2 launches)
//
// The pass is a plain fp32 LDS-tiled form: a block of 256 threads holds TA anchors and streams tiles of TK keys; a thread
// owns an (TA / 16) x (TK / 16) patch of the scores and (TA / 16) x (DP / 16) of W.  The keys are cut into chunks of
// CT_CHUNK, one block per (anchor tile, chunk), so that 2048 anchors fill the chip; the chunks' (max, sum, W) are merged in
// chunk order by the next kernel.  No atomics and no dependence on arrival order anywhere: bit-identical from run to run.
// The library is built with -ffp-contract=off; the inner products below say fmaf themselves.
#include <hip/hip_runtime.h>
#include <math.h>

#include "geot_common.h"
#include "geot_hip.h"
#include "philox.h"

namespace geot {

typedef unsigned long long u64;

constexpr int CT_THREADS = 256, CT_CHUNK = 1024, CT_ROUNDS = 8, CT_MIN_BITS = 10;
constexpr float CT_EPS = 1e-12f;      // F.normalize's eps

// ---------------------------------------------------------------------------------------------------------------- select
// geot_sample_draw's keyed bijection in its n >= m construction (csrc/sample_draw.hip), n read on the device
__device__ __forceinline__ uint32_t ct_walk(uint32_t j, uint32_t n, u64 d, u64 seed)
{
    const uint32_t d_lo = (uint32_t)d, d_hi = (uint32_t)(d >> 32), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    int b = 32 - __clz((int)(n - 1u));
    b = b < CT_MIN_BITS ? CT_MIN_BITS : b;
    const int lb = b >> 1, rb = b - lb;
    const uint32_t mask_l = (1u << lb) - 1u, mask_r = (1u << rb) - 1u;
    uint32_t x = j;
    do {
        uint32_t left = x >> rb, right = x & mask_r;
#pragma unroll
        for (int r = 0; r < CT_ROUNDS; r += 2) {
            left ^= philox4x32_10(right, (uint32_t)r, d_lo, d_hi, k0, k1).w[0] & mask_l;
            right ^= philox4x32_10(left, (uint32_t)r + 1u, d_lo, d_hi, k0, k1).w[0] & mask_r;
        }
        x = (left << rb) | right;
    } while (x >= n);
    return x;
}

// grid (b): a block per cloud walks its scores in ascending order; ws = cand (b * p) | K (b) | counter snapshot (2 words)
__global__ __launch_bounds__(CT_THREADS) void ct_compact_kernel(int p, float th, const float *__restrict__ score,
                                                               const u64 *__restrict__ counter, int *__restrict__ ws,
                                                               int *__restrict__ inv)
{
    __shared__ int wtot[CT_THREADS / 64];
    const int nb = gridDim.x, cloud = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long base = (long long)cloud * p;
    int *cand = ws + base, *kk = ws + (long long)nb * p, *snap = kk + nb;
    int run = 0;
    for (int p0 = 0; p0 < p; p0 += CT_THREADS) {
        const int pt = p0 + tid;
        bool flag = false;
        if (pt < p) {
            flag = score[base + pt] >= th;       // (a NaN score compares false)
            inv[base + pt] = -1;
        }
        const u64 mask = __ballot(flag);
        const int rank = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[wave] = __popcll(mask);
        __syncthreads();
        int woff = 0, total = 0;
#pragma unroll
        for (int w = 0; w < CT_THREADS / 64; ++w) {
            woff += w < wave ? wtot[w] : 0;
            total += wtot[w];
        }
        if (flag) cand[run + woff + rank] = pt;
        run += total;
        __syncthreads();
    }
    if (tid == 0) {
        kk[cloud] = run;
        if (cloud == 0) {
            const u64 c = counter ? *counter : 0ull;
            snap[0] = (int)(uint32_t)c;
            snap[1] = (int)(uint32_t)(c >> 32);
        }
    }
}

// grid (ceil(s / CT_THREADS), b + 1): rows 0 .. b - 1 pack their cloud's anchors, row b lists the rows the bank takes
__global__ __launch_bounds__(CT_THREADS) void ct_pack_kernel(int nb, int p, int s, const long long *__restrict__ perm,
                                                            const long long *__restrict__ perm_q, u64 seed,
                                                            u64 *__restrict__ counter, const int *__restrict__ ws,
                                                            int *__restrict__ anchors, int *__restrict__ count,
                                                            int *__restrict__ enqueue_rows, int *__restrict__ inv)
{
    const int y = blockIdx.y, j = blockIdx.x * CT_THREADS + threadIdx.x;
    const int *kk = ws + (long long)nb * p, *snap = kk + nb;
    const u64 base = (u64)(uint32_t)snap[0] | ((u64)(uint32_t)snap[1] << 32);
    int off = 0, total = 0;
    for (int c = 0; c < nb; ++c) {
        const int m = min(kk[c], s);
        off += c < y ? m : 0;
        total += m;
    }
    if (j >= s) return;
    if (y == nb) {
        const int cnt = min(total, s);
        int row = -1;
        if (j < cnt) {
            if (perm_q) {
                const long long v = perm_q[j];
                row = v >= 0 && v < total ? (int)v : -1;
            } else {
                row = (int)ct_walk((uint32_t)j, (uint32_t)total, base + (u64)nb, seed);
            }
        }
        enqueue_rows[j] = row;
        return;
    }
    const int k = kk[y], m = min(k, s);
    if (j < m) {
        long long idx = perm ? perm[(long long)y * s + j] : (long long)ct_walk((uint32_t)j, (uint32_t)k, base + (u64)y, seed);
        int pt = -1;
        if (idx >= 0 && idx < k) {       // (a given permutation entry outside [0, K) is never followed)
            pt = y * p + ws[(long long)y * p + idx];
            inv[pt] = off + j;
        }
        anchors[off + j] = pt;
    }
    const long long g = (long long)y * s + j;
    if (g >= total) anchors[g] = -1;
    if (j == 0) {
        count[y] = m;
        if (y == 0) {
            count[nb] = total;
            if (counter) *counter = base + (u64)nb + 1ull;     // (every block read the snapshot, never the counter)
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ loss
// butterfly over the 64 lanes / the 16 lanes of a row: every stage adds the same pair in every lane, so all lanes end with
// the same bits
__device__ __forceinline__ float ct_wave_sum(float v)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float ct_row16_sum(float v)
{
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float ct_row16_max(float v)
{
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ long long ct_elem(int pt, int c, int p, int d, int channels_first)
{
    if (!channels_first) return (long long)pt * d + c;
    const int b = pt / p, q = pt - b * p;
    return ((long long)b * d + c) * p + q;
}

// grid (b * s), a wave per slot: rows of both tensors read in place, x / max(|x|, eps)
__global__ __launch_bounds__(64) void ct_gather_kernel(int nb, int p, int d, int channels_first,
                                                      const float *__restrict__ feat_s, const float *__restrict__ feat_t,
                                                      const int *__restrict__ anchors, const int *__restrict__ count,
                                                      float *__restrict__ xhat, float *__restrict__ that,
                                                      float *__restrict__ norm)
{
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= count[nb]) return;
    const int pt = anchors[g];
    float xs[4], ts[4], sx = 0.f, st = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        xs[i] = ts[i] = 0.f;
        if (c < d && pt >= 0) {
            const long long e = ct_elem(pt, c, p, d, channels_first);
            xs[i] = feat_s[e];
            ts[i] = feat_t[e];
        }
        sx = fmaf(xs[i], xs[i], sx);
        st = fmaf(ts[i], ts[i], st);
    }
    const float nx = sqrtf(ct_wave_sum(sx)), nt = sqrtf(ct_wave_sum(st));
    const float dx = fmaxf(nx, CT_EPS), dt = fmaxf(nt, CT_EPS);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        if (c < d) {
            xhat[(long long)g * d + c] = xs[i] / dx;
            that[(long long)g * d + c] = ts[i] / dt;
        }
    }
    if (lane == 0) norm[g] = nx;
}

// grid (ceil(b * s / TA), pos chunks + bank chunks).  Partials per (chunk, anchor): pm max, pz sum, pw (d) weighted key sum
template <int DP, int TA, int TK>
__global__ __launch_bounds__(CT_THREADS) void ct_partial_kernel(int nb, int d, int s4, int cap, int pos_chunks,
                                                               const int *__restrict__ count, const float *__restrict__ xhat,
                                                               const float *__restrict__ that, const float *__restrict__ bank,
                                                               float tau, float *__restrict__ pm, float *__restrict__ pz,
                                                               float *__restrict__ pw)
{
    constexpr int RA = TA / 16, RK = TK / 16, NC = DP / 64, XS = DP + 4, PS = TK + 4;
    __shared__ __attribute__((aligned(16))) float xs[TA * XS];
    __shared__ __attribute__((aligned(16))) float ks[TK * XS];
    __shared__ __attribute__((aligned(16))) float ps[TA * PS];
    const int total = count[nb], a0 = blockIdx.x * TA, chunk = blockIdx.y;
    if (a0 >= total) return;
    const bool pos = chunk < pos_chunks;
    const float *src = pos ? that : bank;
    const int k_begin = (pos ? chunk : chunk - pos_chunks) * CT_CHUNK;
    const int k_end = min(k_begin + CT_CHUNK, pos ? total : s4);
    if (k_begin >= k_end) return;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;

    for (int e = tid; e < TA * DP; e += CT_THREADS) {
        const int r = e / DP, c = e - r * DP;
        xs[r * XS + c] = (c < d && a0 + r < total) ? xhat[(long long)(a0 + r) * d + c] : 0.f;
    }
    float m[RA], z[RA], w[RA][NC * 4];
#pragma unroll
    for (int i = 0; i < RA; ++i) {
        m[i] = -INFINITY;
        z[i] = 0.f;
#pragma unroll
        for (int c = 0; c < NC * 4; ++c) w[i][c] = 0.f;
    }
    for (int k0 = k_begin; k0 < k_end; k0 += TK) {
        for (int e = tid; e < TK * DP; e += CT_THREADS) {
            const int r = e / DP, c = e - r * DP;
            ks[r * XS + c] = (c < d && k0 + r < k_end) ? src[(long long)(k0 + r) * d + c] : 0.f;
        }
        __syncthreads();
        float acc[RA][RK];
#pragma unroll
        for (int i = 0; i < RA; ++i)
#pragma unroll
            for (int j = 0; j < RK; ++j) acc[i][j] = 0.f;
        for (int c = 0; c < DP; c += 4) {
            float4 xa[RA], kb[RK];
#pragma unroll
            for (int i = 0; i < RA; ++i) xa[i] = *(const float4 *)&xs[(ty * RA + i) * XS + c];
#pragma unroll
            for (int j = 0; j < RK; ++j) kb[j] = *(const float4 *)&ks[(tx + 16 * j) * XS + c];
#pragma unroll
            for (int i = 0; i < RA; ++i)
#pragma unroll
                for (int j = 0; j < RK; ++j) {
                    acc[i][j] = fmaf(xa[i].x, kb[j].x, acc[i][j]);
                    acc[i][j] = fmaf(xa[i].y, kb[j].y, acc[i][j]);
                    acc[i][j] = fmaf(xa[i].z, kb[j].z, acc[i][j]);
                    acc[i][j] = fmaf(xa[i].w, kb[j].w, acc[i][j]);
                }
        }
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            float sc[RK], tmax = -INFINITY;
#pragma unroll
            for (int j = 0; j < RK; ++j) {
                sc[j] = k0 + tx + 16 * j < k_end ? acc[i][j] / tau : -INFINITY;
                tmax = fmaxf(tmax, sc[j]);
            }
            tmax = ct_row16_max(tmax);                    // (finite: the tile holds at least one key)
            const float m_new = fmaxf(m[i], tmax);
            const float scale = expf(m[i] - m_new);       // (first tile: exp(-inf) = 0)
            float rs = 0.f;
#pragma unroll
            for (int j = 0; j < RK; ++j) {
                const float pr = expf(sc[j] - m_new);
                ps[(ty * RA + i) * PS + tx + 16 * j] = pr;
                rs += pr;
            }
            rs = ct_row16_sum(rs);
            z[i] = z[i] * scale + rs;
            m[i] = m_new;
#pragma unroll
            for (int c = 0; c < NC * 4; ++c) w[i][c] *= scale;
        }
        __syncthreads();
        for (int k = 0; k < TK; ++k) {
            float pk[RA];
#pragma unroll
            for (int i = 0; i < RA; ++i) pk[i] = ps[(ty * RA + i) * PS + k];
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) {
                const float4 kv = *(const float4 *)&ks[k * XS + cc * 64 + tx * 4];
#pragma unroll
                for (int i = 0; i < RA; ++i) {
                    w[i][cc * 4 + 0] = fmaf(pk[i], kv.x, w[i][cc * 4 + 0]);
                    w[i][cc * 4 + 1] = fmaf(pk[i], kv.y, w[i][cc * 4 + 1]);
                    w[i][cc * 4 + 2] = fmaf(pk[i], kv.z, w[i][cc * 4 + 2]);
                    w[i][cc * 4 + 3] = fmaf(pk[i], kv.w, w[i][cc * 4 + 3]);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < RA; ++i) {
        const int a = a0 + ty * RA + i;
        if (a >= total) continue;
        const long long row = (long long)chunk * cap + a;
        if (tx == 0) {
            pm[row] = m[i];
            pz[row] = z[i];
        }
#pragma unroll
        for (int cc = 0; cc < NC; ++cc)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = cc * 64 + tx * 4 + e;
                if (c < d) pw[row * d + c] = w[i][cc * 4 + e];
            }
    }
}

// grid (b * s), a wave per anchor: the chunks merged in chunk order, l_a and t_a - W_a / Z_a
__global__ __launch_bounds__(64) void ct_merge_kernel(int nb, int d, int s4, int cap, int pos_chunks,
                                                     const int *__restrict__ count, const float *__restrict__ xhat,
                                                     const float *__restrict__ that, const float *__restrict__ pm,
                                                     const float *__restrict__ pz, const float *__restrict__ pw, float tau,
                                                     float tau_b, float *__restrict__ ell, float *__restrict__ gdir)
{
    const int a = blockIdx.x, lane = threadIdx.x, total = count[nb];
    if (a >= total) return;
    const int n_chunks[2] = {(total + CT_CHUNK - 1) / CT_CHUNK, (s4 + CT_CHUNK - 1) / CT_CHUNK};
    const int first[2] = {0, pos_chunks};
    float zsum = 0.f, wsum[4] = {0.f, 0.f, 0.f, 0.f}, mu = 0.f;
#pragma unroll
    for (int part = 0; part < 2; ++part) {
        float mx = -INFINITY;
        for (int c = 0; c < n_chunks[part]; ++c) mx = fmaxf(mx, pm[(long long)(first[part] + c) * cap + a]);
        float zz = 0.f, ww[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < n_chunks[part]; ++c) {
            const long long row = (long long)(first[part] + c) * cap + a;
            const float f = expf(pm[row] - mx);
            zz = fmaf(pz[row], f, zz);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int col = lane + 64 * i;
                if (col < d) ww[i] = fmaf(pw[row * d + col], f, ww[i]);
            }
        }
        zsum += zz;
#pragma unroll
        for (int i = 0; i < 4; ++i) wsum[i] += ww[i];
        if (part == 0) mu = mx;
    }
    float dot = 0.f, tv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int col = lane + 64 * i;
        tv[i] = col < d ? that[(long long)a * d + col] : 0.f;
        dot = fmaf(col < d ? xhat[(long long)a * d + col] : 0.f, tv[i], dot);
    }
    dot = ct_wave_sum(dot);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int col = lane + 64 * i;
        if (col < d) gdir[(long long)a * d + col] = tv[i] - wsum[i] / zsum;
    }
    if (lane == 0) ell[a] = -(tau / tau_b) * ((dot / tau - mu) - logf(zsum));
}

// one block: every thread sums its stride in order, then a fixed tree; A = 0 gives exactly 0
__global__ __launch_bounds__(CT_THREADS) void ct_mean_kernel(int nb, const int *__restrict__ count,
                                                            const float *__restrict__ ell, float *__restrict__ loss)
{
    __shared__ float part[CT_THREADS];
    const int tid = threadIdx.x, total = count[nb];
    float v = 0.f;
    for (int a = tid; a < total; a += CT_THREADS) v += ell[a];
    part[tid] = v;
    __syncthreads();
    for (int h = CT_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) part[tid] += part[tid + h];
        __syncthreads();
    }
    if (tid == 0) *loss = total > 0 ? part[0] / (float)total : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------ grad
// grid (b * s), a wave per anchor: dy = -(g / (A tau_b)) (t - W / Z), then F.normalize's backward
__global__ __launch_bounds__(64) void ct_rowgrad_kernel(int nb, int d, const int *__restrict__ count,
                                                       const float *__restrict__ xhat, const float *__restrict__ norm,
                                                       const float *__restrict__ gdir, const float *__restrict__ upstream,
                                                       float tau_b, float *__restrict__ rows)
{
    const int a = blockIdx.x, lane = threadIdx.x, total = count[nb];
    if (a >= total) return;
    const float scale = -(*upstream / ((float)total * tau_b)), n = norm[a];
    float dy[4], xh[4], dot = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int col = lane + 64 * i;
        dy[i] = col < d ? scale * gdir[(long long)a * d + col] : 0.f;
        xh[i] = col < d ? xhat[(long long)a * d + col] : 0.f;
        dot = fmaf(dy[i], xh[i], dot);
    }
    dot = ct_wave_sum(dot);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int col = lane + 64 * i;
        if (col < d) rows[(long long)a * d + col] = n >= CT_EPS ? (dy[i] - xh[i] * dot) / n : dy[i] / CT_EPS;
    }
}

// every element of the dense gradient, zeros included
__global__ __launch_bounds__(CT_THREADS) void ct_dense_kernel(long long elems, int p, int d, int channels_first,
                                                             const int *__restrict__ inv, const float *__restrict__ rows,
                                                             float *__restrict__ grad)
{
    for (long long e = (long long)blockIdx.x * CT_THREADS + threadIdx.x; e < elems; e += (long long)gridDim.x * CT_THREADS) {
        long long pt;
        int c;
        if (channels_first) {
            const long long bc = e / p;
            c = (int)(bc % d);
            pt = (bc / d) * p + (e - bc * p);
        } else {
            pt = e / d;
            c = (int)(e - pt * d);
        }
        const int slot = inv[pt];
        grad[e] = slot >= 0 ? rows[(long long)slot * d + c] : 0.f;
    }
}

// --------------------------------------------------------------------------------------------------------------- enqueue
// grid (s), a wave per row
__global__ __launch_bounds__(64) void ct_enqueue_kernel(int nb, int d, int s, const int *__restrict__ count,
                                                       const int *__restrict__ enqueue_rows, const float *__restrict__ that,
                                                       float *__restrict__ bank, const long long *__restrict__ ptr)
{
    const int r = blockIdx.x, lane = threadIdx.x, total = count[nb], cnt = min(total, s), s4 = 4 * s;
    if (r >= cnt) return;
    const int j = enqueue_rows[r];
    const long long at = *ptr;
    if (j < 0 || j >= total || at < 0 || at >= s4) return;
    float v[4], sq = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int col = lane + 64 * i;
        v[i] = col < d ? that[(long long)j * d + col] : 0.f;
        sq = fmaf(v[i], v[i], sq);
    }
    const float den = fmaxf(sqrtf(ct_wave_sum(sq)), CT_EPS);
    const long long row = at + cnt > s4 ? (long long)(s4 - cnt + r) : at + r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int col = lane + 64 * i;
        if (col < d) bank[row * d + col] = v[i] / den;
    }
}

__global__ void ct_pointer_kernel(int nb, int s, const int *__restrict__ count, long long *__restrict__ ptr)
{
    const int cnt = min(count[nb], s), s4 = 4 * s;
    const long long at = *ptr;
    if (at < 0 || at >= s4) return;
    *ptr = at + cnt > s4 ? 0 : (at + cnt) % s4;
}

static bool ct_dims(int b, int p, int d, int s)
{
    return b >= 1 && b <= GEOT_CONTRAST_MAX_B && p >= 1 && (long long)b * p <= 0x7fffffffLL && d >= 1 &&
           d <= GEOT_CONTRAST_MAX_D && s >= 1 && s <= GEOT_CONTRAST_MAX_S;
}
static int ct_pos_chunks(int b, int s) { return (b * s + CT_CHUNK - 1) / CT_CHUNK; }
static int ct_bank_chunks(int s) { return (4 * s + CT_CHUNK - 1) / CT_CHUNK; }

} // namespace geot

using namespace geot;

GEOT_EXPORT long long geot_contrast_select_ws_ints(int b, int p) { return (long long)b * p + b + 2; }

GEOT_EXPORT long long geot_contrast_ws_floats(int b, int s, int d)
{
    if (b < 1 || s < 1 || d < 1) return 0;
    return (long long)(ct_pos_chunks(b, s) + ct_bank_chunks(s)) * b * s * (d + 2);
}

GEOT_EXPORT int geot_contrast_select(int b, int p, int s, float th, const float *score, const long long *perm,
                                     const long long *perm_q, unsigned long long seed, unsigned long long *counter, int *ws,
                                     int *anchors, int *count, int *enqueue_rows, int *inv, void *stream)
{
    if (!ct_dims(b, p, 1, s) || !score || !ws || !anchors || !count || !enqueue_rows || !inv) return hipErrorInvalidValue;
    if ((perm == nullptr) != (perm_q == nullptr) || (!perm && !counter)) return hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ct_compact_kernel, dim3(b), dim3(CT_THREADS), 0, st, p, th, score, perm ? nullptr : counter, ws, inv);
    hipLaunchKernelGGL(ct_pack_kernel, dim3((s + CT_THREADS - 1) / CT_THREADS, b + 1), dim3(CT_THREADS), 0, st, b, p, s, perm,
                       perm_q, seed, perm ? nullptr : counter, ws, anchors, count, enqueue_rows, inv);
    return hipGetLastError();
}

template <int DP, int TA, int TK>
static void ct_launch_partial(int b, int d, int s, const int *count, const float *xhat, const float *that, const float *bank,
                              float tau, float *ws, hipStream_t st)
{
    const int cap = b * s, pc = ct_pos_chunks(b, s), chunks = pc + ct_bank_chunks(s);
    float *pm = ws, *pz = pm + (long long)chunks * cap, *pw = pz + (long long)chunks * cap;
    hipLaunchKernelGGL((ct_partial_kernel<DP, TA, TK>), dim3((cap + TA - 1) / TA, chunks), dim3(CT_THREADS), 0, st, b, d, 4 * s,
                       cap, pc, count, xhat, that, bank, tau, pm, pz, pw);
}

GEOT_EXPORT int geot_contrast_loss(int b, int p, int d, int s, int channels_first, const float *feat_s, const float *feat_t,
                                   const int *anchors, const int *count, const float *bank, float tau, float tau_b, float *xhat,
                                   float *that, float *norm, float *ws, float *ell, float *grad_dir, float *loss, void *stream)
{
    if (!ct_dims(b, p, d, s) || !feat_s || !feat_t || !anchors || !count || !bank || !xhat || !that || !norm || !ws || !ell ||
        !grad_dir || !loss || !(tau > 0.f) || !(tau_b > 0.f))
        return hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const int cap = b * s, pc = ct_pos_chunks(b, s), chunks = pc + ct_bank_chunks(s);
    hipLaunchKernelGGL(ct_gather_kernel, dim3(cap), dim3(64), 0, st, b, p, d, channels_first ? 1 : 0, feat_s, feat_t, anchors,
                       count, xhat, that, norm);
    if (d <= 64) ct_launch_partial<64, 64, 64>(b, d, s, count, xhat, that, bank, tau, ws, st);
    else if (d <= 128) ct_launch_partial<128, 64, 32>(b, d, s, count, xhat, that, bank, tau, ws, st);
    else if (d <= 192) ct_launch_partial<192, 32, 32>(b, d, s, count, xhat, that, bank, tau, ws, st);
    else ct_launch_partial<256, 32, 16>(b, d, s, count, xhat, that, bank, tau, ws, st);
    const float *pm = ws, *pz = pm + (long long)chunks * cap, *pw = pz + (long long)chunks * cap;
    hipLaunchKernelGGL(ct_merge_kernel, dim3(cap), dim3(64), 0, st, b, d, 4 * s, cap, pc, count, xhat, that, pm, pz, pw, tau,
                       tau_b, ell, grad_dir);
    hipLaunchKernelGGL(ct_mean_kernel, dim3(1), dim3(CT_THREADS), 0, st, b, count, ell, loss);
    return hipGetLastError();
}

GEOT_EXPORT int geot_contrast_loss_grad(int b, int p, int d, int s, int channels_first, const int *count, const int *inv,
                                        const float *xhat, const float *norm, const float *grad_dir, const float *upstream,
                                        float tau_b, float *rows, float *grad, void *stream)
{
    if (!ct_dims(b, p, d, s) || !count || !inv || !xhat || !norm || !grad_dir || !upstream || !rows || !grad || !(tau_b > 0.f))
        return hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ct_rowgrad_kernel, dim3(b * s), dim3(64), 0, st, b, d, count, xhat, norm, grad_dir, upstream, tau_b, rows);
    const long long elems = (long long)b * p * d;
    long long blocks = (elems + CT_THREADS - 1) / CT_THREADS;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(ct_dense_kernel, dim3((unsigned)blocks), dim3(CT_THREADS), 0, st, elems, p, d, channels_first ? 1 : 0, inv,
                       rows, grad);
    return hipGetLastError();
}

GEOT_EXPORT int geot_contrast_enqueue(int b, int d, int s, const int *count, const int *enqueue_rows, const float *that,
                                      float *bank, long long *ptr, void *stream)
{
    if (!ct_dims(b, 1, d, s) || !count || !enqueue_rows || !that || !bank || !ptr) return hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ct_enqueue_kernel, dim3(s), dim3(64), 0, st, b, d, s, count, enqueue_rows, that, bank, ptr);
    hipLaunchKernelGGL(ct_pointer_kernel, dim3(1), dim3(1), 0, st, b, s, count, ptr);
    return hipGetLastError();
}
