// bnrelu.hip -- BatchNorm (+ ReLU) over channels-first (B, C, L) tensors as HBM-bound streaming kernels, and the
// PointnetFPModule front end fused with the statistics of the BatchNorm behind it (gfx950 / MI355X).
//
// Callers (behaviour, not code): the SharedMLP stages conv1x1 -> BatchNorm -> ReLU of pointnet2/pytorch_utils.py:8-117
// as PointnetFPModule (pointnet2/pointnet2_modules.py:597-642) and the mini-PointNet Encoder
// (openpoints/models/backbone/transformer.py:106-136) run them in training mode.  Stock PyTorch makes 5 passes over
// the tensor forward (statistics; normalise read + write; ReLU read + write) and 8 backward; at 8 clouds x 24 000
// points x 1536 channels one pass is 1.18 GB.  Here: forward = statistics pass (free when the producer is the FP
// front-end kernel below) + ONE apply pass (scale/shift/ReLU); backward = ONE reduce pass + ONE apply pass, the ReLU
// mask recomputed from x instead of stored.  The per-channel arithmetic between the passes (mean, variance, running
// statistics, SyncBatchNorm's all-reduce) is O(C) and stays in the Python wrapper (geot_amd/fused_norm.py).
//
// Algorithmic bytes: apply 8 B/element; backward reduce 8 B, backward apply 12 B; FP front end 4 (C n + C m) + 24 n + 4 Cs n.
//
// The Encoder's folds (geot_bn_*_seg, geot_thin_*): the same passes over x + a per-(channel, segment) addend that is never
// added in memory (same bytes as above, + 4 B per segment), and act(bn(W x)) for J <= 8 input rows with W x never stored
// (apply 4 B/element written, backward 4 B/element read; x itself is J rows, L2-resident).
// Resources on gfx950 (-Rpass-analysis=kernel-resource-usage; no kernel uses scratch or AGPRs):
//   kernel                          VGPRs                              LDS B/block   waves/SIMD
//   bn_stats_seg                    20                                 32            8
//   bn_apply_seg                    17                                 0             8
//   bn_bwd_reduce_seg               34                                 64            8
//   bn_sums_f64                     17                                 0             8
//   bn_bwd_apply_seg<8|4|2|1>       40 40 40 38                        0             8
//   thin_moments<1..8>              17 37 53 61 98 86 104 126          64 .. 1408    8 8 8 8 4 5 4 4
//   thin_bn_sums                    52                                 640           8
//   thin_bn_apply<1..8>             16 34 44 54 64 66 74 82            0             8 8 8 8 8 7 6 5
//   thin_bn_bwd_reduce<1..8>        43 55 67 81 93 105 117 129         96 .. 320     8 8 7 5 5 4 4 3
//   thin_bn_bwd_sums                12                                 0             8
//   thin_bn_wgrad                   32                                 0             8
#include "geot_common.h"
#include "geot_hip.h"

namespace geot {

constexpr int BN_THREADS = 256;
constexpr int BN_MAX_SLICES = 32;

__device__ __forceinline__ float bn_wave_sum(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// two block-wide sums, written by thread 0 / 1 to dst[0], dst[1] (fixed order: deterministic)
__device__ __forceinline__ void bn_block_store2(float a, float b, float *__restrict__ dst)
{
    __shared__ float red[BN_THREADS / 64][2];
    a = bn_wave_sum(a);
    b = bn_wave_sum(b);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = a; red[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    if (threadIdx.x < 2) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < BN_THREADS / 64; ++w) t += red[w][threadIdx.x];
        dst[threadIdx.x] = t;
    }
}

// Batch statistics are accumulated SHIFTED: a slice sums (x - p) and (x - p)^2 around a pivot p = its own first
// element, in fp32, and hands over (s1, s2, p, count); the fp64 pass that adds the slices up rebuilds
// sum x = s1 + n p and sum x^2 = s2 + 2 p s1 + n p^2 exactly.  With plain fp32 sums of x and x^2 the variance
// E[x^2] - mean^2 loses (mean / std)^2 of its digits before any fp64 arithmetic sees them.
// grid (slices, C, B): partial[((b * C + c) * slices + s) * 4 + {0..3}] = s1, s2, pivot, count of the slice
__global__ __launch_bounds__(BN_THREADS) void bn_stats_kernel(int c, int l, const float *__restrict__ x,
                                                              float *__restrict__ partial)
{
    const int bi = blockIdx.z, cc = blockIdx.y;
    const float *row = x + ((size_t)bi * c + cc) * l;
    const int per = (((l + gridDim.x - 1) / gridDim.x) + 3) & ~3;
    const int e0 = blockIdx.x * per, e1 = min(l, e0 + per);
    float s = 0.f, ss = 0.f;
    const float p = e0 < e1 ? row[e0] : 0.f;
    if (e0 >= e1) {
        // empty slice (short rows): contributes zeros
    } else if ((((uintptr_t)row) & 15) == 0) {
        const int v0 = e0 >> 2, v1 = e1 >> 2;
        for (int v = v0 + threadIdx.x; v < v1; v += BN_THREADS) {
            float4 q = reinterpret_cast<const float4 *>(row)[v];
            q.x -= p; q.y -= p; q.z -= p; q.w -= p;
            s += (q.x + q.y) + (q.z + q.w);
            ss = fmaf(q.x, q.x, fmaf(q.y, q.y, fmaf(q.z, q.z, fmaf(q.w, q.w, ss))));
        }
        for (int e = (v1 << 2) + threadIdx.x; e < e1; e += BN_THREADS) { const float d = row[e] - p; s += d; ss = fmaf(d, d, ss); }
    } else {
        for (int e = e0 + threadIdx.x; e < e1; e += BN_THREADS) { const float d = row[e] - p; s += d; ss = fmaf(d, d, ss); }
    }
    float *dst = partial + (((size_t)bi * c + cc) * gridDim.x + blockIdx.x) * 4;
    bn_block_store2(s, ss, dst);
    if (threadIdx.x == 0) { dst[2] = p; dst[3] = (float)max(e1 - e0, 0); }
}

// out = x * scale[c] + shift[c], clamped at 0 when relu (NaN stays NaN: max_nan, geot_common.h); grid (gx, C, B)
__global__ __launch_bounds__(BN_THREADS) void bn_apply_kernel(int c, int l, int relu, const float *__restrict__ x,
                                                              const float *__restrict__ scale,
                                                              const float *__restrict__ shift, float *__restrict__ out)
{
    const int bi = blockIdx.z, cc = blockIdx.y;
    const size_t base = ((size_t)bi * c + cc) * l;
    const float a = scale[cc], b = shift[cc];
    const float lo = relu ? 0.f : -INFINITY;
    if ((((uintptr_t)(x + base) | (uintptr_t)(out + base)) & 15) == 0) {
        const int vec = l >> 2;
        for (int v = blockIdx.x * BN_THREADS + threadIdx.x; v < vec; v += gridDim.x * BN_THREADS) {
            float4 q = reinterpret_cast<const float4 *>(x + base)[v];
            q.x = max_nan(fmaf(q.x, a, b), lo);
            q.y = max_nan(fmaf(q.y, a, b), lo);
            q.z = max_nan(fmaf(q.z, a, b), lo);
            q.w = max_nan(fmaf(q.w, a, b), lo);
            reinterpret_cast<float4 *>(out + base)[v] = q;
        }
        for (int e = (vec << 2) + blockIdx.x * BN_THREADS + threadIdx.x; e < l; e += gridDim.x * BN_THREADS)
            out[base + e] = max_nan(fmaf(x[base + e], a, b), lo);
    } else {
        for (int e = blockIdx.x * BN_THREADS + threadIdx.x; e < l; e += gridDim.x * BN_THREADS)
            out[base + e] = max_nan(fmaf(x[base + e], a, b), lo);
    }
}

// backward reduce: g = dz * [x*scale + shift > 0 or !relu];  partial = (sum g, sum g * xhat),  xhat = (x - mean) rstd
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_reduce_kernel(int c, int l, int relu, const float *__restrict__ x,
                                                                   const float *__restrict__ dz,
                                                                   const float *__restrict__ scale,
                                                                   const float *__restrict__ shift,
                                                                   const float *__restrict__ mean,
                                                                   const float *__restrict__ rstd,
                                                                   float *__restrict__ partial)
{
    const int bi = blockIdx.z, cc = blockIdx.y;
    const size_t base = ((size_t)bi * c + cc) * l;
    const float a = scale[cc], b = shift[cc], mu = mean[cc], r = rstd[cc];
    const int per = (((l + gridDim.x - 1) / gridDim.x) + 3) & ~3;
    const int e0 = blockIdx.x * per, e1 = min(l, e0 + per);
    float s = 0.f, sx = 0.f;
    auto one = [&](float xv, float gv) {
        const float g = (!relu || fmaf(xv, a, b) > 0.f) ? gv : 0.f;
        s += g;
        sx = fmaf(g, (xv - mu) * r, sx);
    };
    if (e0 >= e1) {
        // empty slice
    } else if ((((uintptr_t)(x + base) | (uintptr_t)(dz + base)) & 15) == 0) {
        const int v0 = e0 >> 2, v1 = e1 >> 2;
        for (int v = v0 + threadIdx.x; v < v1; v += BN_THREADS) {
            const float4 q = reinterpret_cast<const float4 *>(x + base)[v];
            const float4 g = reinterpret_cast<const float4 *>(dz + base)[v];
            one(q.x, g.x); one(q.y, g.y); one(q.z, g.z); one(q.w, g.w);
        }
        for (int e = (v1 << 2) + threadIdx.x; e < e1; e += BN_THREADS) one(x[base + e], dz[base + e]);
    } else {
        for (int e = e0 + threadIdx.x; e < e1; e += BN_THREADS) one(x[base + e], dz[base + e]);
    }
    bn_block_store2(s, sx, partial + (((size_t)bi * c + cc) * gridDim.x + blockIdx.x) * 2);
}

// backward apply: dx = k0[c] * (g - c1[c] - xhat * c2[c])   (training: k0 = gamma rstd, c1 = mean(g), c2 = mean(g xhat);
//                                                           eval: k0 = gamma rstd_running, c1 = c2 = 0)
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_apply_kernel(int c, int l, int relu, const float *__restrict__ x,
                                                                  const float *__restrict__ dz,
                                                                  const float *__restrict__ scale,
                                                                  const float *__restrict__ shift,
                                                                  const float *__restrict__ mean,
                                                                  const float *__restrict__ rstd,
                                                                  const float *__restrict__ k0,
                                                                  const float *__restrict__ c1,
                                                                  const float *__restrict__ c2, float *__restrict__ dx)
{
    const int bi = blockIdx.z, cc = blockIdx.y;
    const size_t base = ((size_t)bi * c + cc) * l;
    const float a = scale[cc], b = shift[cc], mu = mean[cc], r = rstd[cc], kk = k0[cc], m1 = c1[cc], m2 = c2[cc];
    auto one = [&](float xv, float gv) {
        const float g = (!relu || fmaf(xv, a, b) > 0.f) ? gv : 0.f;
        return kk * (g - m1 - (xv - mu) * r * m2);
    };
    if ((((uintptr_t)(x + base) | (uintptr_t)(dz + base) | (uintptr_t)(dx + base)) & 15) == 0) {
        const int vec = l >> 2;
        for (int v = blockIdx.x * BN_THREADS + threadIdx.x; v < vec; v += gridDim.x * BN_THREADS) {
            const float4 q = reinterpret_cast<const float4 *>(x + base)[v];
            const float4 g = reinterpret_cast<const float4 *>(dz + base)[v];
            reinterpret_cast<float4 *>(dx + base)[v] = make_float4(one(q.x, g.x), one(q.y, g.y), one(q.z, g.z), one(q.w, g.w));
        }
        for (int e = (vec << 2) + blockIdx.x * BN_THREADS + threadIdx.x; e < l; e += gridDim.x * BN_THREADS)
            dx[base + e] = one(x[base + e], dz[base + e]);
    } else {
        for (int e = blockIdx.x * BN_THREADS + threadIdx.x; e < l; e += gridDim.x * BN_THREADS)
            dx[base + e] = one(x[base + e], dz[base + e]);
    }
}

// ---- the four passes over x + seg[.., e / n]: a per-(batch, channel, segment) addend, never added in memory ---------------
// (the Encoder's second BatchNorm: x = W_f . per-point features, seg = W_g . pooled, n points per group.)  l % n == 0 and
// n % 4 == 0: a float4 of a row lies in ONE segment; the segment is found from the ABSOLUTE column, so a slice boundary may
// fall inside one.  Rows are 16-byte aligned (the launchers check): float4 traffic only.
__global__ __launch_bounds__(BN_THREADS) void bn_stats_seg_kernel(int c, int l, int n, const float *__restrict__ x,
                                                                  const float *__restrict__ seg, float *__restrict__ partial)
{
    const int bi = blockIdx.z, cc = blockIdx.y;
    const size_t rowi = (size_t)bi * c + cc;
    const float *row = x + rowi * l;
    const float *srow = seg + rowi * (l / n);
    const int per = (((l + gridDim.x - 1) / gridDim.x) + 3) & ~3;
    const int e0 = blockIdx.x * per, e1 = min(l, e0 + per);
    float s = 0.f, ss = 0.f;
    const float p = e0 < e1 ? row[e0] + srow[e0 / n] : 0.f;
    for (int v = (e0 >> 2) + threadIdx.x; v < (e1 >> 2); v += BN_THREADS) {
        float4 q = reinterpret_cast<const float4 *>(row)[v];
        const float a = srow[(unsigned)(v << 2) / (unsigned)n];
        q.x = (q.x + a) - p; q.y = (q.y + a) - p; q.z = (q.z + a) - p; q.w = (q.w + a) - p;
        s += (q.x + q.y) + (q.z + q.w);
        ss = fmaf(q.x, q.x, fmaf(q.y, q.y, fmaf(q.z, q.z, fmaf(q.w, q.w, ss))));
    }
    float *dst = partial + (rowi * gridDim.x + blockIdx.x) * 4;
    bn_block_store2(s, ss, dst);
    if (threadIdx.x == 0) { dst[2] = p; dst[3] = (float)max(e1 - e0, 0); }
}

__global__ __launch_bounds__(BN_THREADS) void bn_apply_seg_kernel(int c, int l, int n, int relu, const float *__restrict__ x,
                                                                  const float *__restrict__ seg, const float *__restrict__ scale,
                                                                  const float *__restrict__ shift, float *__restrict__ out)
{
    const int bi = blockIdx.z, cc = blockIdx.y;
    const size_t rowi = (size_t)bi * c + cc;
    const size_t base = rowi * l;
    const float *srow = seg + rowi * (l / n);
    const float a = scale[cc], b = shift[cc];
    const float lo = relu ? 0.f : -INFINITY;
    const int vec = l >> 2;
    for (int v = blockIdx.x * BN_THREADS + threadIdx.x; v < vec; v += gridDim.x * BN_THREADS) {
        float4 q = reinterpret_cast<const float4 *>(x + base)[v];
        const float t = srow[(unsigned)(v << 2) / (unsigned)n];
        q.x = max_nan(fmaf(q.x + t, a, b), lo);
        q.y = max_nan(fmaf(q.y + t, a, b), lo);
        q.z = max_nan(fmaf(q.z + t, a, b), lo);
        q.w = max_nan(fmaf(q.w + t, a, b), lo);
        reinterpret_cast<float4 *>(out + base)[v] = q;
    }
}

__global__ __launch_bounds__(BN_THREADS) void bn_bwd_reduce_seg_kernel(int c, int l, int n, int relu, const float *__restrict__ x,
                                                                       const float *__restrict__ seg,
                                                                       const float *__restrict__ dz,
                                                                       const float *__restrict__ scale,
                                                                       const float *__restrict__ shift,
                                                                       const float *__restrict__ mean,
                                                                       const float *__restrict__ rstd,
                                                                       double *__restrict__ partial)
{
    const int bi = blockIdx.z, cc = blockIdx.y;
    const size_t rowi = (size_t)bi * c + cc;
    const size_t base = rowi * l;
    const float *srow = seg + rowi * (l / n);
    const float a = scale[cc], b = shift[cc], mu = mean[cc], r = rstd[cc];
    const int per = (((l + gridDim.x - 1) / gridDim.x) + 3) & ~3;
    const int e0 = blockIdx.x * per, e1 = min(l, e0 + per);
    // the sums are carried in fp64 from the first add: sum g of a single channel is a sum of terms of both signs, and what
    // fp32 partial sums round away (an ulp of their own size each) can exceed 2e-5 of a result that cancelled
    double s = 0.0, sx = 0.0;
    auto one = [&](float xv, float gv) {
        const float g = (!relu || fmaf(xv, a, b) > 0.f) ? gv : 0.f;
        s += (double)g;
        sx = fma((double)g, (double)((xv - mu) * r), sx);
    };
    for (int v = (e0 >> 2) + threadIdx.x; v < (e1 >> 2); v += BN_THREADS) {
        const float4 q = reinterpret_cast<const float4 *>(x + base)[v];
        const float4 g = reinterpret_cast<const float4 *>(dz + base)[v];
        const float t = srow[(unsigned)(v << 2) / (unsigned)n];
        one(q.x + t, g.x); one(q.y + t, g.y); one(q.z + t, g.z); one(q.w + t, g.w);
    }
    __shared__ double red[BN_THREADS / 64][2];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s += __shfl_xor(s, d);
        sx += __shfl_xor(sx, d);
    }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = s; red[threadIdx.x >> 6][1] = sx; }
    __syncthreads();
    if (threadIdx.x < 2)
        partial[(rowi * gridDim.x + blockIdx.x) * 2 + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// backward apply + the addend's gradient: rows = (b, c, segment) of n elements, LPR adjacent lanes of one wave per row (as
// segment_sum_kernel); dseg[row] = the row's sum of dx: lane sub-sums, then a butterfly -- one writer, fixed order
template <int LPR>
__global__ __launch_bounds__(256) void bn_bwd_apply_seg_kernel(long long rows, int n, int groups, int c, int relu,
                                                               const float *__restrict__ x, const float *__restrict__ seg,
                                                               const float *__restrict__ dz, const float *__restrict__ scale,
                                                               const float *__restrict__ shift, const float *__restrict__ mean,
                                                               const float *__restrict__ rstd, const float *__restrict__ k0,
                                                               const float *__restrict__ c1, const float *__restrict__ c2,
                                                               float *__restrict__ dx, float *__restrict__ dseg)
{
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = gid / LPR;
    const int sub = (int)(gid % LPR);
    if (row >= rows) return;                               // (LPR divides 64 and rows are whole lane groups: no partial group)
    const int cc = (int)((row / groups) % c);
    const float a = scale[cc], b = shift[cc], mu = mean[cc], r = rstd[cc], kk = k0[cc], m1 = c1[cc], m2 = c2[cc];
    const float t = seg[row];
    auto one = [&](float xv, float gv) {
        xv += t;
        const float g = (!relu || fmaf(xv, a, b) > 0.f) ? gv : 0.f;
        return kk * (g - m1 - (xv - mu) * r * m2);
    };
    const float4 *xs = reinterpret_cast<const float4 *>(x + row * n);
    const float4 *gs = reinterpret_cast<const float4 *>(dz + row * n);
    float4 *ds = reinterpret_cast<float4 *>(dx + row * n);
    float s = 0.f;
    for (int v = sub; v < (n >> 2); v += LPR) {
        const float4 q = xs[v], g = gs[v];
        const float4 d = make_float4(one(q.x, g.x), one(q.y, g.y), one(q.z, g.z), one(q.w, g.w));
        ds[v] = d;
        s += (d.x + d.y) + (d.z + d.w);
    }
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) s += __shfl_xor(s, o);
    if (sub == 0) dseg[row] = s;
}

// ---- the thin first stage: act(bn(W x)) for x (J, l), J <= 8, W (c, J); y = W x is never stored ---------------------------
// thin_y / thin_z are THE definitions of y and of the pre-activation: the apply pass and the backward pass both call them,
// so they agree on every bit, hence on every ReLU mask.  y is the fp64 dot product rounded once (J <= 8 fp64 fmas per element
// are nothing beside the 4 bytes it is not stored in): it then differs from the exact w x, whose mean the moments give, by
// half an ulp -- and not at all in the mean of a single column, where z = (y - mean) scale + beta is exactly beta although
// scale = gamma / sqrt(eps) (y scale + shift would lose |y| scale / 2^24 there).
template <int J>
__device__ __forceinline__ double thin_yd(const float (&w)[J], const float (&xv)[J])
{
    double y = (double)w[0] * (double)xv[0];
#pragma unroll
    for (int j = 1; j < J; ++j) y = fma((double)w[j], (double)xv[j], y);
    return y;
}
template <int J>
__device__ __forceinline__ float thin_y(const float (&w)[J], const float (&xv)[J]) { return (float)thin_yd<J>(w, xv); }
__device__ __forceinline__ float thin_z(float y, float mu, float a, float be) { return fmaf(y - mu, a, be); }

constexpr int THIN_MOM_THREADS = 256;
// partial[slice][0 .. J) = sum x'_i, [J + i J + k] = sum x'_i x'_k (both triangles written), x' = x - x[:, 0], in fp64
template <int J>
__global__ __launch_bounds__(THIN_MOM_THREADS) void thin_moments_kernel(int l, const float *__restrict__ x, double *__restrict__ partial)
{
    constexpr int K = J + J * (J + 1) / 2;
    const int per = (l + gridDim.x - 1) / gridDim.x;
    const int e0 = blockIdx.x * per, e1 = min(l, e0 + per);
    double p[J], acc[K];
#pragma unroll
    for (int j = 0; j < J; ++j) p[j] = (double)x[(size_t)j * l];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (int e = e0 + threadIdx.x; e < e1; e += THIN_MOM_THREADS) {
        double d[J];
#pragma unroll
        for (int j = 0; j < J; ++j) d[j] = (double)x[(size_t)j * l + e] - p[j];
        int k = J;
#pragma unroll
        for (int i = 0; i < J; ++i) {
            acc[i] += d[i];
#pragma unroll
            for (int m = i; m < J; ++m, ++k) acc[k] = fma(d[i], d[m], acc[k]);
        }
    }
    __shared__ double red[THIN_MOM_THREADS / 64][K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *dst = partial + (size_t)blockIdx.x * (J + J * J);
        int k = J;
        for (int i = 0; i < J; ++i) {
            dst[i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
            for (int m = i; m < J; ++m, ++k) {
                const double v = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
                dst[J + i * J + m] = v;
                dst[J + m * J + i] = v;
            }
        }
    }
}

// every block adds the slices up in a fixed order (thread t < J + J J owns one moment), block 0 writes mom = p, sum x',
// sum x' x'^T; then one thread per channel: s1 = w . sum x', s2 = w (sum x' x'^T) w^T about q = w . p, and
// sum y = s1 + l q, sum y^2 = s2 + 2 q s1 + l q^2 as bn_sums_shifted_kernel rebuilds them
__global__ __launch_bounds__(256) void thin_bn_sums_kernel(int c, int j, int l, int s, const double *__restrict__ partial,
                                                           const float *__restrict__ w, const float *__restrict__ x,
                                                           double *__restrict__ mom, double *__restrict__ sums)
{
    __shared__ double m[8 + 64], p[8];
    const int k = j + j * j;
    if ((int)threadIdx.x < k) {
        double a = 0.0;
        for (int t = 0; t < s; ++t) a += partial[(size_t)t * k + threadIdx.x];
        m[threadIdx.x] = a;
        if (blockIdx.x == 0) mom[j + threadIdx.x] = a;
    }
    if ((int)threadIdx.x < j) {
        p[threadIdx.x] = (double)x[(size_t)threadIdx.x * l];
        if (blockIdx.x == 0) mom[threadIdx.x] = p[threadIdx.x];
    }
    __syncthreads();
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= c) return;
    double q = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < j; ++i) {
        const double wi = (double)w[(size_t)ch * j + i];
        q += wi * p[i];
        s1 += wi * m[i];
        double t = 0.0;
        for (int u = 0; u < j; ++u) t += (double)w[(size_t)ch * j + u] * m[j + i * j + u];
        s2 += wi * t;
    }
    const double n = (double)l;
    sums[2 * ch] = s1 + n * q;
    sums[2 * ch + 1] = s2 + 2.0 * q * s1 + n * q * q;
}

constexpr int THIN_CH = 8;       // channels per workgroup of the apply pass: x's float4s are loaded once for all of them
// grid (gx, ceil(c / THIN_CH)); l % 4 == 0 and aligned tensors take float4s (vec4 != 0), anything else scalars
template <int J>
__global__ __launch_bounds__(BN_THREADS) void thin_bn_apply_kernel(int c, int l, int relu, int vec4, const float *__restrict__ w,
                                                                   const float *__restrict__ x, const float *__restrict__ mean,
                                                                   const float *__restrict__ scale, const float *__restrict__ beta,
                                                                   float *__restrict__ out)
{
    const int c0 = blockIdx.y * THIN_CH, nch = min(THIN_CH, c - c0);
    const float lo = relu ? 0.f : -INFINITY;
    if (vec4) {
        for (int v = blockIdx.x * BN_THREADS + threadIdx.x; v < (l >> 2); v += gridDim.x * BN_THREADS) {
            float xv[4][J];
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const float4 q = reinterpret_cast<const float4 *>(x + (size_t)j * l)[v];
                xv[0][j] = q.x; xv[1][j] = q.y; xv[2][j] = q.z; xv[3][j] = q.w;
            }
            for (int cl = 0; cl < nch; ++cl) {
                float wr[J];
#pragma unroll
                for (int j = 0; j < J; ++j) wr[j] = w[(size_t)(c0 + cl) * J + j];
                const float mu = mean[c0 + cl], a = scale[c0 + cl], b = beta[c0 + cl];
                reinterpret_cast<float4 *>(out + (size_t)(c0 + cl) * l)[v] =
                    make_float4(max_nan(thin_z(thin_y<J>(wr, xv[0]), mu, a, b), lo), max_nan(thin_z(thin_y<J>(wr, xv[1]), mu, a, b), lo),
                                max_nan(thin_z(thin_y<J>(wr, xv[2]), mu, a, b), lo), max_nan(thin_z(thin_y<J>(wr, xv[3]), mu, a, b), lo));
            }
        }
    } else {
        for (int e = blockIdx.x * BN_THREADS + threadIdx.x; e < l; e += gridDim.x * BN_THREADS) {
            float xv[J];
#pragma unroll
            for (int j = 0; j < J; ++j) xv[j] = x[(size_t)j * l + e];
            for (int cl = 0; cl < nch; ++cl) {
                float wr[J];
#pragma unroll
                for (int j = 0; j < J; ++j) wr[j] = w[(size_t)(c0 + cl) * J + j];
                out[(size_t)(c0 + cl) * l + e] = max_nan(thin_z(thin_y<J>(wr, xv), mean[c0 + cl], scale[c0 + cl], beta[c0 + cl]), lo);
            }
        }
    }
}

// backward: ONE pass over dz (c, l) and x: per (channel, slice) sum g, sum g xhat, sum g x_j; y through thin_y.
// grid (S, c); partial[(ch * S + slice) * (2 + J) + {0, 1, 2 + j}], fp64.  The sums g x_j are ACCUMULATED in fp64 (a product
// of two floats is exact there): the weight gradient subtracts c1 sum x_j from them, which cancels most of both when the
// columns are few or alike -- all of both for a single column, where the gradient is exactly zero.  sum g and sum g xhat are
// carried in fp64 too: c1 = sum g / l multiplies sum x_j there, (mean / std of x) l times larger than what is left.
template <int J>
__global__ __launch_bounds__(BN_THREADS) void thin_bn_bwd_reduce_kernel(int l, int relu, int vec4, const double *__restrict__ mom,
                                                                        const float *__restrict__ w,
                                                                        const float *__restrict__ x, const float *__restrict__ dz,
                                                                        const float *__restrict__ scale,
                                                                        const float *__restrict__ beta,
                                                                        const float *__restrict__ mean,
                                                                        const float *__restrict__ rstd, double *__restrict__ partial)
{
    constexpr int K = 2 + J;
    const int cc = blockIdx.y;
    const float *grow = dz + (size_t)cc * l;
    const float a = scale[cc], b = beta[cc], mu = mean[cc], r = rstd[cc];
    float wr[J];
    double s = 0.0, sx = 0.0, acc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) { wr[j] = w[(size_t)cc * J + j]; acc[j] = 0.0; }
    // xhat for the SUMS in fp64, from the unrounded y and -- where the statistics were this rank's alone (mom given) -- about
    // their exact mean w . (p + S / l): the fp32 mean[c] misses it by up to |mean| 2^-25, which sum g xhat would collect l times
    double mud = (double)mu;
    if (mom) {
        mud = 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j) mud += (double)wr[j] * (mom[j] + mom[J + j] / (double)l);
    }
    const double rd = (double)r;
    const int per = (((l + gridDim.x - 1) / gridDim.x) + 3) & ~3;
    const int e0 = blockIdx.x * per, e1 = min(l, e0 + per);
    auto one = [&](const float (&xv)[J], float gv) {
        const double yd = thin_yd<J>(wr, xv);
        const float g = (!relu || thin_z((float)yd, mu, a, b) > 0.f) ? gv : 0.f;
        s += (double)g;
        sx = fma((double)g, (yd - mud) * rd, sx);
#pragma unroll
        for (int j = 0; j < J; ++j) acc[j] = fma((double)g, (double)xv[j], acc[j]);
    };
    int tail = e0 + threadIdx.x;                           // first element the scalar loop takes
    if (vec4) {
        const int v1 = e1 >> 2;
        for (int v = (e0 >> 2) + threadIdx.x; v < v1; v += BN_THREADS) {
            float xv[4][J];
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const float4 q = reinterpret_cast<const float4 *>(x + (size_t)j * l)[v];
                xv[0][j] = q.x; xv[1][j] = q.y; xv[2][j] = q.z; xv[3][j] = q.w;
            }
            const float4 g = reinterpret_cast<const float4 *>(grow)[v];
            one(xv[0], g.x); one(xv[1], g.y); one(xv[2], g.z); one(xv[3], g.w);
        }
        tail = (v1 << 2) + threadIdx.x;
    }
    for (int e = tail; e < e1; e += BN_THREADS) {
        float xv[J];
#pragma unroll
        for (int j = 0; j < J; ++j) xv[j] = x[(size_t)j * l + e];
        one(xv, grow[e]);
    }
    __shared__ double red[BN_THREADS / 64][K];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        s += __shfl_xor(s, o);
        sx += __shfl_xor(sx, o);
    }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = s; red[threadIdx.x >> 6][1] = sx; }
#pragma unroll
    for (int j = 0; j < J; ++j) {
        double v = acc[j];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][2 + j] = v;
    }
    __syncthreads();
    if (threadIdx.x < K)
        partial[((size_t)cc * gridDim.x + blockIdx.x) * K + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// one thread per (channel, sum): the S slice partials added in fp64, ascending
__global__ __launch_bounds__(256) void thin_bn_bwd_sums_kernel(int c, int j, int s, const double *__restrict__ partial,
                                                               double *__restrict__ local, double *__restrict__ gx)
{
    const int k = 2 + j, t = blockIdx.x * 256 + threadIdx.x;
    if (t >= c * k) return;
    const int ch = t / k, q = t - ch * k;
    double a = 0.0;
    for (int u = 0; u < s; ++u) a += partial[((size_t)ch * s + u) * k + q];
    if (q < 2) local[2 * ch + q] = a;
    else gx[(size_t)ch * j + q - 2] = a;
}

// dw[c][i] = scale_c (gx[c][i] - c1_c sum x_i - c2_c sum xhat_c x_i), everything in fp64: c1, c2 = sums / n (the all-reduced
// sum g, sum g xhat; n = 0: running statistics, dw = scale gx) -- NOT their fp32 roundings: the three terms cancel by a
// factor (mean / std of x)^2.  From the moments about the pivot p, with x' = x - p and d = w . p - mu:
//   sum x_i = S_i + l p_i,   sum (y - mu) x_i = sum (w . x' + d) (x'_i + p_i) = w . M_i + p_i (w . S) + d (S_i + l p_i)
// mu = the mean the statistics were taken with: w . (p + S / l) exactly when they are this rank's alone (local_mean),
// else (SyncBatchNorm over several ranks) its fp32 value mean[c] -- as thin_bn_bwd_reduce_kernel took it for sum g xhat.
__global__ __launch_bounds__(256) void thin_bn_wgrad_kernel(int c, int j, int l, int local_mean, const float *__restrict__ w,
                                                            const double *__restrict__ mom, const double *__restrict__ gx,
                                                            const double *__restrict__ sums, double count,
                                                            const double *__restrict__ count_dev,
                                                            const float *__restrict__ scale, const float *__restrict__ mean,
                                                            const float *__restrict__ rstd, float *__restrict__ dw)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= c * j) return;
    const int ch = t / j, i = t - ch * j;
    double v = gx[t];
    const double cnt = count_dev ? *count_dev : count;
    if (mom && cnt > 0.0) {
        const double n = (double)l;
        const double *p = mom, *s1 = mom + j, *m2 = mom + 2 * j;
        double q = 0.0, ws = 0.0, wm = 0.0;
        for (int u = 0; u < j; ++u) {
            const double wu = (double)w[(size_t)ch * j + u];
            q += wu * p[u];
            ws += wu * s1[u];
            wm += wu * m2[u * j + i];
        }
        const double mu = local_mean ? q + ws / n : (double)mean[ch];
        const double d = q - mu, sxi = s1[i] + n * p[i];
        const double yx = wm + p[i] * ws + d * sxi;
        v -= (sums[2 * ch] / cnt) * sxi + (sums[2 * ch + 1] / cnt) * ((double)rstd[ch] * yx);
    }
    dw[t] = (float)((double)scale[ch] * v);
}

// ---- FP front end: y[b,c,e] = sum_t w[e,t] A[b,c,idx[e,t]] + sum_k Wb[c,k] skip[b,k,e], + its BatchNorm sums -----
// (the first SharedMLP stage of a PointnetFPModule with the 1x1 convolution moved in front of the interpolation:
// A = W_a known_feats; pointnet2_modules.py:619-640).  CH rows of A in LDS, queries streamed, 2 elements per thread in
// flight; per-(b, c, slice) partial sums of y and y^2 leave with the result, so the BatchNorm needs no pass of its own.
constexpr int FP_THREADS = 1024;
constexpr int FP_LDS_BYTES = 144 * 1024;
constexpr int FP_MAX_SKIP = 8;

template <int CH>
__global__ __launch_bounds__(FP_THREADS) void fp_front_kernel(int c, int m, int n, int cs, const float *__restrict__ A,
                                                              const int *__restrict__ idx, const float *__restrict__ w,
                                                              const float *__restrict__ skip, const float *__restrict__ Wb,
                                                              float *__restrict__ y, float *__restrict__ partial)
{
    extern __shared__ float fp_rows[]; // [CH][m]
    __shared__ float wb[CH][FP_MAX_SKIP];
    __shared__ float red[FP_THREADS / 64][CH][2];
    const int bi = blockIdx.z, c0 = blockIdx.y * CH, nch = min(CH, c - c0);
    {
        const float *src = A + ((size_t)bi * c + c0) * m;
        const int count = nch * m;
        if ((((uintptr_t)src) & 15) == 0) {
            const int vec = count >> 2;
            for (int v = threadIdx.x; v < vec; v += FP_THREADS) reinterpret_cast<float4 *>(fp_rows)[v] = reinterpret_cast<const float4 *>(src)[v];
            for (int e = (vec << 2) + threadIdx.x; e < count; e += FP_THREADS) fp_rows[e] = src[e];
        } else {
            for (int e = threadIdx.x; e < count; e += FP_THREADS) fp_rows[e] = src[e];
        }
    }
    if (threadIdx.x < CH * FP_MAX_SKIP) {
        const int l = threadIdx.x / FP_MAX_SKIP, k = threadIdx.x % FP_MAX_SKIP;
        wb[l][k] = (l < nch && k < cs) ? Wb[(size_t)(c0 + l) * cs + k] : 0.f;
    }
    __syncthreads();
    const int per = (n + gridDim.x - 1) / gridDim.x;
    const int e0 = blockIdx.x * per, e1 = min(n, e0 + per);
    float s[CH], ss[CH], piv[CH];
#pragma unroll
    for (int l = 0; l < CH; ++l) s[l] = ss[l] = piv[l] = 0.f;
    if (e0 < e1) {   // pivot of the shifted sums (see bn_stats_kernel): the slice's first value, formed by every thread
        int i3[3];
        float w3[3], sk0[FP_MAX_SKIP];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            i3[t] = idx[((size_t)bi * n + e0) * 3 + t];
            w3[t] = w[((size_t)bi * n + e0) * 3 + t];
        }
#pragma unroll
        for (int k = 0; k < FP_MAX_SKIP; ++k) sk0[k] = k < cs ? skip[((size_t)bi * cs + k) * n + e0] : 0.f;
#pragma unroll
        for (int l = 0; l < CH; ++l) {
            if (l < nch) {
                const float *R = fp_rows + (size_t)l * m;
                float v = R[i3[0]] * w3[0];
                v = v + R[i3[1]] * w3[1];
                v = v + R[i3[2]] * w3[2];
#pragma unroll
                for (int k = 0; k < FP_MAX_SKIP; ++k) v = fmaf(wb[l][k], sk0[k], v);
                piv[l] = v;
            }
        }
    }
    constexpr int U = 2;
    for (int eb = e0 + threadIdx.x; eb < e1; eb += U * FP_THREADS) {
        int ii[U][3];
        float ww[U][3], sk[U][FP_MAX_SKIP];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = eb + u * FP_THREADS;
            const bool ok = e < e1;
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                ii[u][t] = ok ? idx[((size_t)bi * n + e) * 3 + t] : 0;
                ww[u][t] = ok ? w[((size_t)bi * n + e) * 3 + t] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < FP_MAX_SKIP; ++k) sk[u][k] = (ok && k < cs) ? skip[((size_t)bi * cs + k) * n + e] : 0.f;
        }
#pragma unroll
        for (int l = 0; l < CH; ++l) {
            if (l < nch) {
                const float *R = fp_rows + (size_t)l * m;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int e = eb + u * FP_THREADS;
                    float v = R[ii[u][0]] * ww[u][0];
                    v = v + R[ii[u][1]] * ww[u][1];
                    v = v + R[ii[u][2]] * ww[u][2];           // ((p0 w0 + p1 w1) + p2 w2): three_interpolate's order
#pragma unroll
                    for (int k = 0; k < FP_MAX_SKIP; ++k) v = fmaf(wb[l][k], sk[u][k], v);
                    if (e < e1) {
                        y[((size_t)bi * c + c0 + l) * n + e] = v;
                        const float d = v - piv[l];
                        s[l] += d;
                        ss[l] = fmaf(d, d, ss[l]);
                    }
                }
            }
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int l = 0; l < CH; ++l) {
        const float a = bn_wave_sum(s[l]), b = bn_wave_sum(ss[l]);
        if (lane == 0) { red[wave][l][0] = a; red[wave][l][1] = b; }
    }
    __syncthreads();
    if (threadIdx.x < 2 * CH) {
        const int l = threadIdx.x >> 1, q = threadIdx.x & 1;
        if (l < nch) {
            float t = 0.f;
            for (int v = 0; v < FP_THREADS / 64; ++v) t += red[v][l][q];
            float *dst = partial + (((size_t)bi * c + c0 + l) * gridDim.x + blockIdx.x) * 4;
            dst[q] = t;
            dst[2 + q] = q == 0 ? piv[l] : (float)max(e1 - e0, 0);       // (s1, s2, pivot, count)
        }
    }
}

// ---- max over the n innermost (contiguous) elements of every row: (rows, n) -> (rows,) + the arg-max slot ----------
// (the "max over the group's points" of the mini-PointNet Encoder, transformer.py:127-134, and the "max over nsample" of
// the SetAbstraction modules, pointnet2_modules.py:62-66.)  torch's generic reduction reaches 0.5 TB/s on 32-element
// rows; this is a plain stream: LPR lanes share a row with one float4 each per step, first maximum wins (torch.max).
// (value, slot) a beats (value, slot) b: NaN beats every number (torch.max propagates NaN), the earlier slot wins ties
__device__ __forceinline__ bool seg_better(float a, int ja, float b, int jb)
{
    const bool an = a != a, bn = b != b;
    if (an || bn) return an && (!bn || ja < jb);
    return a > b || (a == b && ja < jb);
}
template <int LPR>
__global__ __launch_bounds__(256) void segment_max_kernel(long long rows, int n, const float *__restrict__ x,
                                                          float *__restrict__ out, uint8_t *__restrict__ arg)
{
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = gid / LPR;
    const int sub = (int)(gid % LPR);
    if (row >= rows) return;
    const float4 *src = reinterpret_cast<const float4 *>(x + row * n);
    float best = -INFINITY;
    int bj = 0x7fffffff;
    for (int v = sub; v < (n >> 2); v += LPR) {
        const float4 q = src[v];
        const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = 4 * v + u;
            const bool take = seg_better(e[u], j, best, bj);
            best = take ? e[u] : best;
            bj = take ? j : bj;
        }
    }
#pragma unroll
    for (int d = 1; d < LPR; d <<= 1) {                       // the LPR lanes of a row are adjacent lanes of one wave
        const float ob = __shfl_xor(best, d);
        const int oj = __shfl_xor(bj, d);
        const bool take = seg_better(ob, oj, best, bj);
        best = take ? ob : best;
        bj = take ? oj : bj;
    }
    if (sub == 0) {
        out[row] = best;
        arg[row] = (uint8_t)(bj == 0x7fffffff ? 0 : bj);
    }
}
// out[row] = sum of the row's n elements: fixed order (lane sub-sums, then a butterfly), LPR adjacent lanes per row
template <int LPR>
__global__ __launch_bounds__(256) void segment_sum_kernel(long long rows, int n, const float *__restrict__ x,
                                                          float *__restrict__ out)
{
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = gid / LPR;
    const int sub = (int)(gid % LPR);
    if (row >= rows) return;
    const float4 *src = reinterpret_cast<const float4 *>(x + row * n);
    float s = 0.f;
    for (int v = sub; v < (n >> 2); v += LPR) {
        const float4 q = src[v];
        s += (q.x + q.y) + (q.z + q.w);
    }
#pragma unroll
    for (int d = 1; d < LPR; d <<= 1) s += __shfl_xor(s, d);
    if (sub == 0) out[row] = s;
}
// partial[(row * S + slice) * J + j] = sum over the slice of a[row][l] * b[j][l], J <= 8 rows of b: the weight gradient of
// a 1x1 convolution with a handful of input channels (the Encoder's Conv1d(3, 128) over 131 072 columns is a
// 128 x 3 x 131072 GEMM to the libraries: 436 us; this streams the 67 MB once)
template <int J>
__global__ __launch_bounds__(256) void rowdot_small_kernel(int l, const float *__restrict__ a, const float *__restrict__ b,
                                                           float *__restrict__ partial)
{
    const int row = blockIdx.y, per = (((l + gridDim.x - 1) / gridDim.x) + 3) & ~3;
    const int e0 = blockIdx.x * per, e1 = min(l, e0 + per);
    const float *ar = a + (size_t)row * l;
    float acc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) acc[j] = 0.f;
    for (int e = e0 + threadIdx.x; e < e1; e += 256) {
        const float v = ar[e];
#pragma unroll
        for (int j = 0; j < J; ++j) acc[j] = fmaf(v, b[(size_t)j * l + e], acc[j]);
    }
    __shared__ float sh[J][4];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        float v = acc[j];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) sh[j][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < J)
        partial[((size_t)row * gridDim.x + blockIdx.x) * J + threadIdx.x] =
            (sh[threadIdx.x][0] + sh[threadIdx.x][1]) + (sh[threadIdx.x][2] + sh[threadIdx.x][3]);
}
// Column sums of a row-major (rows, cols) matrix -- the bias gradient of a Linear layer (grad_output.sum(0); torch's
// generic reduction takes 19 us + a 5 us fill for (4096, 384)).  grid (col blocks of 64, S row slices): a wave reads 64
// consecutive columns of a row (256 B), the block's 4 waves take every 4th row of the slice; partial (S, cols).
__global__ __launch_bounds__(256) void colsum_kernel(int rows, int cols, const float *__restrict__ x, float *__restrict__ partial)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;
    const int per = (rows + gridDim.y - 1) / gridDim.y;
    const int r0 = blockIdx.y * per, r1 = min(rows, r0 + per);
    float s0 = 0.f;
    if (col < cols) {
        int r = r0 + wave;
        for (; r + 28 < r1; r += 32) {                     // eight rows in flight per wave (the pass is latency-bound)
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = x[(size_t)(r + 4 * u) * cols + col];
#pragma unroll
            for (int u = 0; u < 8; ++u) s0 += v[u];
        }
        for (; r < r1; r += 4) s0 += x[(size_t)r * cols + col];
    }
    __shared__ float sh[4][64];
    sh[wave][lane] = s0;
    __syncthreads();
    if (wave == 0 && col < cols) partial[(size_t)blockIdx.y * cols + col] = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
}
__global__ __launch_bounds__(256) void colsum_finish_kernel(int s, int cols, const float *__restrict__ partial, float *__restrict__ out)
{
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= cols) return;
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = i < s ? partial[(size_t)i * cols + col] : 0.f;   // independent loads, then a fixed order
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) a += v[i];
    out[col] = a;
}
// ---- BatchNorm -> ReLU -> max over the n innermost elements, without materialising the normalised tensor ---------------
// max_j relu(a y_j + b) = relu(a sel + b) with sel = max_j y_j if a >= 0 else min_j y_j (the affine map is monotone): the
// last stage of a SetAbstraction module in training mode (pointnet2_modules.py:57-66: SharedMLP then max_pool2d over
// nsample).  Forward: rows = (b, c, group) of n elements; out = relu(a_c sel + b_c), sel, arg = slot of the first
// extremum.  Backward: the gradient of the (never built) normalised tensor is g at arg (if the pre-activation was
// positive) and 0 elsewhere, so  dx_j = k0_c ([j == arg] gm - c1_c - xhat_j c2_c)  in one pass over y.
template <int LPR>
__global__ __launch_bounds__(256) void bn_pool_kernel(long long rows, int n, int groups, int c, int relu,
                                                      const float *__restrict__ y, const float *__restrict__ scale,
                                                      const float *__restrict__ shift, float *__restrict__ out,
                                                      float *__restrict__ sel_out, uint8_t *__restrict__ arg)
{
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = gid / LPR;
    const int sub = (int)(gid % LPR);
    if (row >= rows) return;
    const int cc = (int)((row / groups) % c);
    const float a = scale[cc];
    const float sgn = a >= 0.f ? 1.f : -1.f;               // max of sgn * y: the maximum, or the minimum
    const float4 *src = reinterpret_cast<const float4 *>(y + row * n);
    float best = -INFINITY;
    int bj = 0x7fffffff;
    for (int v = sub; v < (n >> 2); v += LPR) {
        const float4 q = src[v];
        const float e[4] = {sgn * q.x, sgn * q.y, sgn * q.z, sgn * q.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = 4 * v + u;
            const bool take = seg_better(e[u], j, best, bj);
            best = take ? e[u] : best;
            bj = take ? j : bj;
        }
    }
#pragma unroll
    for (int d = 1; d < LPR; d <<= 1) {
        const float ob = __shfl_xor(best, d);
        const int oj = __shfl_xor(bj, d);
        const bool take = seg_better(ob, oj, best, bj);
        best = take ? ob : best;
        bj = take ? oj : bj;
    }
    if (sub == 0) {
        float sv = sgn * best;
        if (a == 0.f) {                                    // every slot ties at relu(b): the reference's max takes the first
            bj = 0;
            sv = y[row * n];
        }
        const float z = fmaf(sv, a, shift[cc]);
        out[row] = relu ? max_nan(z, 0.f) : z;             // (a NaN stays a NaN, as the reference's relu keeps it)
        sel_out[row] = sv;
        arg[row] = (uint8_t)(bj == 0x7fffffff ? 0 : bj);
    }
}
__global__ __launch_bounds__(256) void bn_pool_bwd_kernel(long long total4, int n4, int groups, int c,
                                                          const float *__restrict__ y, const float *__restrict__ gm,
                                                          const uint8_t *__restrict__ arg, const float *__restrict__ mean,
                                                          const float *__restrict__ rstd, const float *__restrict__ k0,
                                                          const float *__restrict__ c1, const float *__restrict__ c2,
                                                          float *__restrict__ dx)
{
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < total4; v += (long long)gridDim.x * 256) {
        const long long row = v / n4;
        const int cc = (int)((row / groups) % c);
        const int j0 = (int)(v - row * n4) * 4, a = arg[row];
        const float g = gm[row], mu = mean[cc], r = rstd[cc], kk = k0[cc], m1 = c1[cc], m2 = c2[cc];
        const float4 q = reinterpret_cast<const float4 *>(y)[v];
        reinterpret_cast<float4 *>(dx)[v] =
            make_float4(kk * ((a == j0 ? g : 0.f) - m1 - (q.x - mu) * r * m2), kk * ((a == j0 + 1 ? g : 0.f) - m1 - (q.y - mu) * r * m2),
                        kk * ((a == j0 + 2 ? g : 0.f) - m1 - (q.z - mu) * r * m2), kk * ((a == j0 + 3 ? g : 0.f) - m1 - (q.w - mu) * r * m2));
    }
}
// dx (rows, n) = dy[row] at the arg-max slot, 0 elsewhere (written in full)
__global__ __launch_bounds__(256) void segment_max_grad_kernel(long long total4, int n4, const float *__restrict__ dy,
                                                               const uint8_t *__restrict__ arg, float *__restrict__ dx)
{
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < total4; v += (long long)gridDim.x * 256) {
        const long long row = v / n4;
        const int j0 = (int)(v - row * n4) * 4, a = arg[row];
        const float g = dy[row];
        reinterpret_cast<float4 *>(dx)[v] = make_float4(a == j0 ? g : 0.f, a == j0 + 1 ? g : 0.f, a == j0 + 2 ? g : 0.f,
                                                        a == j0 + 3 ? g : 0.f);
    }
}

static int bn_slices_for(int b, int c, int l)
{
    long long rows = (long long)b * c;
    long long sl = (1024 + rows - 1) / rows;       // >= 1024 workgroups when the rows alone do not give them
    const long long maxs = l / 4096;
    if (sl > maxs) sl = maxs;
    if (sl < 1) sl = 1;
    if (sl > BN_MAX_SLICES) sl = BN_MAX_SLICES;
    return (int)sl;
}
static int fp_ch_for(int m)
{
    const int fit = FP_LDS_BYTES / ((int)sizeof(float) * m);
    return fit >= 8 ? 8 : (fit >= 4 ? 4 : (fit >= 2 ? 2 : (fit >= 1 ? 1 : 0)));
}
static int fp_slices_for(int b, int c, int ch, int n)
{
    const long long chunks = ((long long)c + ch - 1) / ch * b;
    long long sl = (512 + chunks - 1) / chunks;
    const long long maxs = n / 4096;
    if (sl > maxs) sl = maxs;
    if (sl < 1) sl = 1;
    if (sl > BN_MAX_SLICES) sl = BN_MAX_SLICES;
    return (int)sl;
}
static bool bn_dims_ok(int b, int c, int l) { return b >= 1 && c >= 1 && l >= 1 && b <= 65535 && c <= 65535; }
static int bn_gx(int l)
{
    int gx = (l / 4 + BN_THREADS * 4 - 1) / (BN_THREADS * 4);
    return gx < 1 ? 1 : (gx > 64 ? 64 : gx);
}

// ---- the O(c) arithmetic between the passes --------------------------------------------------------------------
// One wave per channel sums the (b x S) partial pairs in fp64, lanes striding over them, then a fixed butterfly:
// the same order on every run.
__global__ __launch_bounds__(64) void bn_sums_kernel(int b, int c, int s, const float *__restrict__ partial,
                                                     double *__restrict__ sums)
{
    const int ch = blockIdx.x, lane = threadIdx.x;
    double a0 = 0.0, a1 = 0.0;
    for (int t = lane; t < b * s; t += 64) {
        const int bi = t / s, sl = t - bi * s;
        const float2 v = reinterpret_cast<const float2 *>(partial)[((size_t)bi * c + ch) * s + sl];
        a0 += (double)v.x;
        a1 += (double)v.y;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        a0 += __shfl_xor(a0, o);
        a1 += __shfl_xor(a1, o);
    }
    if (lane == 0) {
        sums[2 * ch] = a0;
        sums[2 * ch + 1] = a1;
    }
}

// the same for the fp64 (b, c, S, 2) partials of bn_bwd_reduce_seg_kernel
__global__ __launch_bounds__(64) void bn_sums_f64_kernel(int b, int c, int s, const double *__restrict__ partial,
                                                         double *__restrict__ sums)
{
    const int ch = blockIdx.x, lane = threadIdx.x;
    double a0 = 0.0, a1 = 0.0;
    for (int t = lane; t < b * s; t += 64) {
        const int bi = t / s, sl = t - bi * s;
        const double2 v = reinterpret_cast<const double2 *>(partial)[((size_t)bi * c + ch) * s + sl];
        a0 += v.x;
        a1 += v.y;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        a0 += __shfl_xor(a0, o);
        a1 += __shfl_xor(a1, o);
    }
    if (lane == 0) {
        sums[2 * ch] = a0;
        sums[2 * ch + 1] = a1;
    }
}

// the same for the shifted statistics records (s1, s2, pivot, count) of bn_stats_kernel / fp_front_kernel: every record is
// turned back into (sum x, sum x^2) in fp64 before it is added
__global__ __launch_bounds__(64) void bn_sums_shifted_kernel(int b, int c, int s, const float *__restrict__ partial,
                                                             double *__restrict__ sums)
{
    const int ch = blockIdx.x, lane = threadIdx.x;
    double a0 = 0.0, a1 = 0.0;
    for (int t = lane; t < b * s; t += 64) {
        const int bi = t / s, sl = t - bi * s;
        const float4 v = reinterpret_cast<const float4 *>(partial)[((size_t)bi * c + ch) * s + sl];
        const double s1 = v.x, s2 = v.y, p = v.z, n = v.w;
        a0 += s1 + n * p;
        a1 += s2 + 2.0 * p * s1 + n * p * p;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        a0 += __shfl_xor(a0, o);
        a1 += __shfl_xor(a1, o);
    }
    if (lane == 0) {
        sums[2 * ch] = a0;
        sums[2 * ch + 1] = a1;
    }
}

// mean / biased variance from (sum x, sum x^2) and the element count, everything BatchNorm derives from them:
// rstd, the affine pair of the apply pass, the running statistics (unbiased variance, factor eaf).
__global__ __launch_bounds__(256) void bn_finalize_kernel(int c, const double *__restrict__ sums, double count,
                                                          const double *__restrict__ count_dev, double eps, double eaf,
                                                          const float *__restrict__ gamma, const float *__restrict__ beta,
                                                          const float *__restrict__ pre_bias,
                                                          float *__restrict__ running_mean, float *__restrict__ running_var,
                                                          float *__restrict__ mean, float *__restrict__ rstd,
                                                          float *__restrict__ scale, float *__restrict__ shift)
{
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= c) return;
    const double n = count_dev ? *count_dev : count;
    const double m64 = sums[2 * ch] / n;
    double v64 = sums[2 * ch + 1] / n - m64 * m64;
    v64 = v64 > 0.0 ? v64 : 0.0;
    const float m = (float)m64, r = (float)(1.0 / sqrt(v64 + eps));
    const float sc = (gamma ? gamma[ch] : 1.f) * r;
    mean[ch] = m;
    rstd[ch] = r;
    scale[ch] = sc;
    shift[ch] = (beta ? beta[ch] : 0.f) - m * sc;
    // pre_bias: the statistics are of y, the layer normalises y + pre_bias (same output; the running mean sees the bias)
    if (running_mean)
        running_mean[ch] = running_mean[ch] * (float)(1.0 - eaf) + (float)eaf * (pre_bias ? (float)(m64 + (double)pre_bias[ch]) : m);
    if (running_var) {
        const double unbiased = v64 * (n / (n - 1.0 > 1.0 ? n - 1.0 : 1.0));
        running_var[ch] = running_var[ch] * (float)(1.0 - eaf) + (float)eaf * (float)unbiased;
    }
}

// backward: the parameter gradients from this rank's sums, the two means of the input gradient from the (all-reduced)
// sums; count == 0 (running statistics were used: constants) gives c1 = c2 = 0
__global__ __launch_bounds__(256) void bn_bwd_coef_kernel(int c, const double *__restrict__ local, const double *__restrict__ sums,
                                                          double count, const double *__restrict__ count_dev,
                                                          float *__restrict__ g_gamma, float *__restrict__ g_beta,
                                                          float *__restrict__ c1, float *__restrict__ c2)
{
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= c) return;
    const double n = count_dev ? *count_dev : count;
    g_beta[ch] = (float)local[2 * ch];
    g_gamma[ch] = (float)local[2 * ch + 1];
    c1[ch] = n > 0.0 ? (float)(sums[2 * ch] / n) : 0.f;
    c2[ch] = n > 0.0 ? (float)(sums[2 * ch + 1] / n) : 0.f;
}

} // namespace geot

using namespace geot;

GEOT_EXPORT int geot_bn_slices(int b, int c, int l) { return bn_dims_ok(b, c, l) ? bn_slices_for(b, c, l) : -1; }

GEOT_EXPORT int geot_bn_stats(int b, int c, int l, const float *x, float *partial, void *stream)
{
    if (!bn_dims_ok(b, c, l)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bn_stats_kernel, dim3(bn_slices_for(b, c, l), c, b), dim3(BN_THREADS), 0, (hipStream_t)stream, c, l, x, partial);
    return hipGetLastError();
}

GEOT_EXPORT int geot_bn_apply(int b, int c, int l, int relu, const float *x, const float *scale, const float *shift,
                              float *out, void *stream)
{
    if (!bn_dims_ok(b, c, l)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bn_apply_kernel, dim3(bn_gx(l), c, b), dim3(BN_THREADS), 0, (hipStream_t)stream, c, l, relu, x, scale, shift, out);
    return hipGetLastError();
}

GEOT_EXPORT int geot_bn_bwd_reduce(int b, int c, int l, int relu, const float *x, const float *dz, const float *scale,
                                   const float *shift, const float *mean, const float *rstd, float *partial, void *stream)
{
    if (!bn_dims_ok(b, c, l)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(bn_slices_for(b, c, l), c, b), dim3(BN_THREADS), 0, (hipStream_t)stream, c, l,
                       relu, x, dz, scale, shift, mean, rstd, partial);
    return hipGetLastError();
}

GEOT_EXPORT int geot_bn_bwd_apply(int b, int c, int l, int relu, const float *x, const float *dz, const float *scale,
                                  const float *shift, const float *mean, const float *rstd, const float *k0,
                                  const float *c1, const float *c2, float *dx, void *stream)
{
    if (!bn_dims_ok(b, c, l)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(bn_gx(l), c, b), dim3(BN_THREADS), 0, (hipStream_t)stream, c, l, relu, x, dz,
                       scale, shift, mean, rstd, k0, c1, c2, dx);
    return hipGetLastError();
}

static bool bn_seg_ok(int b, int c, int l, int n)
{
    return bn_dims_ok(b, c, l) && n >= 4 && n <= 256 && (n & 3) == 0 && l % n == 0;
}
static bool aligned16(const void *a, const void *b = nullptr, const void *c = nullptr)
{
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 15) == 0;
}

GEOT_EXPORT int geot_bn_stats_seg(int b, int c, int l, int n, const float *x, const float *seg, float *partial, void *stream)
{
    if (!bn_seg_ok(b, c, l, n) || !x || !seg || !partial || !aligned16(x)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bn_stats_seg_kernel, dim3(bn_slices_for(b, c, l), c, b), dim3(BN_THREADS), 0, (hipStream_t)stream, c, l, n, x,
                       seg, partial);
    return hipGetLastError();
}

GEOT_EXPORT int geot_bn_apply_seg(int b, int c, int l, int n, int relu, const float *x, const float *seg, const float *scale,
                                  const float *shift, float *out, void *stream)
{
    if (!bn_seg_ok(b, c, l, n) || !x || !seg || !scale || !shift || !out || !aligned16(x, out)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bn_apply_seg_kernel, dim3(bn_gx(l), c, b), dim3(BN_THREADS), 0, (hipStream_t)stream, c, l, n, relu, x, seg,
                       scale, shift, out);
    return hipGetLastError();
}

GEOT_EXPORT int geot_bn_bwd_reduce_seg(int b, int c, int l, int n, int relu, const float *x, const float *seg, const float *dz,
                                       const float *scale, const float *shift, const float *mean, const float *rstd,
                                       double *partial, void *stream)
{
    if (!bn_seg_ok(b, c, l, n) || !x || !seg || !dz || !scale || !shift || !mean || !rstd || !partial ||
        !aligned16(x, dz, partial))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(bn_bwd_reduce_seg_kernel, dim3(bn_slices_for(b, c, l), c, b), dim3(BN_THREADS), 0, (hipStream_t)stream, c, l,
                       n, relu, x, seg, dz, scale, shift, mean, rstd, partial);
    return hipGetLastError();
}

GEOT_EXPORT int geot_bn_sums_f64(int b, int c, int s, const double *partial, double *sums, void *stream)
{
    if (b < 1 || c < 1 || s < 1 || !partial || !sums || !aligned16(partial)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bn_sums_f64_kernel, dim3(c), dim3(64), 0, (hipStream_t)stream, b, c, s, partial, sums);
    return hipGetLastError();
}

GEOT_EXPORT int geot_bn_bwd_apply_seg(int b, int c, int l, int n, int relu, const float *x, const float *seg, const float *dz,
                                      const float *scale, const float *shift, const float *mean, const float *rstd,
                                      const float *k0, const float *c1, const float *c2, float *dx, float *dseg, void *stream)
{
    if (!bn_seg_ok(b, c, l, n) || !x || !seg || !dz || !scale || !shift || !mean || !rstd || !k0 || !c1 || !c2 || !dx || !dseg ||
        !aligned16(x, dz, dx))
        return hipErrorInvalidValue;
    const int groups = l / n;
    const long long rows = (long long)b * c * groups;
    const int lpr = n >= 32 ? 8 : (n >= 16 ? 4 : (n >= 8 ? 2 : 1));
    const long long blocks = (rows * lpr + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
#define GEOT_BAS(L) hipLaunchKernelGGL(bn_bwd_apply_seg_kernel<L>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rows, n, \
                                       groups, c, relu, x, seg, dz, scale, shift, mean, rstd, k0, c1, c2, dx, dseg)
    if (lpr == 8) GEOT_BAS(8); else if (lpr == 4) GEOT_BAS(4); else if (lpr == 2) GEOT_BAS(2); else GEOT_BAS(1);
#undef GEOT_BAS
    return hipGetLastError();
}

#define GEOT_THIN_J(J, CALL)                                                                                      \
    switch (J) {                                                                                                  \
    case 1: CALL(1); break;                                                                                       \
    case 2: CALL(2); break;                                                                                       \
    case 3: CALL(3); break;                                                                                       \
    case 4: CALL(4); break;                                                                                       \
    case 5: CALL(5); break;                                                                                       \
    case 6: CALL(6); break;                                                                                       \
    case 7: CALL(7); break;                                                                                       \
    default: CALL(8); break;                                                                                      \
    }
static bool thin_ok(int c, int j, int l) { return c >= 1 && c <= 65535 * THIN_CH && j >= 1 && j <= 8 && l >= 1; }

GEOT_EXPORT int geot_thin_moments_slices(int l)
{
    if (l < 1) return -1;
    const int s = (l + 2047) / 2048;
    return s > 64 ? 64 : s;
}

GEOT_EXPORT int geot_thin_moments(int j, int l, const float *x, double *partial, void *stream)
{
    if (!thin_ok(1, j, l) || !x || !partial) return hipErrorInvalidValue;
    const dim3 grid(geot_thin_moments_slices(l));
#define GEOT_TM(JV) hipLaunchKernelGGL(thin_moments_kernel<JV>, grid, dim3(THIN_MOM_THREADS), 0, (hipStream_t)stream, l, x, partial)
    GEOT_THIN_J(j, GEOT_TM)
#undef GEOT_TM
    return hipGetLastError();
}

GEOT_EXPORT int geot_thin_bn_sums(int c, int j, int l, int s, const double *partial, const float *w, const float *x, double *mom,
                                  double *sums, void *stream)
{
    if (!thin_ok(c, j, l) || s < 1 || !partial || !w || !x || !mom || !sums) return hipErrorInvalidValue;
    hipLaunchKernelGGL(thin_bn_sums_kernel, dim3((c + 255) / 256), dim3(256), 0, (hipStream_t)stream, c, j, l, s, partial, w, x, mom,
                       sums);
    return hipGetLastError();
}

GEOT_EXPORT int geot_thin_bn_apply(int c, int j, int l, int relu, const float *w, const float *x, const float *mean,
                                   const float *scale, const float *beta, float *out, void *stream)
{
    if (!thin_ok(c, j, l) || !w || !x || !mean || !scale || !beta || !out) return hipErrorInvalidValue;
    const int vec4 = (l & 3) == 0 && aligned16(x, out);
    int gx = ((vec4 ? l >> 2 : l) + BN_THREADS - 1) / BN_THREADS;
    gx = gx > 256 ? 256 : gx;
    const dim3 grid(gx, (c + THIN_CH - 1) / THIN_CH);
#define GEOT_TA(JV) hipLaunchKernelGGL(thin_bn_apply_kernel<JV>, grid, dim3(BN_THREADS), 0, (hipStream_t)stream, c, l, relu, vec4, w, \
                                       x, mean, scale, beta, out)
    GEOT_THIN_J(j, GEOT_TA)
#undef GEOT_TA
    return hipGetLastError();
}

GEOT_EXPORT int geot_thin_bn_bwd_slices(int c, int l) { return (c >= 1 && c <= 65535 && l >= 1) ? bn_slices_for(1, c, l) : -1; }

GEOT_EXPORT int geot_thin_bn_bwd_reduce(int c, int j, int l, int relu, const double *mom, const float *w, const float *x, const float *dz,
                                        const float *scale, const float *beta, const float *mean, const float *rstd,
                                        double *partial, void *stream)
{
    if (!thin_ok(c, j, l) || c > 65535 || !w || !x || !dz || !scale || !beta || !mean || !rstd || !partial)
        return hipErrorInvalidValue;
    const int vec4 = (l & 3) == 0 && aligned16(x, dz);
    const dim3 grid(bn_slices_for(1, c, l), c);
#define GEOT_TR(JV) hipLaunchKernelGGL(thin_bn_bwd_reduce_kernel<JV>, grid, dim3(BN_THREADS), 0, (hipStream_t)stream, l, relu, vec4, mom, w, \
                                       x, dz, scale, beta, mean, rstd, partial)
    GEOT_THIN_J(j, GEOT_TR)
#undef GEOT_TR
    return hipGetLastError();
}

GEOT_EXPORT int geot_thin_bn_bwd_sums(int c, int j, int s, const double *partial, double *local, double *gx, void *stream)
{
    if (!thin_ok(c, j, 1) || s < 1 || !partial || !local || !gx) return hipErrorInvalidValue;
    hipLaunchKernelGGL(thin_bn_bwd_sums_kernel, dim3((c * (2 + j) + 255) / 256), dim3(256), 0, (hipStream_t)stream, c, j, s, partial,
                       local, gx);
    return hipGetLastError();
}

GEOT_EXPORT int geot_thin_bn_wgrad(int c, int j, int l, int local_mean, const float *w, const double *mom, const double *gx,
                                   const double *sums, double count, const double *count_dev, const float *scale,
                                   const float *mean, const float *rstd, float *dw, void *stream)
{
    if (!thin_ok(c, j, l) || !w || !gx || !scale || !dw || (mom && (!sums || !mean || !rstd))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(thin_bn_wgrad_kernel, dim3((c * j + 255) / 256), dim3(256), 0, (hipStream_t)stream, c, j, l, local_mean, w,
                       mom, gx, sums, count, count_dev, scale, mean, rstd, dw);
    return hipGetLastError();
}
#undef GEOT_THIN_J

GEOT_EXPORT int geot_bn_sums_shifted(int b, int c, int s, const float *partial, double *sums, void *stream)
{
    if (b < 0 || c < 0 || s < 0) return hipErrorInvalidValue;
    if (c == 0) return hipSuccess;
    hipLaunchKernelGGL(bn_sums_shifted_kernel, dim3(c), dim3(64), 0, (hipStream_t)stream, b, c, s, partial, sums);
    return hipGetLastError();
}

GEOT_EXPORT int geot_bn_sums(int b, int c, int s, const float *partial, double *sums, void *stream)
{
    if (b < 1 || c < 1 || s < 1 || !partial || !sums) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bn_sums_kernel, dim3(c), dim3(64), 0, (hipStream_t)stream, b, c, s, partial, sums);
    return hipGetLastError();
}

GEOT_EXPORT int geot_bn_finalize(int c, const double *sums, double count, const double *count_dev, double eps, double eaf,
                                 const float *gamma, const float *beta, const float *pre_bias, float *running_mean,
                                 float *running_var, float *mean, float *rstd, float *scale, float *shift, void *stream)
{
    if (c < 1 || !sums || !mean || !rstd || !scale || !shift || (!count_dev && !(count > 0.0))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((c + 255) / 256), dim3(256), 0, (hipStream_t)stream, c, sums, count, count_dev,
                       eps, eaf, gamma, beta, pre_bias, running_mean, running_var, mean, rstd, scale, shift);
    return hipGetLastError();
}

GEOT_EXPORT int geot_bn_bwd_coef(int c, const double *local_sums, const double *sums, double count, const double *count_dev,
                                 float *g_gamma, float *g_beta, float *c1, float *c2, void *stream)
{
    if (c < 1 || !local_sums || !sums || !g_gamma || !g_beta || !c1 || !c2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bn_bwd_coef_kernel, dim3((c + 255) / 256), dim3(256), 0, (hipStream_t)stream, c, local_sums, sums, count,
                       count_dev, g_gamma, g_beta, c1, c2);
    return hipGetLastError();
}

GEOT_EXPORT int geot_fp_front_slices(int b, int c, int m, int n)
{
    const int ch = fp_ch_for(m);
    return (bn_dims_ok(b, c, n) && m >= 1 && ch >= 1) ? fp_slices_for(b, c, ch, n) : -1;
}

GEOT_EXPORT int geot_fp_front(int b, int c, int m, int n, int cs, const float *A, const int *idx, const float *weight,
                              const float *skip, const float *Wb, float *y, float *partial, void *stream)
{
    const int ch = fp_ch_for(m);
    if (!bn_dims_ok(b, c, n) || m < 1 || ch < 1 || cs < 0 || cs > FP_MAX_SKIP || (cs > 0 && (!skip || !Wb)))
        return hipErrorInvalidValue;
    const int slices = fp_slices_for(b, c, ch, n);
    const size_t lds = (size_t)ch * m * sizeof(float);
    const dim3 grid(slices, (c + ch - 1) / ch, b);
    hipError_t e = hipSuccess;
#define GEOT_FP_LAUNCH(CHV)                                                                                       \
    {                                                                                                             \
        e = allow_big_lds((const void *)fp_front_kernel<CHV>, lds);                                               \
        if (e != hipSuccess) return e;                                                                            \
        hipLaunchKernelGGL((fp_front_kernel<CHV>), grid, dim3(FP_THREADS), lds, (hipStream_t)stream, c, m, n, cs, A, \
                           idx, weight, skip, Wb, y, partial);                                                    \
    }
    if (ch == 8) GEOT_FP_LAUNCH(8) else if (ch == 4) GEOT_FP_LAUNCH(4) else if (ch == 2) GEOT_FP_LAUNCH(2) else GEOT_FP_LAUNCH(1)
#undef GEOT_FP_LAUNCH
    return hipGetLastError();
}

GEOT_EXPORT int geot_segment_max(long long rows, int n, const float *x, float *out, unsigned char *arg, void *stream)
{
    if (rows < 0 || n < 4 || n > 256 || (n & 3) || (((uintptr_t)x) & 15)) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    const int lpr = n >= 32 ? 8 : (n >= 16 ? 4 : (n >= 8 ? 2 : 1));
    const long long blocks = (rows * lpr + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (lpr == 8) hipLaunchKernelGGL(segment_max_kernel<8>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rows, n, x, out, arg);
    else if (lpr == 4) hipLaunchKernelGGL(segment_max_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rows, n, x, out, arg);
    else if (lpr == 2) hipLaunchKernelGGL(segment_max_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rows, n, x, out, arg);
    else hipLaunchKernelGGL(segment_max_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rows, n, x, out, arg);
    return hipGetLastError();
}

GEOT_EXPORT int geot_rowdot_small_slices(int rows, int l)
{
    if (rows < 1 || l < 1) return -1;
    long long s = (1024 + rows - 1) / rows;                  // >= 1024 workgroups, slices of >= 2048 elements
    const long long most = (l + 2047) / 2048;
    s = s > most ? most : s;
    return (int)(s < 1 ? 1 : (s > 64 ? 64 : s));
}

GEOT_EXPORT int geot_rowdot_small(int rows, int l, int j, const float *a, const float *b, float *partial, void *stream)
{
    if (rows < 1 || rows > 65535 || l < 1 || j < 1 || j > 8 || !a || !b || !partial) return hipErrorInvalidValue;
    const dim3 grid(geot_rowdot_small_slices(rows, l), rows);
#define GEOT_RD(JV) hipLaunchKernelGGL(rowdot_small_kernel<JV>, grid, dim3(256), 0, (hipStream_t)stream, l, a, b, partial)
    switch (j) {
    case 1: GEOT_RD(1); break;
    case 2: GEOT_RD(2); break;
    case 3: GEOT_RD(3); break;
    case 4: GEOT_RD(4); break;
    case 5: GEOT_RD(5); break;
    case 6: GEOT_RD(6); break;
    case 7: GEOT_RD(7); break;
    default: GEOT_RD(8); break;
    }
#undef GEOT_RD
    return hipGetLastError();
}

static int colsum_slices(int rows, int cols)
{
    const int cb = (cols + 63) / 64;
    long long s = (256 + cb - 1) / cb;                     // ~256 workgroups, slices of >= 32 rows, at most 16 slices: the
    const long long most = (rows + 31) / 32;               // finish pass reads them one after the other
    s = s > most ? most : s;
    return (int)(s < 1 ? 1 : (s > 16 ? 16 : s));
}
GEOT_EXPORT long long geot_colsum_ws_floats(int rows, int cols)
{
    if (rows < 1 || cols < 1) return -1;
    return (long long)colsum_slices(rows, cols) * cols;
}
GEOT_EXPORT int geot_colsum(int rows, int cols, const float *x, float *out, float *workspace, void *stream)
{
    if (rows < 1 || cols < 1 || !x || !out || !workspace) return hipErrorInvalidValue;
    const int s = colsum_slices(rows, cols);
    hipLaunchKernelGGL(colsum_kernel, dim3((cols + 63) / 64, s), dim3(256), 0, (hipStream_t)stream, rows, cols, x, workspace);
    hipLaunchKernelGGL(colsum_finish_kernel, dim3((cols + 255) / 256), dim3(256), 0, (hipStream_t)stream, s, cols, workspace, out);
    return hipGetLastError();
}

namespace geot {
// out[r] = sum of the n floats of row r, accumulated in fp64 in a fixed order (a lane's strided share ascending, then a
// fixed tree): one workgroup per row.  For the long, few-row sums whose torch form (aten::sum over 10^5 elements into a
// handful of outputs) zeroes a semaphore buffer with hipMemsetAsync -- a memset NODE once captured, which ROCm 7.0's graph
// packet capture does not keep ordered (geot_amd/graph_step.py): bias gradients of 1x1 convolutions over (B, C, N), the
// per-channel sums of the FP stage's skip input.
__global__ __launch_bounds__(256) void rowsum_f64_kernel(int n, const float *__restrict__ x, double *__restrict__ out)
{
    const float *row = x + (size_t)blockIdx.x * n;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += (double)row[i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    __shared__ double part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}
} // namespace geot

GEOT_EXPORT int geot_rowsum_f64(long long rows, int n, const float *x, double *out, void *stream)
{
    if (rows < 0 || n < 0 || rows > 0x7fffffffLL) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    hipLaunchKernelGGL(geot::rowsum_f64_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, n, x, out);
    return hipGetLastError();
}

GEOT_EXPORT int geot_segment_sum(long long rows, int n, const float *x, float *out, void *stream)
{
    if (rows < 0 || n < 4 || n > 256 || (n & 3) || (((uintptr_t)x) & 15)) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    const int lpr = n >= 32 ? 8 : (n >= 16 ? 4 : (n >= 8 ? 2 : 1));
    const long long blocks = (rows * lpr + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (lpr == 8) hipLaunchKernelGGL(segment_sum_kernel<8>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rows, n, x, out);
    else if (lpr == 4) hipLaunchKernelGGL(segment_sum_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rows, n, x, out);
    else if (lpr == 2) hipLaunchKernelGGL(segment_sum_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rows, n, x, out);
    else hipLaunchKernelGGL(segment_sum_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rows, n, x, out);
    return hipGetLastError();
}

GEOT_EXPORT int geot_bn_pool(int b, int c, int groups, int n, int relu, const float *y, const float *scale, const float *shift,
                             float *out, float *sel, unsigned char *arg, void *stream)
{
    if (b < 1 || c < 1 || groups < 1 || n < 4 || n > 256 || (n & 3) || !y || !scale || !shift || !out || !sel || !arg ||
        (((uintptr_t)y) & 15))
        return hipErrorInvalidValue;
    const long long rows = (long long)b * c * groups;
    const int lpr = n >= 32 ? 8 : (n >= 16 ? 4 : (n >= 8 ? 2 : 1));
    const long long blocks = (rows * lpr + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
#define GEOT_BP(L) hipLaunchKernelGGL(bn_pool_kernel<L>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rows, n, groups, c, \
                                      relu, y, scale, shift, out, sel, arg)
    if (lpr == 8) GEOT_BP(8); else if (lpr == 4) GEOT_BP(4); else if (lpr == 2) GEOT_BP(2); else GEOT_BP(1);
#undef GEOT_BP
    return hipGetLastError();
}

GEOT_EXPORT int geot_bn_pool_grad(int b, int c, int groups, int n, const float *y, const float *gm, const unsigned char *arg,
                                  const float *mean, const float *rstd, const float *k0, const float *c1, const float *c2,
                                  float *dx, void *stream)
{
    if (b < 1 || c < 1 || groups < 1 || n < 4 || n > 256 || (n & 3) || !y || !gm || !arg || !mean || !rstd || !k0 || !c1 || !c2 ||
        !dx || ((((uintptr_t)y) | ((uintptr_t)dx)) & 15))
        return hipErrorInvalidValue;
    const long long total4 = (long long)b * c * groups * (n >> 2);
    long long blocks = (total4 + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(bn_pool_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, total4, n >> 2, groups, c, y, gm,
                       arg, mean, rstd, k0, c1, c2, dx);
    return hipGetLastError();
}

GEOT_EXPORT int geot_segment_max_grad(long long rows, int n, const float *dy, const unsigned char *arg, float *dx, void *stream)
{
    if (rows < 0 || n < 4 || n > 256 || (n & 3) || (((uintptr_t)dx) & 15)) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    const long long total4 = rows * (n >> 2);
    long long blocks = (total4 + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(segment_max_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, total4, n >> 2, dy, arg, dx);
    return hipGetLastError();
}
