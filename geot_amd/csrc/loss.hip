// Poly-1 focal loss on channels-first logits (B, C, N) with integer labels (B, N), forward + backward as streaming
// kernels (the reference composes ~15 element-wise torch ops each way on one-hot tensors:
// openpoints/loss/build.py:183-258 Poly1FocalLoss, :799-892 Poly1FocalLoss_U_corr).
//   y = [label == c],  p = sigmoid(x),  ce = BCE-with-logits(x, y),  pt = y p + (1 - y)(1 - p),  q = 1 - pt
//   l = at * ce * q^gamma + eps * q^(gamma + 1),   at = alpha y + (1 - alpha)(1 - y) if alpha >= 0 else 1
// mean form:   loss = sum l / (B C N);   masked form:  loss = sum l * keep[b, n] / (C * sum keep + 0.001).
#include "geot_common.h"
#include "geot_hip.h"

namespace geot {

constexpr int PL_THREADS = 256;

struct Poly1 {
    float alpha, gamma, eps;
    __device__ __forceinline__ float powg(float q, float g) const { return g == 2.f ? q * q : (g == 1.f ? q : powf(q, g)); }
    // value and d/dx for one logit
    __device__ __forceinline__ void eval(float x, bool pos, float &l, float &dl) const
    {
        const float p = 1.f / (1.f + expf(-x));
        const float ce = fmaxf(x, 0.f) - (pos ? x : 0.f) + log1pf(expf(-fabsf(x)));   // torch's stable form
        const float q = pos ? 1.f - p : p;                                               // 1 - pt
        const float at = alpha >= 0.f ? (pos ? alpha : 1.f - alpha) : 1.f;
        const float qg = powg(q, gamma);
        l = at * ce * qg + eps * qg * q;
        const float dq = (pos ? -1.f : 1.f) * p * (1.f - p);                             // d q / d x
        const float qg1 = gamma == 2.f ? q : (q > 0.f ? qg / q : 0.f);                   // q^(gamma - 1)
        dl = at * ((p - (pos ? 1.f : 0.f)) * qg + ce * gamma * qg1 * dq) + eps * (gamma + 1.f) * qg * dq;
    }
};

// grid (blocks over n, C, B): partial[block] = (sum l * keep, sum keep) in fp64 (keep counted once per point: c == 0)
__global__ __launch_bounds__(PL_THREADS) void poly1_fwd_kernel(int c, int n, Poly1 P, const float *__restrict__ logits,
                                                               const long long *__restrict__ labels,
                                                               const unsigned char *__restrict__ keep, double *__restrict__ partial)
{
    const int bi = blockIdx.z, cc = blockIdx.y;
    const float *row = logits + ((size_t)bi * c + cc) * n;
    const long long *lab = labels + (size_t)bi * n;
    const unsigned char *kp = keep ? keep + (size_t)bi * n : nullptr;
    double s = 0.0, k = 0.0;
    for (int i = blockIdx.x * PL_THREADS + threadIdx.x; i < n; i += gridDim.x * PL_THREADS) {
        float l, dl;
        P.eval(row[i], lab[i] == cc, l, dl);
        const float w = kp ? (kp[i] ? 1.f : 0.f) : 1.f;
        s += (double)(l * w);
        if (cc == 0) {
            k += (double)w;
            // the reference's F.one_hot raises on a label outside [0, C) (an ignore index of -1 / 255, say); a kernel
            // cannot raise, and treating the point as all-negative would be a silently different loss: poison it
            if (lab[i] < 0 || lab[i] >= c) s += (double)__int_as_float(0x7fc00000);
        }
    }
    __shared__ double sh[2][PL_THREADS / 64];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { s += __shfl_xor(s, o); k += __shfl_xor(k, o); }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = s; sh[1][threadIdx.x >> 6] = k; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int w = 0; w < PL_THREADS / 64; ++w) { a += sh[0][w]; b += sh[1][w]; }
        double *dst = partial + 2 * (((size_t)bi * c + cc) * gridDim.x + blockIdx.x);
        dst[0] = a;
        dst[1] = b;
    }
}

// one block: out[0] = loss, out[1] = 1 / denominator (kept for the backward)
__global__ __launch_bounds__(PL_THREADS) void poly1_finish_kernel(int nparts, int c, int masked, double count,
                                                                  const double *__restrict__ partial, float *__restrict__ out)
{
    double s = 0.0, k = 0.0;
    for (int i = threadIdx.x; i < nparts; i += PL_THREADS) { s += partial[2 * i]; k += partial[2 * i + 1]; }
    __shared__ double sh[2][PL_THREADS / 64];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { s += __shfl_xor(s, o); k += __shfl_xor(k, o); }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = s; sh[1][threadIdx.x >> 6] = k; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int w = 0; w < PL_THREADS / 64; ++w) { a += sh[0][w]; b += sh[1][w]; }
        const double den = masked ? b * c + 0.001 : count;
        out[0] = (float)(a / den);
        out[1] = (float)(1.0 / den);
    }
}

// grad_logits = upstream * inv_den * keep * dl/dx
__global__ __launch_bounds__(PL_THREADS) void poly1_bwd_kernel(int c, int n, Poly1 P, const float *__restrict__ logits,
                                                               const long long *__restrict__ labels,
                                                               const unsigned char *__restrict__ keep,
                                                               const float *__restrict__ fin, const float *__restrict__ upstream,
                                                               float *__restrict__ grad)
{
    const int bi = blockIdx.z, cc = blockIdx.y;
    const size_t base = ((size_t)bi * c + cc) * n;
    const long long *lab = labels + (size_t)bi * n;
    const unsigned char *kp = keep ? keep + (size_t)bi * n : nullptr;
    const float g = upstream[0] * fin[1];
    for (int i = blockIdx.x * PL_THREADS + threadIdx.x; i < n; i += gridDim.x * PL_THREADS) {
        float l, dl;
        P.eval(logits[base + i], lab[i] == cc, l, dl);
        grad[base + i] = (kp && !kp[i]) ? 0.f : g * dl;
    }
}

static int pl_gx(int n)
{
    int gx = (n + PL_THREADS * 4 - 1) / (PL_THREADS * 4);
    return gx < 1 ? 1 : (gx > 32 ? 32 : gx);
}


// ---- class-weighted soft-max cross-entropy (openpoints/loss/build.py:913-925 Weight_CELoss, :928-938 Weight_CELoss_U) ----
//   w = class_weights.mean(dim=0);  per point  -w[y] * log_softmax(x)[y];  loss = sum / (B N)  (the reference takes .mean()
//   of a reduction='none' tensor: ignored points count in the denominator).  _U form (conf given): a point is ignored when
//   !(conf >= thresh) (a NaN confidence ignores it), when y == 0 and when y == 255.
// One lane per point walking the C channels at stride N (coalesced across the wave), the column in registers (CMAX).
constexpr int WCE_THREADS = 256;

static int wce_gx(int n)
{
    const int gx = (n + WCE_THREADS - 1) / WCE_THREADS;
    return gx < 1 ? 1 : (gx > 64 ? 64 : gx);
}

// w[cls] into LDS: a sequential fp32 sum over the bw rows, then one division
__device__ __forceinline__ void wce_weights(int c, int bw, const float *__restrict__ cw, float *sh_w)
{
    if ((int)threadIdx.x < c) {
        float s = cw[threadIdx.x];
        for (int r = 1; r < bw; ++r) s += cw[(size_t)r * c + threadIdx.x];
        sh_w[threadIdx.x] = s / (float)bw;
    }
    __syncthreads();
}

__device__ __forceinline__ bool wce_ignored(long long y, const float *cf, int i, float thresh)
{
    return cf != nullptr && (!(cf[i] >= thresh) || y == 0 || y == 255);
}

template <int CMAX>
__global__ __launch_bounds__(WCE_THREADS) void wce_fwd_kernel(int c, int n, int bw, float thresh, const float *__restrict__ logits,
                                                              const long long *__restrict__ labels,
                                                              const float *__restrict__ cw, const float *__restrict__ conf,
                                                              double *__restrict__ partial)
{
    __shared__ float sh_w[GEOT_NTM_MAX_C];
    __shared__ double sh[WCE_THREADS / 64];
    wce_weights(c, bw, cw, sh_w);
    const int bi = blockIdx.y;
    const float *col0 = logits + (size_t)bi * c * n;
    const long long *lab = labels + (size_t)bi * n;
    const float *cf = conf ? conf + (size_t)bi * n : nullptr;
    double s = 0.0;
    for (int i = blockIdx.x * WCE_THREADS + threadIdx.x; i < n; i += gridDim.x * WCE_THREADS) {
        const long long y = lab[i];
        if (wce_ignored(y, cf, i, thresh)) continue;
        float x[CMAX];
#pragma unroll
        for (int cc = 0; cc < CMAX; ++cc) x[cc] = cc < c ? col0[(size_t)cc * n + i] : -INFINITY;
        float m = x[0], xy = 0.f;
#pragma unroll
        for (int cc = 1; cc < CMAX; ++cc) m = fmaxf(m, x[cc]);
        float e = 0.f;
#pragma unroll
        for (int cc = 0; cc < CMAX; ++cc) {
            if (cc < c) e += expf(x[cc] - m);
            xy = (long long)cc == y ? x[cc] : xy;
        }
        // a label outside [0, C) (other than the _U form's 255): the reference raises; a kernel cannot -- poison the loss
        const float wy = (y >= 0 && y < c) ? sh_w[y] : __int_as_float(0x7fc00000);
        s += (double)(-(wy * ((xy - m) - logf(e))));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0;
        for (int w = 0; w < WCE_THREADS / 64; ++w) a += sh[w];
        double *dst = partial + 2 * ((size_t)bi * gridDim.x + blockIdx.x);
        dst[0] = a;
        dst[1] = 0.0;
    }
}

// grad_logits = upstream * w[y] / (B N) * (softmax - onehot); exactly 0 for ignored points; every element written
template <int CMAX>
__global__ __launch_bounds__(WCE_THREADS) void wce_bwd_kernel(int c, int n, int bw, float thresh, const float *__restrict__ logits,
                                                              const long long *__restrict__ labels,
                                                              const float *__restrict__ cw, const float *__restrict__ conf,
                                                              const float *__restrict__ fin, const float *__restrict__ upstream,
                                                              float *__restrict__ grad)
{
    __shared__ float sh_w[GEOT_NTM_MAX_C];
    wce_weights(c, bw, cw, sh_w);
    const int bi = blockIdx.y;
    const size_t base = (size_t)bi * c * n;
    const long long *lab = labels + (size_t)bi * n;
    const float *cf = conf ? conf + (size_t)bi * n : nullptr;
    const float g = upstream[0] * fin[1];
    for (int i = blockIdx.x * WCE_THREADS + threadIdx.x; i < n; i += gridDim.x * WCE_THREADS) {
        const long long y = lab[i];
        if (wce_ignored(y, cf, i, thresh)) {
#pragma unroll
            for (int cc = 0; cc < CMAX; ++cc)
                if (cc < c) grad[base + (size_t)cc * n + i] = 0.f;
            continue;
        }
        float x[CMAX];
#pragma unroll
        for (int cc = 0; cc < CMAX; ++cc) x[cc] = cc < c ? logits[base + (size_t)cc * n + i] : -INFINITY;
        float m = x[0];
#pragma unroll
        for (int cc = 1; cc < CMAX; ++cc) m = fmaxf(m, x[cc]);
        float e = 0.f;
#pragma unroll
        for (int cc = 0; cc < CMAX; ++cc) {
            x[cc] = expf(x[cc] - m);
            if (cc < c) e += x[cc];
        }
        const float gw = g * ((y >= 0 && y < c) ? sh_w[y] : __int_as_float(0x7fc00000));
#pragma unroll
        for (int cc = 0; cc < CMAX; ++cc)
            if (cc < c) grad[base + (size_t)cc * n + i] = gw * (x[cc] / e - ((long long)cc == y ? 1.f : 0.f));
    }
}

// ---- Poly-1 focal with a per-point factor (openpoints/loss/build.py:564-688 Poly1FocalLoss_U_T) ----------------------------
//   loss = sum l(x[b,c,n]) * beta[b,n] * keep[b,n] / (C sum keep + 0.001),  beta = conf[b,n] / t[b, y[b,n], n]
// (the reference multiplies by the 0/1 mask: a NaN or infinite beta of a dropped point still reaches the sum).
__device__ __forceinline__ float pb_beta(int c, int n, const float *__restrict__ t_b, const float *__restrict__ cf, long long y, int i)
{
    // a label outside [0, C): the reference's F.one_hot raises; poison instead of reading outside t
    return (y >= 0 && y < c) ? cf[i] / t_b[(size_t)y * n + i] : __int_as_float(0x7fc00000);
}

__global__ __launch_bounds__(PL_THREADS) void poly1_beta_fwd_kernel(int c, int n, Poly1 P, const float *__restrict__ logits,
                                                                    const long long *__restrict__ labels,
                                                                    const unsigned char *__restrict__ keep,
                                                                    const float *__restrict__ conf, const float *__restrict__ t,
                                                                    double *__restrict__ partial)
{
    const int bi = blockIdx.z, cc = blockIdx.y;
    const float *row = logits + ((size_t)bi * c + cc) * n;
    const float *t_b = t + (size_t)bi * c * n;
    const long long *lab = labels + (size_t)bi * n;
    const unsigned char *kp = keep + (size_t)bi * n;
    const float *cf = conf + (size_t)bi * n;
    double s = 0.0, k = 0.0;
    for (int i = blockIdx.x * PL_THREADS + threadIdx.x; i < n; i += gridDim.x * PL_THREADS) {
        float l, dl;
        const long long y = lab[i];
        P.eval(row[i], y == cc, l, dl);
        const float w = kp[i] ? 1.f : 0.f;
        s += (double)((l * pb_beta(c, n, t_b, cf, y, i)) * w);
        if (cc == 0) k += (double)w;
    }
    __shared__ double sh[2][PL_THREADS / 64];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { s += __shfl_xor(s, o); k += __shfl_xor(k, o); }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = s; sh[1][threadIdx.x >> 6] = k; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int w = 0; w < PL_THREADS / 64; ++w) { a += sh[0][w]; b += sh[1][w]; }
        double *dst = partial + 2 * (((size_t)bi * c + cc) * gridDim.x + blockIdx.x);
        dst[0] = a;
        dst[1] = b;
    }
}

// grad_logits = up/den * keep * beta * dl/dx;   grad_t[b,c,n] = [c == y] * up/den * keep * (-conf / t^2) * sum_c' l(x[b,c',n])
__global__ __launch_bounds__(PL_THREADS) void poly1_beta_bwd_kernel(int c, int n, Poly1 P, const float *__restrict__ logits,
                                                                    const long long *__restrict__ labels,
                                                                    const unsigned char *__restrict__ keep,
                                                                    const float *__restrict__ conf, const float *__restrict__ t,
                                                                    const float *__restrict__ fin, const float *__restrict__ upstream,
                                                                    float *__restrict__ grad, float *__restrict__ grad_t)
{
    const int bi = blockIdx.z, cc = blockIdx.y;
    const size_t base = ((size_t)bi * c + cc) * n;
    const float *x_b = logits + (size_t)bi * c * n;
    const float *t_b = t + (size_t)bi * c * n;
    const long long *lab = labels + (size_t)bi * n;
    const unsigned char *kp = keep + (size_t)bi * n;
    const float *cf = conf + (size_t)bi * n;
    const float g = upstream[0] * fin[1];
    for (int i = blockIdx.x * PL_THREADS + threadIdx.x; i < n; i += gridDim.x * PL_THREADS) {
        const long long y = lab[i];
        float gx = 0.f, gt = 0.f;
        if (kp[i]) {
            float l, dl;
            P.eval(logits[base + i], y == cc, l, dl);
            gx = (g * pb_beta(c, n, t_b, cf, y, i)) * dl;
            if (y == cc) {
                float sum = 0.f;
                for (int k = 0; k < c; ++k) {
                    P.eval(x_b[(size_t)k * n + i], k == cc, l, dl);
                    sum += l;
                }
                const float tv = t_b[(size_t)cc * n + i];
                gt = (g * sum) * (-cf[i] / (tv * tv));
            }
        }
        grad[base + i] = gx;
        grad_t[base + i] = gt;
    }
}

} // namespace geot

using namespace geot;

GEOT_EXPORT long long geot_poly1_focal_ws_doubles(int b, int c, int n)
{
    if (b < 1 || c < 1 || n < 1) return -1;
    return 2LL * b * c * pl_gx(n);
}

GEOT_EXPORT int geot_poly1_focal(int b, int c, int n, float alpha, float gamma, float epsilon, const float *logits,
                                 const long long *labels, const unsigned char *keep, double *workspace, float *out2,
                                 void *stream)
{
    if (b < 1 || c < 1 || n < 1 || b > 65535 || c > 65535 || !logits || !labels || !workspace || !out2) return hipErrorInvalidValue;
    const int gx = pl_gx(n);
    const Poly1 P{alpha, gamma, epsilon};
    hipLaunchKernelGGL(poly1_fwd_kernel, dim3(gx, c, b), dim3(PL_THREADS), 0, (hipStream_t)stream, c, n, P, logits, labels, keep,
                       workspace);
    hipLaunchKernelGGL(poly1_finish_kernel, dim3(1), dim3(PL_THREADS), 0, (hipStream_t)stream, b * c * gx, c, keep ? 1 : 0,
                       (double)b * c * n, workspace, out2);
    return hipGetLastError();
}

GEOT_EXPORT int geot_poly1_focal_grad(int b, int c, int n, float alpha, float gamma, float epsilon, const float *logits,
                                      const long long *labels, const unsigned char *keep, const float *out2,
                                      const float *upstream, float *grad_logits, void *stream)
{
    if (b < 1 || c < 1 || n < 1 || b > 65535 || c > 65535 || !logits || !labels || !out2 || !upstream || !grad_logits)
        return hipErrorInvalidValue;
    const Poly1 P{alpha, gamma, epsilon};
    hipLaunchKernelGGL(poly1_bwd_kernel, dim3(pl_gx(n), c, b), dim3(PL_THREADS), 0, (hipStream_t)stream, c, n, P, logits, labels,
                       keep, out2, upstream, grad_logits);
    return hipGetLastError();
}

#define GEOT_WCE_CASE(KERNEL, ...)                                                                                      \
    do {                                                                                                                \
        if (c <= 8) hipLaunchKernelGGL(KERNEL<8>, grid, dim3(WCE_THREADS), 0, (hipStream_t)stream, __VA_ARGS__);        \
        else if (c <= 17) hipLaunchKernelGGL(KERNEL<17>, grid, dim3(WCE_THREADS), 0, (hipStream_t)stream, __VA_ARGS__); \
        else hipLaunchKernelGGL(KERNEL<32>, grid, dim3(WCE_THREADS), 0, (hipStream_t)stream, __VA_ARGS__);              \
    } while (0)

GEOT_EXPORT long long geot_weighted_ce_ws_doubles(int b, int c, int n)
{
    if (b < 1 || c < 1 || c > GEOT_NTM_MAX_C || n < 1) return -1;
    return 2LL * b * wce_gx(n);
}

GEOT_EXPORT int geot_weighted_ce(int b, int c, int n, int bw, float thresh, const float *logits, const long long *labels,
                                 const float *class_weights, const float *conf, double *workspace, float *out2, void *stream)
{
    if (b < 1 || c < 1 || n < 1 || bw < 1 || b > 65535 || c > GEOT_NTM_MAX_C || !logits || !labels || !class_weights ||
        !workspace || !out2)
        return hipErrorInvalidValue;
    const int gx = wce_gx(n);
    const dim3 grid(gx, b);
    GEOT_WCE_CASE(wce_fwd_kernel, c, n, bw, thresh, logits, labels, class_weights, conf, workspace);
    hipLaunchKernelGGL(poly1_finish_kernel, dim3(1), dim3(PL_THREADS), 0, (hipStream_t)stream, b * gx, c, 0, (double)b * n,
                       workspace, out2);
    return hipGetLastError();
}

GEOT_EXPORT int geot_weighted_ce_grad(int b, int c, int n, int bw, float thresh, const float *logits, const long long *labels,
                                      const float *class_weights, const float *conf, const float *out2, const float *upstream,
                                      float *grad_logits, void *stream)
{
    if (b < 1 || c < 1 || n < 1 || bw < 1 || b > 65535 || c > GEOT_NTM_MAX_C || !logits || !labels || !class_weights || !out2 ||
        !upstream || !grad_logits)
        return hipErrorInvalidValue;
    const dim3 grid(wce_gx(n), b);
    GEOT_WCE_CASE(wce_bwd_kernel, c, n, bw, thresh, logits, labels, class_weights, conf, out2, upstream, grad_logits);
    return hipGetLastError();
}

GEOT_EXPORT int geot_poly1_focal_beta(int b, int c, int n, float alpha, float gamma, float epsilon, const float *logits,
                                      const long long *labels, const unsigned char *keep, const float *conf, const float *t,
                                      double *workspace, float *out2, void *stream)
{
    if (b < 1 || c < 1 || n < 1 || b > 65535 || c > 65535 || !logits || !labels || !keep || !conf || !t || !workspace || !out2)
        return hipErrorInvalidValue;
    const int gx = pl_gx(n);
    const Poly1 P{alpha, gamma, epsilon};
    hipLaunchKernelGGL(poly1_beta_fwd_kernel, dim3(gx, c, b), dim3(PL_THREADS), 0, (hipStream_t)stream, c, n, P, logits, labels,
                       keep, conf, t, workspace);
    hipLaunchKernelGGL(poly1_finish_kernel, dim3(1), dim3(PL_THREADS), 0, (hipStream_t)stream, b * c * gx, c, 1,
                       (double)b * c * n, workspace, out2);
    return hipGetLastError();
}

GEOT_EXPORT int geot_poly1_focal_beta_grad(int b, int c, int n, float alpha, float gamma, float epsilon, const float *logits,
                                           const long long *labels, const unsigned char *keep, const float *conf,
                                           const float *t, const float *out2, const float *upstream, float *grad_logits,
                                           float *grad_t, void *stream)
{
    if (b < 1 || c < 1 || n < 1 || b > 65535 || c > 65535 || !logits || !labels || !keep || !conf || !t || !out2 || !upstream ||
        !grad_logits || !grad_t)
        return hipErrorInvalidValue;
    const Poly1 P{alpha, gamma, epsilon};
    hipLaunchKernelGGL(poly1_beta_bwd_kernel, dim3(pl_gx(n), c, b), dim3(PL_THREADS), 0, (hipStream_t)stream, c, n, P, logits,
                       labels, keep, conf, t, out2, upstream, grad_logits, grad_t);
    return hipGetLastError();
}
