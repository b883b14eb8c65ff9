// Whole scans decoded at full resolution from ONE backbone pass (geot_scan_decode_front, geot_scan_decode_finish).
// PointTransformer_seg_T's last decoder stage -- propogation_0 and seg_head -- is a pure function of a query's position once
// the backbone has produced the features of its 8192 centres: three_nn against the centres, the inverse-distance
// interpolation, the skip channels [one_hot(cls), xyz], two 1x1 convolutions with BatchNorm, the head.  In eval mode nothing
// ties the query set to the sampled set, so every vertex of a scan can be a query: no further forward pass, no interpolation
// of class probabilities.  What the dense kernels (geot_three_nn, geot_fp_front_cl) do not cover is the ragged case: scans of
// different sizes concatenated with offsets, read in place, no BatchNorm batch sums.
//
//   front   one workgroup per work record (slot, first vertex, vertex count, first output row), as scan_predict.hip's table
//           with the fourth word in use.  256 vertices at a time, one lane per vertex: the vertex goes through the slot's two
//           normalisations (the batcher's single fp32 operations, so a sampled vertex gets the bits of its pos row), then
//           three_nn_kernel's search -- the slot's m centres streamed through an LDS tile, strict '<' in ascending index order,
//           hence the three smallest by (d2, index) -- and fp_weights_kernel's weights.  (q, idx, weight) of the 256 vertices
//           go through LDS; then the workgroup writes their rows: a lane keeps the folded BatchNorm, the xyz columns and the
//           slot's constant of ITS channels in registers and walks the wave's vertices, three gathered rows of a per vertex,
//           so a wave instruction stores 1 KB of one row (four channels per lane where c_out is a multiple of 4 and every
//           pointer is 16-byte aligned; one channel per lane otherwise).  One writer per element, no atomics.
//   finish  the head's logits of a chunk (c, rows) channel-first -> pred and / or the confusion counts, over the same work
//           records: a lane per vertex reads its column (coalesced across the wave), scan_finish.h's arg-max rule, the wave's
//           LDS histogram of seg_metrics.h.
//
// Brute force: at m = 8192 a scan of 1e5 vertices costs 8.2e8 distance evaluations.  Measured (profiles/scan_decode_timing.txt)
// the launch runs at 0.2 TB/s of the bytes its shapes require, far below the memory rate: the 1.2 GB of rows do not set its
// time, the search and the row gathers do (not yet separated).  A grid over the centres (scan_predict.hip's) is the open end.
#include "geot_common.h"
#include "geot_hip.h"
#include "scan_finish.h"
#include "seg_metrics.h"

namespace geot {

constexpr int SD_THREADS = 256;
constexpr int SD_WAVES = SD_THREADS / GEOT_WAVE;
constexpr int SD_TILE = 1024;           // centres per LDS tile (12 KB), as three_nn_kernel

struct SdJob {
    int s;                // batch slot; -1: the record (or its slot) is skipped
    long long lo;         // first vertex of the slot's scan in the concatenated arrays
    int first, cnt;       // the record's vertices [first, first + cnt) of that scan
    long long row0;       // its first output row
};

// scan_predict_kernel's skip rules, and the fourth word: the record's cnt rows must lie in [0, rows)
__device__ __forceinline__ SdJob sd_job(const int4 *__restrict__ work, int b, long long total, const long long *__restrict__ offsets,
                                        int n_scans, const long long *__restrict__ scan_ids, long long rows)
{
    SdJob j = {-1, 0, 0, 0, 0};
    const int4 job = work[blockIdx.x];
    if (job.x < 0 || job.x >= b) return j;
    const long long sid = scan_ids[job.x];
    if (sid < 0 || sid >= n_scans) return j;
    const long long lo = offsets[sid], hi = offsets[sid + 1];
    if (lo < 0 || hi <= lo || hi > total || hi - lo > 0x7fffffffll) return j;
    const int size = (int)(hi - lo);
    if (job.y < 0 || job.y >= size || job.z < 1) return j;
    const int cnt = job.z < size - job.y ? job.z : size - job.y;
    if (job.w < 0 || (long long)job.w + cnt > rows) return j;
    j.s = job.x; j.lo = lo; j.first = job.y; j.cnt = cnt; j.row0 = job.w;
    return j;
}

// one channel group (VEC: four channels) of one row: act(ch_scale (w0 a0 + w1 a1 + w2 a2 + skip + W_xyz q) + ch_shift), every
// statement one fp32 operation, left to right
__device__ __forceinline__ float sd_elem(float a0, float a1, float a2, float w0, float w1, float w2, float skip, float wx, float wy,
                                         float wz, float qx, float qy, float qz, float sc, float sh, bool relu)
{
    float t = w0 * a0;
    t = t + w1 * a1;
    t = t + w2 * a2;
    t = t + skip;
    float x = wx * qx;
    x = x + wy * qy;
    x = x + wz * qz;
    t = t + x;
    t = sc * t + sh;
    return relu ? max_nan(t, 0.f) : t;
}

template <bool VEC>
__global__ __launch_bounds__(SD_THREADS) void scan_decode_front_kernel(
    int b, int m, int c_out, int relu, long long total, const float *__restrict__ points, const long long *__restrict__ offsets,
    int n_scans, const long long *__restrict__ scan_ids, const float *__restrict__ center, const float *__restrict__ scale,
    const float *__restrict__ view_center, const float *__restrict__ view_scale, const float *__restrict__ known,
    const float *__restrict__ a, const float *__restrict__ skip_const, const float *__restrict__ w_xyz,
    const float *__restrict__ ch_scale, const float *__restrict__ ch_shift, const int4 *__restrict__ work, long long rows,
    float *__restrict__ z, float *__restrict__ q_out, int *__restrict__ idx_out, float *__restrict__ weight_out)
{
    __shared__ float tile[SD_TILE * 3];
    __shared__ float sq[SD_THREADS * 3], sw[SD_THREADS * 3];
    __shared__ int si[SD_THREADS * 3];
    // everything up to the loop is uniform over the workgroup; a record or a slot that cannot be used is skipped whole
    const SdJob job = sd_job(work, b, total, offsets, n_scans, scan_ids, rows);
    if (job.s < 0) return;
    const int s = job.s;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float *V = points + (size_t)(job.lo + job.first) * 3;
    const float *K = known + (size_t)s * m * 3;
    const float *A = a + (size_t)s * m * c_out;
    const float ox = center[s * 3], oy = center[s * 3 + 1], oz = center[s * 3 + 2], os = scale[s];
    const float vx = view_center[s * 3], vy = view_center[s * 3 + 1], vz = view_center[s * 3 + 2], vs = view_scale[s];

    for (int base = 0; base < job.cnt; base += SD_THREADS) {
        const int i = base + (int)threadIdx.x;
        const bool live = i < job.cnt;
        float qx = 0.f, qy = 0.f, qz = 0.f;
        if (live) {      // pc_norm, then the view's centre-and-normalise: geot_cloud_sample_batch's and the views' statements
            qx = ((V[(size_t)i * 3] - ox) / os - vx) / vs;
            qy = ((V[(size_t)i * 3 + 1] - oy) / os - vy) / vs;
            qz = ((V[(size_t)i * 3 + 2] - oz) / os - vz) / vs;
        }
        float b1 = INFINITY, b2 = INFINITY, b3 = INFINITY;
        int i1 = 0, i2 = 0, i3 = 0;
        for (int k0 = 0; k0 < m; k0 += SD_TILE) {
            const int cnt = min(SD_TILE, m - k0);
            __syncthreads();
            for (int t = threadIdx.x; t < cnt * 3; t += SD_THREADS) tile[t] = K[(size_t)k0 * 3 + t];
            __syncthreads();
            for (int t = 0; t < cnt; ++t) {
                const float d = sqdist3(qx, qy, qz, tile[t * 3], tile[t * 3 + 1], tile[t * 3 + 2]);
                if (d < b3) {
                    const int k = k0 + t;
                    if (d < b1) { b3 = b2; i3 = i2; b2 = b1; i2 = i1; b1 = d; i1 = k; }
                    else if (d < b2) { b3 = b2; i3 = i2; b2 = d; i2 = k; }
                    else { b3 = d; i3 = k; }
                }
            }
        }
        // fp_weights_kernel's statements
        const float r0 = 1.0f / (sqrtf(b1) + 1e-8f), r1 = 1.0f / (sqrtf(b2) + 1e-8f), r2 = 1.0f / (sqrtf(b3) + 1e-8f);
        const float norm = (r0 + r1) + r2;
        const float w0 = r0 / norm, w1 = r1 / norm, w2 = r2 / norm;
        const int t3 = threadIdx.x * 3;
        sq[t3] = qx; sq[t3 + 1] = qy; sq[t3 + 2] = qz;
        sw[t3] = w0; sw[t3 + 1] = w1; sw[t3 + 2] = w2;
        si[t3] = i1; si[t3 + 1] = i2; si[t3 + 2] = i3;
        if (live) {
            const size_t o = (size_t)(job.row0 + i) * 3;
            if (q_out) { q_out[o] = qx; q_out[o + 1] = qy; q_out[o + 2] = qz; }
            if (idx_out) { idx_out[o] = i1; idx_out[o + 1] = i2; idx_out[o + 2] = i3; }
            if (weight_out) { weight_out[o] = w0; weight_out[o + 1] = w1; weight_out[o + 2] = w2; }
        }
        __syncthreads();
        // the rows of these nb vertices: wave w takes vertices w, w + 4, ...; a lane keeps its channels' constants
        const int nb = job.cnt - base < SD_THREADS ? job.cnt - base : SD_THREADS;
        const size_t zrow = (size_t)(job.row0 + base);
        if constexpr (VEC) {
            const int c4 = c_out >> 2;
            const float4 *A4 = reinterpret_cast<const float4 *>(A);
            float4 *Z4 = reinterpret_cast<float4 *>(z);
            for (int k = lane; k < c4; k += 64) {
                const float4 sc = reinterpret_cast<const float4 *>(ch_scale)[k], sh = reinterpret_cast<const float4 *>(ch_shift)[k];
                const float4 sk = reinterpret_cast<const float4 *>(skip_const + (size_t)s * c_out)[k];
                const float4 x0 = reinterpret_cast<const float4 *>(w_xyz)[3 * k], x1 = reinterpret_cast<const float4 *>(w_xyz)[3 * k + 1],
                             x2 = reinterpret_cast<const float4 *>(w_xyz)[3 * k + 2];      // W_xyz rows 4 k .. 4 k + 3
#pragma unroll 4
                for (int j = wave; j < nb; j += SD_WAVES) {       // four vertices' gathers in flight
                    const float px = sq[j * 3], py = sq[j * 3 + 1], pz = sq[j * 3 + 2];
                    const float u0 = sw[j * 3], u1 = sw[j * 3 + 1], u2 = sw[j * 3 + 2];
                    const float4 a0 = A4[(size_t)si[j * 3] * c4 + k], a1 = A4[(size_t)si[j * 3 + 1] * c4 + k],
                                 a2 = A4[(size_t)si[j * 3 + 2] * c4 + k];
                    float4 o;
                    o.x = sd_elem(a0.x, a1.x, a2.x, u0, u1, u2, sk.x, x0.x, x0.y, x0.z, px, py, pz, sc.x, sh.x, relu);
                    o.y = sd_elem(a0.y, a1.y, a2.y, u0, u1, u2, sk.y, x0.w, x1.x, x1.y, px, py, pz, sc.y, sh.y, relu);
                    o.z = sd_elem(a0.z, a1.z, a2.z, u0, u1, u2, sk.z, x1.z, x1.w, x2.x, px, py, pz, sc.z, sh.z, relu);
                    o.w = sd_elem(a0.w, a1.w, a2.w, u0, u1, u2, sk.w, x2.y, x2.z, x2.w, px, py, pz, sc.w, sh.w, relu);
                    Z4[(zrow + j) * c4 + k] = o;
                }
            }
        } else {
            for (int k = lane; k < c_out; k += 64) {
                const float sc = ch_scale[k], sh = ch_shift[k], sk = skip_const[(size_t)s * c_out + k];
                const float wx = w_xyz[3 * k], wy = w_xyz[3 * k + 1], wz = w_xyz[3 * k + 2];
#pragma unroll 4
                for (int j = wave; j < nb; j += SD_WAVES) {
                    const float a0 = A[(size_t)si[j * 3] * c_out + k], a1 = A[(size_t)si[j * 3 + 1] * c_out + k],
                                a2 = A[(size_t)si[j * 3 + 2] * c_out + k];
                    z[(zrow + j) * c_out + k] = sd_elem(a0, a1, a2, sw[j * 3], sw[j * 3 + 1], sw[j * 3 + 2], sk, wx, wy, wz, sq[j * 3],
                                                        sq[j * 3 + 1], sq[j * 3 + 2], sc, sh, relu);
                }
            }
        }
        __syncthreads();       // the next round overwrites sq / sw / si
    }
}

// one workgroup per work record; a lane per vertex, 256 at a time
__global__ __launch_bounds__(SD_THREADS) void scan_decode_finish_kernel(
    int b, int c, long long total, const int *__restrict__ labels, const long long *__restrict__ offsets, int n_scans,
    const long long *__restrict__ scan_ids, const int4 *__restrict__ work, long long rows, const float *__restrict__ logits,
    const long long *__restrict__ out_offsets, long long *__restrict__ pred, unsigned long long *__restrict__ counts)
{
    __shared__ unsigned h[SD_WAVES * SM_MAX_SLOTS];
    const SdJob job = sd_job(work, b, total, offsets, n_scans, scan_ids, rows);
    if (job.s < 0) return;
    const int s = job.s;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slots = c * (c + 1) + 1;
    unsigned *hw = h + wave * slots;
    if (counts) {
        for (int i = threadIdx.x; i < SD_WAVES * slots; i += SD_THREADS) h[i] = 0;
        __syncthreads();
    }
    const long long out0 = pred ? out_offsets[s] : 0;
    for (int base = 0; base < job.cnt; base += SD_THREADS) {       // uniform trip count: sm_count needs every lane of a wave
        const int i = base + (int)threadIdx.x;
        const bool active = i < job.cnt;
        const int cls = active ? sp_argmax_strided(logits + (size_t)(job.row0 + i), (size_t)rows, c) : 0;
        if (pred && active) pred[out0 + job.first + i] = cls;
        if (counts) {
            const int key = active ? sm_slot(labels[job.lo + job.first + i], cls, c) : 0;
            sm_count(hw, key, active);
        }
    }
    if (counts) {
        __syncthreads();
        for (int i = threadIdx.x; i < slots; i += SD_THREADS) {
            unsigned t = 0;
#pragma unroll
            for (int w = 0; w < SD_WAVES; ++w) t += h[w * slots + i];
            if (t) atomicAdd(&counts[(size_t)s * slots + i], (unsigned long long)t);
        }
    }
}

static bool sd_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

} // namespace geot

using namespace geot;

GEOT_EXPORT int geot_scan_decode_front(int b, int m, int c_out, int relu, int n_scans, long long total, const float *points,
                                       const long long *offsets, const long long *scan_ids, const float *center,
                                       const float *scale, const float *view_center, const float *view_scale, const float *known,
                                       const float *a, const float *skip_const, const float *w_xyz, const float *ch_scale,
                                       const float *ch_shift, int n_work, const int *work, long long rows, float *z, float *q,
                                       int *idx, float *weight, void *stream)
{
    if (b < 0 || b > 65535 || m < 3 || c_out < 1 || n_scans < 1 || total < 1 || n_work < 0 || rows < 0 || (relu != 0 && relu != 1))
        return hipErrorInvalidValue;
    if (rows > 0x7fffffffll) return hipErrorInvalidValue;
    if (!points || !offsets || !scan_ids || !center || !scale || !view_center || !view_scale || !known || !a || !skip_const ||
        !w_xyz || !ch_scale || !ch_shift || !z)
        return hipErrorInvalidValue;
    if (b == 0 || n_work == 0 || rows == 0) return hipSuccess;
    if (!work || !sd_aligned16(work)) return hipErrorInvalidValue;
    const bool vec = (c_out & 3) == 0 && sd_aligned16(a) && sd_aligned16(z) && sd_aligned16(skip_const) && sd_aligned16(w_xyz) &&
                     sd_aligned16(ch_scale) && sd_aligned16(ch_shift);
#define SD_LAUNCH(VEC)                                                                                                         \
    hipLaunchKernelGGL((scan_decode_front_kernel<VEC>), dim3(n_work), dim3(SD_THREADS), 0, (hipStream_t)stream, b, m, c_out, relu, \
                       total, points, offsets, n_scans, scan_ids, center, scale, view_center, view_scale, known, a, skip_const,  \
                       w_xyz, ch_scale, ch_shift, reinterpret_cast<const int4 *>(work), rows, z, q, idx, weight)
    if (vec) SD_LAUNCH(true); else SD_LAUNCH(false);
#undef SD_LAUNCH
    return hipGetLastError();
}

GEOT_EXPORT int geot_scan_decode_finish(int b, int c, int n_scans, long long total, const int *labels, const long long *offsets,
                                        const long long *scan_ids, int n_work, const int *work, long long rows, const float *logits,
                                        const long long *out_offsets, long long *pred, long long *counts, void *stream)
{
    if (b < 0 || b > 65535 || c < 1 || c > GEOT_NTM_MAX_C || n_scans < 1 || total < 1 || n_work < 0 || rows < 0 ||
        rows > 0x7fffffffll)
        return hipErrorInvalidValue;
    if (!offsets || !scan_ids || !logits || (counts && !labels) || (!pred && !counts) || (pred && !out_offsets))
        return hipErrorInvalidValue;
    if (b == 0 || n_work == 0 || rows == 0) return hipSuccess;
    if (!work || !sd_aligned16(work)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scan_decode_finish_kernel, dim3(n_work), dim3(SD_THREADS), 0, (hipStream_t)stream, b, c, total, labels,
                       offsets, n_scans, scan_ids, reinterpret_cast<const int4 *>(work), rows, logits, out_offsets, pred,
                       reinterpret_cast<unsigned long long *>(counts));
    return hipGetLastError();
}
