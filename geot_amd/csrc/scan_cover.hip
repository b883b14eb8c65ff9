// Whole-scan prediction by covering passes (geot_scan_cover): the samples of P = ceil(M / m) passes drawn with
// geot_sample_draw_cover partition a scan, so every vertex takes the class probabilities the model produced for that very
// vertex -- no neighbour search, no interpolation, no workspace.  Two launches:
//
//   scatter  grid (ceil(m / 256), b): sample j of slot s OWNS vertex sel[s][j] iff pass * m + j < n_s (a position past n_s is
//            wrap-around fill that repeats the start of the permutation) and 0 <= sel[s][j] < n_s.  An owner stores its c
//            probabilities into (GEOT_VOTE_SET), or adds them to, the vertex's row of the vertex-major accumulator of
//            geot_scan_vote.  Over the passes of one cover every row has exactly one writer: no atomics.
//   finish   (GEOT_VOTE_FINISH, and only for someone who reads it) over scan_predict.hip's work table: the arg-max of every
//            row of sums -> pred and / or the confusion counts, by geot_scan_vote's rule (scan_finish.h, seg_metrics.h).
//
// The scatter reads prob (b, c, m) along j and writes rows of c floats at scattered vertices.  Of the two forms
// scan_predict.hip has for its accumulator (GEOT_VOTE_IMPL=row|tile) only the LDS-transposed tile is kept here: with a lane
// per sample the reads coalesce (64 consecutive j of one class) but every store instruction touches 64 different rows, 4
// bytes each, c times over; with a lane per (sample, class) the stores of a row coalesce but the reads stride by m floats.
// Through a wave-private tile [64][c | 1] both sides are contiguous: 256-byte reads per class, then each row's 4 c bytes
// written by c consecutive lanes.  geot_scan_vote's row form is fast because its wave holds ONE vertex's values in lanes
// < c already; here a wave holds 64 samples, so that form would be the strided one.  The odd row stride keeps the 32 lanes
// of a half on 32 banks when they write their own rows.
#include "geot_common.h"
#include "geot_hip.h"
#include "scan_finish.h"
#include "seg_metrics.h"

namespace geot {

constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / GEOT_WAVE;

// grid (ceil(m / SC_THREADS), b): blockIdx.y = batch slot, one wave per 64 consecutive samples
__global__ __launch_bounds__(SC_THREADS) void scan_cover_scatter_kernel(
    int c, int m, long long total, const long long *__restrict__ offsets, int n_scans, const long long *__restrict__ scan_ids,
    const long long *__restrict__ sel, const float *__restrict__ prob, int pass, const long long *__restrict__ out_offsets,
    float *__restrict__ acc, int set)
{
    extern __shared__ float tiles[];             // SC_WAVES tiles of 64 rows of c | 1 floats
    const int s = blockIdx.y;
    const PnScan sc = pnb_scan(s, n_scans, total, offsets, scan_ids);
    if (!sc.n) return;                           // an unusable slot is skipped whole
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long base = (long long)blockIdx.x * SC_THREADS + wave * 64;
    if (base >= m) return;                       // (no workgroup barrier below: the waves are on their own)
    const int cnt = m - base < 64 ? (int)(m - base) : 64;
    const bool active = lane < cnt;
    const long long j = base + lane;
    int v = -1;                                  // the vertex this lane's sample owns
    if (active) {
        const long long q = (long long)pass * m + j, x = sel[(size_t)s * m + j];
        if (q < sc.n && x >= 0 && x < sc.n) v = (int)x;
    }
    if (!__ballot(v >= 0)) return;               // nothing but fill
    const int cs = c | 1;
    float *tile = tiles + wave * 64 * cs;
    const float *P = prob + (size_t)s * c * m + j;
    for (int k = 0; k < c; ++k) tile[lane * cs + k] = active ? P[(size_t)k * m] : 0.f;
    sp_wave_lds_sync();
    float *A = acc + (size_t)out_offsets[s] * c;
    const int elems = cnt * c;
    for (int i0 = 0; i0 < elems; i0 += 64) {     // uniform trip count: every lane takes part in the shuffle
        const int i = i0 + lane;
        const bool in = i < elems;
        const int r = in ? i / c : 0, k = i - r * c;
        const int vr = __shfl(v, r);
        if (in && vr >= 0) {
            float *a = A + (size_t)vr * c + k;
            const float x = tile[r * cs + k];
            *a = set ? x : *a + x;
        }
    }
}

// one workgroup per work-table entry, as scan_predict_kernel: each wave a contiguous quarter, 64 vertices at a time
__global__ __launch_bounds__(SC_THREADS) void scan_cover_finish_kernel(
    int b, int c, long long total, const int *__restrict__ labels, const long long *__restrict__ offsets, int n_scans,
    const long long *__restrict__ scan_ids, const int4 *__restrict__ work, const long long *__restrict__ out_offsets,
    const float *__restrict__ acc, long long *__restrict__ pred, unsigned long long *__restrict__ counts)
{
    __shared__ unsigned h[SC_WAVES * SM_MAX_SLOTS];
    extern __shared__ float tiles[];
    // everything up to the loop is uniform over the workgroup; an entry or a slot that cannot be used is skipped whole
    const int4 job = work[blockIdx.x];
    const int s = job.x;
    if (s < 0 || s >= b) return;
    const long long sid = scan_ids[s];
    if (sid < 0 || sid >= n_scans) return;
    const long long lo = offsets[sid], hi = offsets[sid + 1];
    if (lo < 0 || hi <= lo || hi > total || hi - lo > 0x7fffffffll) return;
    const int size = (int)(hi - lo);
    if (job.y < 0 || job.y >= size || job.z < 1) return;
    const int first = job.y;
    const int end = job.z < size - first ? first + job.z : size;

    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slots = c * (c + 1) + 1;
    unsigned *hw = h + wave * slots;
    if (counts) {
        for (int i = threadIdx.x; i < SC_WAVES * slots; i += SC_THREADS) h[i] = 0;
        __syncthreads();
    }
    const long long out0 = out_offsets[s];
    const int cs = c | 1;
    float *tile = tiles + wave * 64 * cs;
    const long long per = ((long long)(end - first) + SC_WAVES - 1) / SC_WAVES;
    const long long w0 = first + wave * per, w1 = w0 + per < end ? w0 + per : end;
    for (long long base = w0; base < w1; base += 64) {
        const int cnt = w1 - base < 64 ? (int)(w1 - base) : 64;
        const bool active = lane < cnt;
        const long long v = base + lane;
        const float *A = acc + (size_t)(out0 + base) * c;       // the wave's cnt rows are contiguous: one coalesced read
        for (int i = lane; i < cnt * c; i += 64) {
            const int r = i / c;
            tile[r * cs + (i - r * c)] = A[i];
        }
        sp_wave_lds_sync();
        const int cls = active ? sp_argmax_row(tile + lane * cs, c) : 0;
        sp_wave_lds_sync();
        if (pred && active) pred[out0 + v] = cls;
        if (counts) {
            const int key = active ? sm_slot(labels[lo + v], cls, c) : 0;
            sm_count(hw, key, active);
        }
    }
    if (counts) {
        __syncthreads();
        for (int i = threadIdx.x; i < slots; i += SC_THREADS) {
            unsigned t = 0;
#pragma unroll
            for (int w = 0; w < SC_WAVES; ++w) t += h[w * slots + i];
            if (t) atomicAdd(&counts[(size_t)s * slots + i], (unsigned long long)t);
        }
    }
}

} // namespace geot

using namespace geot;

GEOT_EXPORT int geot_scan_cover(int b, int c, int n, int n_scans, long long total, const int *labels, const long long *offsets,
                                const long long *scan_ids, const long long *sel, const float *prob, int pass, int n_work,
                                const int *work, const long long *out_offsets, float *acc, int mode, long long *pred,
                                long long *counts, void *stream)
{
    if (b < 0 || b > 65535 || c < 1 || c > GEOT_NTM_MAX_C || n < 1 || n_scans < 1 || total < 1 || n_work < 0 || pass < 0)
        return hipErrorInvalidValue;
    if (!offsets || !scan_ids || !sel || !prob || (counts && !labels)) return hipErrorInvalidValue;
    if (!acc || !out_offsets || (mode & ~(GEOT_VOTE_SET | GEOT_VOTE_FINISH)) != 0) return hipErrorInvalidValue;
    if ((pred || counts) && !(mode & GEOT_VOTE_FINISH)) return hipErrorInvalidValue;
    if (b == 0 || n_work == 0) return hipSuccess;
    if (!work || ((uintptr_t)work & 15) != 0) return hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)SC_WAVES * 64 * (c | 1) * sizeof(float);
    hipLaunchKernelGGL(scan_cover_scatter_kernel, dim3(((unsigned)n + SC_THREADS - 1) / SC_THREADS, (unsigned)b), dim3(SC_THREADS),
                       lds, s, c, n, total, offsets, n_scans, scan_ids, sel, prob, pass, out_offsets, acc,
                       (mode & GEOT_VOTE_SET) != 0);
    if ((mode & GEOT_VOTE_FINISH) && (pred || counts))
        hipLaunchKernelGGL(scan_cover_finish_kernel, dim3(n_work), dim3(SC_THREADS), lds, s, b, c, total, labels, offsets, n_scans,
                           scan_ids, reinterpret_cast<const int4 *>(work), out_offsets, acc, pred,
                           reinterpret_cast<unsigned long long *>(counts));
    return hipGetLastError();
}
