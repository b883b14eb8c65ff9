// Per-tooth moments of whole-scan labels (geot_tooth_moments): what the 3DTeethSeg challenge's three scores are made of.
// TSA needs counts, TLA and TIR need geometry -- per scan and class the centroid of the predicted vertices, the centroid of
// the labelled vertices and the labelled tooth's extent -- which the confusion counts of seg_metrics.hip do not hold.  One
// pass over every vertex of every batch slot, read in place from the concatenated scan set through scan_predict.hip's work
// records, one workgroup each; one launch whatever the batch holds, no host synchronisation.
//
// Everything is an integer.  A position is quantised around the slot's centre, q = rint((p - center) * 65536), |q| < 2^30, so
// sums are 64-bit additions and extents 64-bit maxima: no result depends on the order of arrival, and numpy's np.add.at /
// np.maximum.at give the same bits.  The extents are stored as max(q + 2^30) and max(2^30 - q), both positive where a vertex
// was seen, so a zero-filled row is the empty state and the caller's memset is the only initialisation.
//
// Accumulation: one LDS table of 21 c + 2 64-bit words per workgroup, added into the slot's row once at the end, skipping
// the words that stayed zero (the classes the record never met).  The vertex order of a scan is spatially coherent and
// class 0 is about half of it, so most waves hold one class or two: 64 lanes sending ten atomics each at the same ten LDS
// words serialise.  The default form therefore combines inside the wave first, as sm_count and fo_count do for their
// histograms: the lanes that share the first pending lane's class are found by ballot, their ten entries reduced across the
// wave with DPP (a sum of 64 q is taken as two 32-bit sums of the 16-bit halves, exact), and one lane adds them; after
// TM_PEEL such rounds the lanes still pending add their own.  GEOT_TOOTH_MOMENTS_IMPL=basic: every lane adds its own from the
// start.  The same integers either way.
#include "geot_common.h"
#include "geot_hip.h"
#include <cstdlib>

namespace geot {

constexpr int TM_THREADS = 256;
constexpr int TM_ENTRIES = 21;                               // per class
constexpr int TM_MAX_WORDS = TM_ENTRIES * GEOT_NTM_MAX_C + 2;
constexpr int TM_PEEL = 2;                                   // classes per wave and step combined by ballot, per side
constexpr int TM_BIAS = 1 << 30;
constexpr float TM_LIMIT = 16384.0f;                         // |d| below this: |q| < 2^30
constexpr float TM_SCALE = 65536.0f;

typedef unsigned long long tm_word;

__device__ __forceinline__ int row16_add_i32(int v)
{
    v += (int)dpp_mov<DPP_QUAD_XOR1>((uint32_t)v);
    v += (int)dpp_mov<DPP_QUAD_XOR2>((uint32_t)v);
    v += (int)dpp_mov<DPP_ROW_HALF_MIRROR>((uint32_t)v);
    v += (int)dpp_mov<DPP_ROW_MIRROR>((uint32_t)v);
    return v;
}
// the sum of the wave's 64 values, wave-uniform; every lane takes part (the four steps pair disjoint groups of lanes)
__device__ __forceinline__ int wave_add_i32(int v)
{
    v = row16_add_i32(v);
    return (__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) +
           (__builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}

// one vertex into the ten entries of one side of its class
__device__ __forceinline__ void tm_add_own(tm_word *e, int qx, int qy, int qz)
{
    atomicAdd(&e[0], (tm_word)1);
    atomicAdd(&e[1], (tm_word)(long long)qx);
    atomicAdd(&e[2], (tm_word)(long long)qy);
    atomicAdd(&e[3], (tm_word)(long long)qz);
    atomicMax(&e[4], (tm_word)(qx + TM_BIAS));
    atomicMax(&e[5], (tm_word)(qy + TM_BIAS));
    atomicMax(&e[6], (tm_word)(qz + TM_BIAS));
    atomicMax(&e[7], (tm_word)(TM_BIAS - qx));
    atomicMax(&e[8], (tm_word)(TM_BIAS - qy));
    atomicMax(&e[9], (tm_word)(TM_BIAS - qz));
}

// The lanes of `same` (a ballot, not empty) into the ten entries at e, added by one lane: wave-uniform values throughout.
__device__ __forceinline__ void tm_add_group(tm_word *e, bool same, unsigned long long group, int lane, int leader, int qx, int qy,
                                             int qz)
{
    const int q[3] = {qx, qy, qz};
    long long sum[3];
    uint32_t hi[3], lo[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        // q = 65536 (q >> 16) + (q & 65535): 64 high halves of at most 2^14 and 64 low ones below 2^16 each fit 32 bits
        const int top = wave_add_i32(same ? q[a] >> 16 : 0), low = wave_add_i32(same ? q[a] & 0xffff : 0);
        sum[a] = (long long)top * 65536 + low;
        hi[a] = wave_max_u32(same ? (uint32_t)(q[a] + TM_BIAS) : 0u);
        lo[a] = wave_max_u32(same ? (uint32_t)(TM_BIAS - q[a]) : 0u);
    }
    if (lane == leader) {
        atomicAdd(&e[0], (tm_word)__popcll(group));
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            atomicAdd(&e[1 + a], (tm_word)sum[a]);
            atomicMax(&e[4 + a], (tm_word)hi[a]);
            atomicMax(&e[7 + a], (tm_word)lo[a]);
        }
    }
}

// One side (label: side = 0, prediction: side = 10) of a wave's 64 vertices: key in [0, c) or -1 for a lane that adds nothing.
// Called by every lane of the wave.
template <bool BASIC>
__device__ __forceinline__ void tm_side(tm_word *tab, int side, int key, int lane, int qx, int qy, int qz)
{
    bool pending = key >= 0;
    if constexpr (!BASIC) {
        for (int k = 0; k < TM_PEEL; ++k) {
            const unsigned long long left = __ballot(pending);
            if (left == 0) return;
            const int leader = __ffsll(left) - 1;
            const int lkey = __builtin_amdgcn_readlane(key, leader);
            const bool same = pending && key == lkey;
            tm_add_group(tab + lkey * TM_ENTRIES + side, same, __ballot(same), lane, leader, qx, qy, qz);
            pending = pending && !same;
        }
    }
    if (pending) tm_add_own(tab + key * TM_ENTRIES + side, qx, qy, qz);
}

// adds 1 to *word for every lane with `on`; called by every lane of the wave
template <bool BASIC>
__device__ __forceinline__ void tm_tally(tm_word *word, bool on, int lane)
{
    if constexpr (BASIC) {
        if (on) atomicAdd(word, (tm_word)1);
    } else {
        const unsigned long long m = __ballot(on);
        if (m && lane == __ffsll(m) - 1) atomicAdd(word, (tm_word)__popcll(m));
    }
}

template <bool BASIC>
__global__ __launch_bounds__(TM_THREADS) void tooth_moments_kernel(
    int b, int c, int n_scans, long long total, const float *__restrict__ points, const int *__restrict__ labels,
    const long long *__restrict__ offsets, const long long *__restrict__ scan_ids, const float *__restrict__ center,
    const int4 *__restrict__ work, const long long *__restrict__ out_offsets, const long long *__restrict__ pred,
    tm_word *__restrict__ moments)
{
    __shared__ tm_word tab[TM_MAX_WORDS];
    // everything up to the loop is uniform over the workgroup; a record or a slot that cannot be used is skipped whole
    // (scan_predict_kernel's rules)
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

    const int words = TM_ENTRIES * c + 2;
    for (int i = threadIdx.x; i < words; i += TM_THREADS) tab[i] = 0;
    __syncthreads();

    const int lane = lane_id();
    const float cx = center[(size_t)s * 3], cy = center[(size_t)s * 3 + 1], cz = center[(size_t)s * 3 + 2];
    const float *V = points + (size_t)lo * 3;
    const int *L = labels + lo;
    const long long *P = pred + out_offsets[s];
    // `base` is uniform over a wave: every lane reaches the ballots and the DPP reductions together
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (long long base = (long long)first + wave * 64; base < end; base += TM_THREADS) {     // 64-bit: end may be 2^31 - 1
        const long long v = base + lane;
        const bool active = v < end;
        bool usable = false;
        int qx = 0, qy = 0, qz = 0;
        long long lab = -1, prd = -1;
        if (active) {
            const float dx = V[(size_t)v * 3] - cx, dy = V[(size_t)v * 3 + 1] - cy, dz = V[(size_t)v * 3 + 2] - cz;
            usable = fabsf(dx) < TM_LIMIT && fabsf(dy) < TM_LIMIT && fabsf(dz) < TM_LIMIT;      // false for a NaN and for +-inf
            if (usable) {
                qx = (int)rintf(dx * TM_SCALE);
                qy = (int)rintf(dy * TM_SCALE);
                qz = (int)rintf(dz * TM_SCALE);
                lab = L[v];
                prd = P[v];
            }
        }
        const int kl = usable && lab >= 0 && lab < c ? (int)lab : -1;
        const int kp = usable && prd >= 0 && prd < c ? (int)prd : -1;
        tm_side<BASIC>(tab, 0, kl, lane, qx, qy, qz);
        tm_side<BASIC>(tab, 10, kp, lane, qx, qy, qz);
        // the overlap of class k: one word per class, its lanes counted by ballot like a side's
        {
            bool pending = kl >= 0 && kl == kp;
            if constexpr (!BASIC) {
                for (int k = 0; k < TM_PEEL; ++k) {
                    const unsigned long long left = __ballot(pending);
                    if (left == 0) break;
                    const int leader = __ffsll(left) - 1;
                    const int lkey = __builtin_amdgcn_readlane(kl, leader);
                    const bool same = pending && kl == lkey;
                    const unsigned long long group = __ballot(same);
                    if (lane == leader) atomicAdd(&tab[lkey * TM_ENTRIES + 20], (tm_word)__popcll(group));
                    pending = pending && !same;
                }
            }
            if (pending) atomicAdd(&tab[kl * TM_ENTRIES + 20], (tm_word)1);
        }
        tm_tally<BASIC>(&tab[TM_ENTRIES * c], kl >= 1 && kp >= 1, lane);
        tm_tally<BASIC>(&tab[TM_ENTRIES * c + 1], active && !usable, lane);
    }
    __syncthreads();
    tm_word *row = moments + (size_t)s * words;
    for (int i = threadIdx.x; i < words; i += TM_THREADS) {
        const tm_word t = tab[i];
        if (t == 0) continue;               // nothing met: adding 0 or max-combining 0 changes nothing
        const int e = i < TM_ENTRIES * c ? i % TM_ENTRIES : 0;
        const bool extent = (e >= 4 && e < 10) || (e >= 14 && e < 20);
        if (extent) atomicMax(&row[i], t); else atomicAdd(&row[i], t);
    }
}

} // namespace geot

using namespace geot;

GEOT_EXPORT int geot_tooth_moments(int b, int c, int n_scans, long long total, const float *points, const int *labels,
                                   const long long *offsets, const long long *scan_ids, const float *center, int n_work,
                                   const int *work, const long long *out_offsets, const long long *pred, long long *moments,
                                   void *stream)
{
    if (b < 0 || b > 65535 || c < 1 || c > GEOT_NTM_MAX_C || n_scans < 1 || total < 1 || n_work < 0) return hipErrorInvalidValue;
    if (!points || !labels || !offsets || !scan_ids || !center || !out_offsets || !pred || !moments) return hipErrorInvalidValue;
    if (b == 0 || n_work == 0) return hipSuccess;
    if (!work || ((uintptr_t)work & 15) != 0) return hipErrorInvalidValue;
    const char *e = getenv("GEOT_TOOTH_MOMENTS_IMPL");      // read at every call, like the other A/B switches
    const int4 *jobs = reinterpret_cast<const int4 *>(work);
    tm_word *out = reinterpret_cast<tm_word *>(moments);
    hipStream_t s = (hipStream_t)stream;
    if (e && e[0] == 'b')
        hipLaunchKernelGGL((tooth_moments_kernel<true>), dim3(n_work), dim3(TM_THREADS), 0, s, b, c, n_scans, total, points, labels,
                           offsets, scan_ids, center, jobs, out_offsets, pred, out);
    else
        hipLaunchKernelGGL((tooth_moments_kernel<false>), dim3(n_work), dim3(TM_THREADS), 0, s, b, c, n_scans, total, points, labels,
                           offsets, scan_ids, center, jobs, out_offsets, pred, out);
    return hipGetLastError();
}
