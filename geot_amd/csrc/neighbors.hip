// neighbors.hip -- radius / nearest-neighbour searches for gfx950 (MI355X).
//
// Replaces (behaviour, not code):
//   ball query : pointnet2/_ext_src/src/ball_query_gpu.cu:12-57,
//                openpoints/cpp/pointnet2_batch/src/ball_query_gpu.cu:15-74,
//                openpoints/cpp/pointops/src/ballquery/ballquery_cuda_kernel.cu:13-88
//   three_nn   : pointnet2/_ext_src/src/interpolate_gpu.cu:12-71,
//                openpoints/cpp/pointnet2_batch/src/interpolate_gpu.cu:16-72
//   kNN (heap) : pointops/src/knnquery/knnquery_cuda_kernel.cu:21-116
//   kNN (sorted): contract of knn_cuda.KNN / knn_point
//
// All of these are O(queries x support) scans of fp32 coordinates that fit in
// L2; they are VALU-bound, not HBM-bound. Support points are staged through
// LDS in tiles so that every lane of a wave reads the same address
// (broadcast, conflict-free) while each lane owns one query.
#include "geot_common.h"
#include "geot_hip.h"
#include <cstdlib>

namespace geot {

// ---------------------------------------------------------------------------
// Ball query: one wave per query, the 64 lanes test 64 consecutive support
// points per step, so "the first nsample hits in ascending index order" falls
// out of a ballot + prefix popcount, and the wave stops as soon as nsample
// hits are found (same early exit as the reference's serial scan).
// ---------------------------------------------------------------------------
constexpr int BQ_WAVES = 4;

__device__ __forceinline__ void ball_query_one(const float *__restrict__ P, int n_pts, int idx_base,
                                               float qx, float qy, float qz, float r2, int nsample,
                                               int *__restrict__ hits, int *__restrict__ out)
{
    const int lane = lane_id();
    int cnt = 0;
    for (int k0 = 0; k0 < n_pts && cnt < nsample; k0 += 64) {
        int k = k0 + lane;
        bool hit = false;
        if (k < n_pts) {
            float d2 = sqdist3(qx, qy, qz, P[k * 3 + 0], P[k * 3 + 1], P[k * 3 + 2]);
            hit = d2 < r2;
        }
        unsigned long long mask = __ballot(hit);
        if (mask) {
            int rank = cnt + __popcll(mask & ((1ull << lane) - 1ull));
            if (hit && rank < nsample) hits[rank] = idx_base + k;
            cnt += __popcll(mask);
        }
    }
    if (cnt > nsample) cnt = nsample;
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    int first = cnt ? hits[0] : 0;
    for (int l = lane; l < nsample; l += 64) out[l] = l < cnt ? hits[l] : first;
}

__global__ __launch_bounds__(BQ_WAVES * 64) void ball_query_kernel(
    int b, int n, int m, float radius, int nsample, const float *__restrict__ new_xyz,
    const float *__restrict__ xyz, int *__restrict__ idx)
{
    extern __shared__ int bq_hits[];
    const int wave = threadIdx.x >> 6;
    int *hits = bq_hits + wave * nsample;
    const float r2 = radius * radius;
    const long long total = (long long)b * m;
    for (long long q = (long long)blockIdx.x * BQ_WAVES + wave; q < total;
         q += (long long)gridDim.x * BQ_WAVES) {
        int bi = (int)(q / m);
        const float *Q = new_xyz + q * 3;
        ball_query_one(xyz + (size_t)bi * n * 3, n, 0, Q[0], Q[1], Q[2], r2, nsample, hits,
                       idx + q * nsample);
        __builtin_amdgcn_wave_barrier();
    }
}

__device__ __forceinline__ int segment_of(int pt, const int *__restrict__ off, int b)
{
    int i = 0;
    while (i < b - 1 && !(pt < off[i])) ++i;
    return i;
}

__global__ __launch_bounds__(BQ_WAVES * 64) void ballquery_offset_kernel(
    int b, int m, float radius, int nsample, const float *__restrict__ xyz,
    const float *__restrict__ new_xyz, const int *__restrict__ offset,
    const int *__restrict__ new_offset, int *__restrict__ idx)
{
    extern __shared__ int bq_hits[];
    const int wave = threadIdx.x >> 6;
    int *hits = bq_hits + wave * nsample;
    const float r2 = radius * radius;
    for (int q = blockIdx.x * BQ_WAVES + wave; q < m; q += gridDim.x * BQ_WAVES) {
        int bt = segment_of(q, new_offset, b);
        int start = bt ? offset[bt - 1] : 0, end = offset[bt];
        const float *Q = new_xyz + (size_t)q * 3;
        ball_query_one(xyz + (size_t)start * 3, end - start, start, Q[0], Q[1], Q[2], r2, nsample,
                       hits, idx + (size_t)q * nsample);
        __builtin_amdgcn_wave_barrier();
    }
}

// ---------------------------------------------------------------------------
// three_nn: one lane per unknown point, known points streamed through LDS.
// Result = 3 smallest by (d2, index): strict '<' while scanning k ascending.
// The reference keeps the running bests as doubles initialised to 1e40; with
// fp32 candidates that is the same as fp32 bests initialised to +inf.
// ---------------------------------------------------------------------------
constexpr int NN_THREADS = 256;
constexpr int NN_TILE = 1024;

__global__ __launch_bounds__(NN_THREADS) void three_nn_kernel(
    int n, int m, const float *__restrict__ unknown, const float *__restrict__ known,
    float *__restrict__ dist2, int *__restrict__ idx)
{
    __shared__ float tile[NN_TILE * 3];
    const int bi = blockIdx.y;
    const float *U = unknown + (size_t)bi * n * 3;
    const float *K = known + (size_t)bi * m * 3;
    const int j = blockIdx.x * NN_THREADS + threadIdx.x;
    const bool live = j < n;
    float ux = 0, uy = 0, uz = 0;
    if (live) { ux = U[j * 3]; uy = U[j * 3 + 1]; uz = U[j * 3 + 2]; }
    float b1 = INFINITY, b2 = INFINITY, b3 = INFINITY;
    int i1 = 0, i2 = 0, i3 = 0;
    for (int k0 = 0; k0 < m; k0 += NN_TILE) {
        int cnt = min(NN_TILE, m - k0);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt * 3; t += NN_THREADS) tile[t] = K[(size_t)k0 * 3 + t];
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            float d = sqdist3(ux, uy, uz, tile[t * 3], tile[t * 3 + 1], tile[t * 3 + 2]);
            if (d < b3) {
                int k = k0 + t;
                if (d < b1) { b3 = b2; i3 = i2; b2 = b1; i2 = i1; b1 = d; i1 = k; }
                else if (d < b2) { b3 = b2; i3 = i2; b2 = d; i2 = k; }
                else { b3 = d; i3 = k; }
            }
        }
    }
    if (live) {
        size_t o = ((size_t)bi * n + j) * 3;
        dist2[o] = b1; dist2[o + 1] = b2; dist2[o + 2] = b3;
        idx[o] = i1; idx[o + 1] = i2; idx[o + 2] = i3;
    }
}

// ---------------------------------------------------------------------------
// kNN, both flavours: one lane per query, its candidate list in LDS laid out
// [slot][lane] (bank = lane, so the common "all lanes touch slot s" access is
// conflict-free), support points read through the L1/L2 (same address across
// the wave except at segment boundaries).
// ---------------------------------------------------------------------------
constexpr int KNN_THREADS = 64;

// LANES lists interleaved [slot][lane]: a workgroup of LANES lanes holds nsample * LANES * 8 bytes of LDS
template <int LANES = KNN_THREADS>
struct LdsList {
    float *d;
    int *i;
    __device__ __forceinline__ float &D(int s) { return d[s * LANES]; }
    __device__ __forceinline__ int &I(int s) { return i[s * LANES]; }
};

// Max-heap sift-down with the reference's exact comparison structure
// (knnquery_cuda_kernel.cu:21-36): take the right child only if strictly
// larger; stop only if root strictly larger than that child.
template <int LANES>
__device__ __forceinline__ void heap_sift(LdsList<LANES> h, int k)
{
    int root = 0, child = 1;
    while (child < k) {
        if (child + 1 < k && h.D(child + 1) > h.D(child)) ++child;
        float dr = h.D(root), dc = h.D(child);
        if (dr > dc) return;
        h.D(root) = dc; h.D(child) = dr;
        int ir = h.I(root); h.I(root) = h.I(child); h.I(child) = ir;
        root = child;
        child = 2 * root + 1;
    }
}

// qlist / qcount (nullable): process only the listed queries (the ones the fast path could not certify).
// LANES queries per workgroup: 64 up to nsample 128 (64 KB of lists), fewer for the longer lists (the 1024-slot
// lists of 16 lanes take 128 KB), so that nsample up to KMAX_HEAP fits one CU's LDS.
template <int LANES>
__global__ __launch_bounds__(LANES) void knnquery_heap_kernel(
    int b, int m, int nsample, const float *__restrict__ xyz, const float *__restrict__ new_xyz,
    const int *__restrict__ offset, const int *__restrict__ new_offset, const int *__restrict__ qlist,
    const int *__restrict__ qcount, int *__restrict__ idx, float *__restrict__ dist2)
{
    extern __shared__ float knn_lds[];
    LdsList<LANES> h{knn_lds + threadIdx.x, (int *)(knn_lds + nsample * LANES) + threadIdx.x};
    const int t = blockIdx.x * LANES + threadIdx.x;
    if (t >= (qcount ? min(*qcount, m) : m)) return;
    const int p = qlist ? qlist[t] : t;
    int bt = segment_of(p, new_offset, b);
    int start = bt ? offset[bt - 1] : 0, end = offset[bt];
    float qx = new_xyz[p * 3], qy = new_xyz[p * 3 + 1], qz = new_xyz[p * 3 + 2];
    for (int s = 0; s < nsample; ++s) { h.D(s) = 1e10f; h.I(s) = start; }
    float root = 1e10f;
    for (int i = start; i < end; ++i) {
        float d2 = sqdist3(qx, qy, qz, xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2]);
        if (d2 < root) {
            h.D(0) = d2; h.I(0) = i;
            heap_sift(h, nsample);
            root = h.D(0);
        }
    }
    for (int i = nsample - 1; i > 0; --i) {
        float t = h.D(0); h.D(0) = h.D(i); h.D(i) = t;
        int u = h.I(0); h.I(0) = h.I(i); h.I(i) = u;
        heap_sift(h, i);
    }
    for (int s = 0; s < nsample; ++s) {
        idx[(size_t)p * nsample + s] = h.I(s);
        dist2[(size_t)p * nsample + s] = h.D(s);
    }
}

// Sorted list, ascending by (d2, index): a candidate enters only if strictly
// smaller than the current k-th, and is inserted after all entries <= it.
__global__ __launch_bounds__(KNN_THREADS) void knn_sorted_kernel(
    int nq, int nr, int k, const float *__restrict__ query, const float *__restrict__ ref,
    int *__restrict__ idx, float *__restrict__ dist2)
{
    extern __shared__ float knn_lds[];
    LdsList<> h{knn_lds + threadIdx.x, (int *)(knn_lds + k * KNN_THREADS) + threadIdx.x};
    const int bi = blockIdx.y;
    const int j = blockIdx.x * KNN_THREADS + threadIdx.x;
    if (j >= nq) return;
    const float *Q = query + ((size_t)bi * nq + j) * 3;
    const float *R = ref + (size_t)bi * nr * 3;
    float qx = Q[0], qy = Q[1], qz = Q[2];
    for (int s = 0; s < k; ++s) { h.D(s) = INFINITY; h.I(s) = 0; }
    float kth = INFINITY;
    int filled = 0;
    for (int r = 0; r < nr; ++r) {
        float d = sqdist3(qx, qy, qz, R[r * 3], R[r * 3 + 1], R[r * 3 + 2]);
        if (filled == k && !(d < kth)) continue;
        int pos = filled < k ? filled : k - 1;
        while (pos > 0 && d < h.D(pos - 1)) {
            h.D(pos) = h.D(pos - 1); h.I(pos) = h.I(pos - 1);
            --pos;
        }
        h.D(pos) = d; h.I(pos) = r;
        if (filled < k) ++filled;
        kth = h.D(k - 1);
    }
    size_t o = ((size_t)bi * nq + j) * k;
    for (int s = 0; s < k; ++s) { idx[o + s] = h.I(s); dist2[o + s] = h.D(s); }
}

// ---------------------------------------------------------------------------
// Wave-cooperative sorted kNN (k <= 64): the 64 lanes each take one reference point per
// step, the wave serves QW queries whose running best-k lists live one entry per lane
// (lane i = i-th smallest, lanes >= k hold +inf).  A step costs ~10 VALU per query for all
// 64 pairs; a candidate beating the current k-th distance tau (wave-uniform) is inserted
// with one ballot (its rank = #entries <= it, i.e. after equal distances: the (d2, index)
// order, since lanes are visited in ascending index) and one wave_shr:1 DPP shift.
// Expected insertions per query are ~k ln(n/k), so the scan dominates.
// Result identical to knn_sorted_kernel / the reference contract; also serves three_nn
// (k = 3: "3 smallest by (d2, index)", interpolate_gpu.cu:31-53).
// ---------------------------------------------------------------------------
constexpr int KW_QW = 4;     // queries per wave
constexpr int KW_WAVES = 4;  // waves per block
constexpr int DPP_WAVE_SHR1 = 0x138;

__device__ __forceinline__ float dpp_wave_shr1(float v, float fill)
{
    // lane l receives lane l-1; lane 0 keeps `fill` (bound_ctrl off => old value)
    return __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp((int)__float_as_uint(fill), (int)__float_as_uint(v),
                                                                 DPP_WAVE_SHR1, 0xF, 0xF, false));
}
__device__ __forceinline__ int dpp_wave_shr1(int v, int fill)
{
    return __builtin_amdgcn_update_dpp(fill, v, DPP_WAVE_SHR1, 0xF, 0xF, false);
}

__global__ __launch_bounds__(KW_WAVES * 64) void knn_wave_kernel(
    int nq, int nr, int k, const float *__restrict__ query, const float *__restrict__ ref,
    int *__restrict__ idx, float *__restrict__ dist2)
{
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int bi = blockIdx.y;
    const int q0 = (blockIdx.x * KW_WAVES + wave) * KW_QW;
    if (q0 >= nq) return;
    const float *Q = query + (size_t)bi * nq * 3;
    const float *R = ref + (size_t)bi * nr * 3;
    float qx[KW_QW], qy[KW_QW], qz[KW_QW], ld[KW_QW], tau[KW_QW];
    int li[KW_QW];
#pragma unroll
    for (int q = 0; q < KW_QW; ++q) {
        int j = min(q0 + q, nq - 1); // tail waves recompute the last query; stores are guarded
        qx[q] = Q[j * 3]; qy[q] = Q[j * 3 + 1]; qz[q] = Q[j * 3 + 2];
        ld[q] = INFINITY; li[q] = 0; tau[q] = INFINITY;
    }
    for (int c0 = 0; c0 < nr; c0 += 64) {
        const int r = c0 + lane;
        const bool in = r < nr;
        float rx = 0.f, ry = 0.f, rz = 0.f;
        if (in) { rx = R[r * 3]; ry = R[r * 3 + 1]; rz = R[r * 3 + 2]; }
#pragma unroll
        for (int q = 0; q < KW_QW; ++q) {
            float d = sqdist3(qx[q], qy[q], qz[q], rx, ry, rz);
            unsigned long long mask = __ballot(in && d < tau[q]);
            while (mask) {
                int l = __builtin_ctzll(mask);
                mask &= mask - 1;
                float dc = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(d), l));
                if (!(dc < tau[q])) continue; // tau may have dropped within this step
                int pos = __popcll(__ballot(ld[q] <= dc));
                float sd = dpp_wave_shr1(ld[q], ld[q]);
                int si = dpp_wave_shr1(li[q], li[q]);
                ld[q] = lane > pos ? sd : (lane == pos ? dc : ld[q]);
                li[q] = lane > pos ? si : (lane == pos ? c0 + l : li[q]);
                tau[q] = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(ld[q]), k - 1));
            }
        }
    }
#pragma unroll
    for (int q = 0; q < KW_QW; ++q) {
        int j = q0 + q;
        if (j < nq && lane < k) {
            size_t o = ((size_t)bi * nq + j) * k + lane;
            idx[o] = li[q];
            dist2[o] = ld[q];
        }
    }
}

// ---- sorted kNN in D dimensions (feature space: feature_space_loss searches its neighbours among the
// 17-dimensional soft-max vectors, utils/insT_loss.py:19) ------------------------------------------------
// Same wave-cooperative scheme as knn_wave_kernel: 64 lanes = 64 reference points per step, KW_QW queries per
// wave with their coordinates in registers, best-k list one entry per lane, ties by smaller index.
// d2 = sum_j (q_j - r_j)^2 accumulated in index order, un-contracted.  D <= KN_DMAX.
constexpr int KN_DMAX = 32;

template <int DPAD>
__global__ __launch_bounds__(KW_WAVES * 64) void knn_wave_nd_kernel(
    int nq, int nr, int d, int k, const float *__restrict__ query, const float *__restrict__ ref,
    int *__restrict__ idx, float *__restrict__ dist2)
{
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int bi = blockIdx.y;
    const int q0 = (blockIdx.x * KW_WAVES + wave) * KW_QW;
    if (q0 >= nq) return;
    const float *Q = query + (size_t)bi * nq * d;
    const float *R = ref + (size_t)bi * nr * d;
    float qv[KW_QW][DPAD], ld[KW_QW], tau[KW_QW];
    int li[KW_QW];
#pragma unroll
    for (int q = 0; q < KW_QW; ++q) {
        const int j = min(q0 + q, nq - 1);
#pragma unroll
        for (int t = 0; t < DPAD; ++t) qv[q][t] = t < d ? Q[(size_t)j * d + t] : 0.f;
        ld[q] = INFINITY; li[q] = 0; tau[q] = INFINITY;
    }
    for (int c0 = 0; c0 < nr; c0 += 64) {
        const int r = c0 + lane;
        const bool in = r < nr;
        float rv[DPAD];
#pragma unroll
        for (int t = 0; t < DPAD; ++t) rv[t] = (in && t < d) ? R[(size_t)r * d + t] : 0.f;
#pragma unroll
        for (int q = 0; q < KW_QW; ++q) {
            float dd = 0.f;
#pragma unroll
            for (int t = 0; t < DPAD; ++t) {
                const float df = qv[q][t] - rv[t]; // padded dimensions contribute exactly 0
                dd = dd + df * df;
            }
            unsigned long long mask = __ballot(in && dd < tau[q]);
            while (mask) {
                const int l = __builtin_ctzll(mask);
                mask &= mask - 1;
                const float dc = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(dd), l));
                if (!(dc < tau[q])) continue;
                const int pos = __popcll(__ballot(ld[q] <= dc));
                const float sd = dpp_wave_shr1(ld[q], ld[q]);
                const int si = dpp_wave_shr1(li[q], li[q]);
                ld[q] = lane > pos ? sd : (lane == pos ? dc : ld[q]);
                li[q] = lane > pos ? si : (lane == pos ? c0 + l : li[q]);
                tau[q] = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(ld[q]), k - 1));
            }
        }
    }
#pragma unroll
    for (int q = 0; q < KW_QW; ++q) {
        const int j = q0 + q;
        if (j < nq && lane < k) {
            const size_t o = ((size_t)bi * nq + j) * k + lane;
            idx[o] = li[q];
            dist2[o] = ld[q];
        }
    }
}

// ---------------------------------------------------------------------------
// Sorted kNN for long lists (65 <= k <= KMAX_SORTED): one workgroup per query.
//   1. every squared distance, as its IEEE bits (a non-negative float orders like its bits), kept in LDS when the
//      cloud fits (`cache`), recomputed from the L2-resident coordinates on every pass otherwise; min / max of the keys;
//   2. radix select of the k-th smallest key T over the key range [min, max]: each pass histograms the keys still in
//      the candidate range by their next 11 bits (int LDS atomics), one wave finds the bin that holds rank k and the
//      range shrinks to it -- at most three passes for 32-bit keys;
//   3. one pass in index order collects every key < T (unordered) and the first k - #(< T) keys == T by ascending
//      index (a block-wide prefix count), so the selected set is the k smallest by (d2, index);
//   4. a bitonic sort of the (d2 bits << 32 | index) words in LDS gives the (d2, index) order.
// Slots beyond nr are (inf, 0).  `cert_ns` > 0 is pointops.knn's fast path (k = cert_ns + 1): a query whose k sorted
// distances are strictly increasing and below the heap's 1e10 sentinel has the literal heap's answer, which is written
// (cert_ns slots, global indices bi * nr + r); the others are appended to qlist for the literal heap.
// ---------------------------------------------------------------------------
constexpr int KS_BITS = 11;
constexpr int KS_BINS = 1 << KS_BITS;
constexpr int KS_RED = 128;       // LDS words: [0,16) min, [16,32) max, [32,34) select, [36] count, [37] flag, [64,80) waves
constexpr int KS_CACHE_THREADS = 1024;

__host__ __device__ constexpr int ks_pow2(int k)
{
    int n = 2;
    while (n < k) n <<= 1;
    return n;
}

__global__ __launch_bounds__(KS_CACHE_THREADS) void knn_select_kernel(
    int nq, int nr, int k, int cache, const float *__restrict__ query, const float *__restrict__ ref,
    int *__restrict__ idx, float *__restrict__ dist2, int cert_ns, int *__restrict__ qlist, int *__restrict__ qcount)
{
    extern __shared__ unsigned long long ks_lds[];
    const int n2 = ks_pow2(k);
    unsigned long long *cand = ks_lds;
    uint32_t *hist = (uint32_t *)(cand + n2);
    uint32_t *red = hist + KS_BINS;
    uint32_t *ck = red + KS_RED;                       // the key cache (nr words) when `cache`
    const int tid = threadIdx.x, T = blockDim.x, lane = lane_id(), wave = tid >> 6, W = T >> 6;
    const int bi = blockIdx.y, j = blockIdx.x;
    const float *Q = query + ((size_t)bi * nq + j) * 3;
    const float *R = ref + (size_t)bi * nr * 3;
    const float qx = Q[0], qy = Q[1], qz = Q[2];
    auto key_of = [&](int r) -> uint32_t {
        return cache ? ck[r] : __float_as_uint(sqdist3(qx, qy, qz, R[r * 3], R[r * 3 + 1], R[r * 3 + 2]));
    };

    // 1. keys, their min and max
    uint32_t kmin = 0xffffffffu, kmax = 0u;
    for (int r = tid; r < nr; r += T) {
        const uint32_t key = __float_as_uint(sqdist3(qx, qy, qz, R[r * 3], R[r * 3 + 1], R[r * 3 + 2]));
        if (cache) ck[r] = key;
        kmin = min(kmin, key);
        kmax = max(kmax, key);
    }
    kmin = wave_min_u32(kmin);
    kmax = wave_max_u32(kmax);
    if (lane == 0) { red[wave] = kmin; red[16 + wave] = kmax; }
    __syncthreads();
    for (int w = 0; w < W; ++w) { kmin = min(kmin, red[w]); kmax = max(kmax, red[16 + w]); }

    // 2. radix select: the keys < lo number `below`, the wanted key has rank `want` (1-based) within [lo, hi]
    const bool all = nr <= k;                          // every point is a neighbour
    uint32_t lo = kmin, hi = kmax;
    int below = 0, want = k;
    while (!all && hi != lo) {
        const uint32_t range = hi - lo;
        const int width = 32 - __clz(range);
        const int shift = width > KS_BITS ? width - KS_BITS : 0;
        const int nb = (int)(range >> shift) + 1;
        for (int i = tid; i < nb; i += T) hist[i] = 0u;
        __syncthreads();
        for (int r = tid; r < nr; r += T) {
            const uint32_t key = key_of(r);
            if (key >= lo && key <= hi) atomicAdd(&hist[(key - lo) >> shift], 1u);
        }
        __syncthreads();
        if (wave == 0) {                               // 32 bins per lane, scan over the lanes
            constexpr int PER = KS_BINS / 64;
            int sum = 0;
            for (int e = 0; e < PER; ++e) sum += lane * PER + e < nb ? (int)hist[lane * PER + e] : 0;
            int inc = sum;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(inc, d);
                if (lane >= d) inc += o;
            }
            int run = inc - sum;
            if (run < want && want <= inc) {
                for (int e = 0; e < PER; ++e) {
                    const int c = lane * PER + e < nb ? (int)hist[lane * PER + e] : 0;
                    if (run + c >= want) { red[32] = (uint32_t)(lane * PER + e); red[33] = (uint32_t)run; break; }
                    run += c;
                }
            }
        }
        __syncthreads();
        const uint32_t bin = red[32];
        const int before = (int)red[33];
        below += before;
        want -= before;
        lo += bin << shift;
        const unsigned long long top = (unsigned long long)lo + ((1ull << shift) - 1ull);
        hi = top < (unsigned long long)hi ? (uint32_t)top : hi;
        if (shift == 0) break;                         // (red[32..33] are rewritten only after the next two barriers)
    }
    const uint32_t thr = lo;                           // the k-th smallest key; `want` keys == thr are taken

    // 3. collect: keys < thr anywhere in [0, below), keys == thr in index order into [below, k)
    if (tid == 0) { red[36] = 0u; red[37] = 0u; }
    __syncthreads();
    int eq_seen = 0;
    for (int c0 = 0; c0 < nr; c0 += T) {
        const int r = c0 + tid;
        const uint32_t key = r < nr ? key_of(r) : 0xffffffffu;
        const bool lt = r < nr && (all || key < thr);
        const unsigned long long mlt = __ballot(lt);
        if (mlt) {
            int base = 0;
            if (lane == 0) base = (int)atomicAdd(&red[36], (uint32_t)__popcll(mlt));
            base = __shfl(base, 0);
            if (lt) cand[base + __popcll(mlt & ((1ull << lane) - 1ull))] = ((unsigned long long)key << 32) | (uint32_t)r;
        }
        if (!all && eq_seen < want) {                  // block-uniform
            const bool eq = r < nr && key == thr;
            const unsigned long long meq = __ballot(eq);
            if (lane == 0) red[64 + wave] = (uint32_t)__popcll(meq);
            __syncthreads();
            int off = eq_seen, tot = 0;
            for (int w = 0; w < W; ++w) {
                const int c = (int)red[64 + w];
                off += w < wave ? c : 0;
                tot += c;
            }
            const int rank = off + __popcll(meq & ((1ull << lane) - 1ull));
            if (eq && rank < want) cand[below + rank] = ((unsigned long long)key << 32) | (uint32_t)r;
            eq_seen += tot;
            __syncthreads();
        }
    }
    const int n = all ? nr : k;
    for (int s = n + tid; s < n2; s += T) cand[s] = ~0ull;
    __syncthreads();

    // 4. bitonic sort of the n2 words
    for (int size = 2; size <= n2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < (n2 >> 1); i += T) {
                const int a = 2 * i - (i & (stride - 1)), c = a + stride;
                const unsigned long long x = cand[a], y = cand[c];
                if ((x > y) == ((a & size) == 0)) { cand[a] = y; cand[c] = x; }
            }
            __syncthreads();
        }
    }

    const size_t p = (size_t)bi * nq + j;
    if (cert_ns == 0) {
        for (int s = tid; s < k; s += T) {
            const unsigned long long v = cand[s];
            idx[p * k + s] = s < n ? (int)(uint32_t)v : 0;
            dist2[p * k + s] = s < n ? __uint_as_float((uint32_t)(v >> 32)) : INFINITY;
        }
        return;
    }
    bool strict = !all || nr > cert_ns;                // k = cert_ns + 1 real candidates are needed
    for (int s = tid; s < cert_ns && strict; s += T)
        strict = __uint_as_float((uint32_t)(cand[s] >> 32)) < __uint_as_float((uint32_t)(cand[s + 1] >> 32));
    if (tid == 0) strict = strict && __uint_as_float((uint32_t)(cand[cert_ns] >> 32)) < 1e10f;
    if (!strict) red[37] = 1u;                         // (same value from every writer)
    __syncthreads();
    if (red[37] == 0u) {
        for (int s = tid; s < cert_ns; s += T) {
            const unsigned long long v = cand[s];
            idx[p * cert_ns + s] = bi * nr + (int)(uint32_t)v;
            dist2[p * cert_ns + s] = __uint_as_float((uint32_t)(v >> 32));
        }
    } else if (tid == 0) {
        qlist[atomicAdd(qcount, 1)] = (int)p;
    }
}

// LDS of knn_select_kernel: the sort words, the histogram, the reduction words and (cache) one key per point
static size_t ks_lds_bytes(int k, int nr, bool cache)
{
    return (size_t)ks_pow2(k) * 8 + (size_t)(KS_BINS + KS_RED) * 4 + (cache ? (size_t)nr * 4 : 0);
}

static hipError_t launch_knn_select(int b, int nq, int nr, int k, const float *query, const float *ref, int *idx,
                                    float *dist2, int cert_ns, int *qlist, int *qcount, hipStream_t s)
{
    const bool cache = ks_lds_bytes(k, nr, true) <= (size_t)160 * 1024;
    const size_t lds = ks_lds_bytes(k, nr, cache);
    hipError_t e = allow_big_lds((const void *)knn_select_kernel, lds);
    if (e != hipSuccess) return e;
    const int threads = nr >= 4096 ? KS_CACHE_THREADS : 256;
    hipLaunchKernelGGL(knn_select_kernel, dim3(nq, b), dim3(threads), lds, s, nq, nr, k, cache ? 1 : 0, query, ref, idx,
                       dist2, cert_ns, qlist, qcount);
    return hipGetLastError();
}

static bool nn_impl_basic()
{
    const char *e = getenv("GEOT_NN_IMPL"); // "basic" = the one-lane-per-query kernels (A/B testing)
    return e && e[0] == 'b';
}

template <int LANES>
static hipError_t launch_heap(int b, int m, int nsample, const float *xyz, const float *new_xyz, const int *offset,
                              const int *new_offset, const int *qlist, const int *qcount, int *idx, float *dist2,
                              hipStream_t s)
{
    const size_t lds = (size_t)nsample * LANES * 8;
    hipError_t e = allow_big_lds((const void *)knnquery_heap_kernel<LANES>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(knnquery_heap_kernel<LANES>, dim3((int)(((long long)m + LANES - 1) / LANES)), dim3(LANES), lds, s,
                       b, m, nsample, xyz, new_xyz, offset, new_offset, qlist, qcount, idx, dist2);
    return hipGetLastError();
}

// the literal heap: 64 lanes per workgroup up to nsample 128 (GEOT_NN_IMPL=basic: up to 256, 128 KB), 32 lanes up to
// 256 and 16 lanes up to KMAX_HEAP (64 / 128 KB), so that the lists always fit
static hipError_t launch_heap_any(int b, int m, int nsample, const float *xyz, const float *new_xyz, const int *offset,
                                  const int *new_offset, const int *qlist, const int *qcount, int *idx, float *dist2,
                                  hipStream_t s)
{
    if (nsample <= 128 || (nsample <= 256 && nn_impl_basic()))
        return launch_heap<64>(b, m, nsample, xyz, new_xyz, offset, new_offset, qlist, qcount, idx, dist2, s);
    if (nsample <= 256)
        return launch_heap<32>(b, m, nsample, xyz, new_xyz, offset, new_offset, qlist, qcount, idx, dist2, s);
    return launch_heap<16>(b, m, nsample, xyz, new_xyz, offset, new_offset, qlist, qcount, idx, dist2, s);
}

static inline int grid_cap(long long want, int cap) { return (int)(want < cap ? (want < 1 ? 1 : want) : cap); }

} // namespace geot

using namespace geot;

GEOT_EXPORT int geot_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz,
                                const float *xyz, int *idx, void *stream)
{
    if (b < 0 || n < 0 || m < 0 || nsample < 0) return hipErrorInvalidValue;
    if (b == 0 || m == 0 || nsample == 0) return hipSuccess;
    size_t lds = (size_t)BQ_WAVES * nsample * sizeof(int);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    long long blocks = ((long long)b * m + BQ_WAVES - 1) / BQ_WAVES;
    hipLaunchKernelGGL(ball_query_kernel, dim3(grid_cap(blocks, 1 << 16)), dim3(BQ_WAVES * 64), lds,
                       (hipStream_t)stream, b, n, m, radius, nsample, new_xyz, xyz, idx);
    return hipGetLastError();
}

GEOT_EXPORT int geot_ballquery_offset(int b, int m, float radius, int nsample, const float *xyz,
                                      const float *new_xyz, const int *offset, const int *new_offset,
                                      int *idx, void *stream)
{
    if (b < 0 || m < 0 || nsample < 0) return hipErrorInvalidValue;
    if (b == 0 || m == 0 || nsample == 0) return hipSuccess;
    size_t lds = (size_t)BQ_WAVES * nsample * sizeof(int);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    long long blocks = ((long long)m + BQ_WAVES - 1) / BQ_WAVES;
    hipLaunchKernelGGL(ballquery_offset_kernel, dim3(grid_cap(blocks, 1 << 16)), dim3(BQ_WAVES * 64),
                       lds, (hipStream_t)stream, b, m, radius, nsample, xyz, new_xyz, offset,
                       new_offset, idx);
    return hipGetLastError();
}

GEOT_EXPORT int geot_three_nn(int b, int n, int m, const float *unknown, const float *known,
                              float *dist2, int *idx, void *stream)
{
    if (b < 0 || n < 0 || m < 0) return hipErrorInvalidValue;
    if (b == 0 || n == 0) return hipSuccess;
    if (b > 65535) return hipErrorInvalidValue;
    const char *e = getenv("GEOT_NN_IMPL"); // "basic" = one-lane-per-query kernels (A/B testing)
    if (e && e[0] == 'b') {
        hipLaunchKernelGGL(three_nn_kernel, dim3((n + NN_THREADS - 1) / NN_THREADS, b), dim3(NN_THREADS), 0,
                           (hipStream_t)stream, n, m, unknown, known, dist2, idx);
    } else {
        int per_block = KW_WAVES * KW_QW;
        hipLaunchKernelGGL(knn_wave_kernel, dim3((n + per_block - 1) / per_block, b), dim3(KW_WAVES * 64), 0,
                           (hipStream_t)stream, n, m, 3, unknown, known, idx, dist2);
    }
    return hipGetLastError();
}

GEOT_EXPORT int geot_knnquery_heap(int b, int m, int nsample, const float *xyz, const float *new_xyz,
                                   const int *offset, const int *new_offset, int *idx, float *dist2,
                                   void *stream)
{
    if (b < 0 || m < 0 || nsample < 0 || nsample > GEOT_KNN_KMAX_HEAP) return hipErrorInvalidValue;
    if (b == 0 || m == 0 || nsample == 0) return hipSuccess;
    return launch_heap_any(b, m, nsample, xyz, new_xyz, offset, new_offset, nullptr, nullptr, idx, dist2,
                           (hipStream_t)stream);
}

// ---- pointops kNN, fast path for uniform batches ------------------------------------------------
// The reference's max-heap + heap-sort (knnquery_cuda_kernel.cu:21-108) returns the k nearest in ascending
// order; only the order among EQUAL distances depends on the heap mechanics.  So: sorted (k+1)-NN from the
// exact grid search; a query whose first k+1 distances are strictly increasing has a unique answer, which
// is copied; the others (duplicates, lattice ties, fewer than k+1 candidates) are listed and go through the
// literal heap kernel.  Identical output to geot_knnquery_heap.  From nsample 64 on, the sorted (k+1)-NN comes from
// knn_select_kernel, which certifies in its epilogue (same rule), so the workspace is only the query list.
__global__ __launch_bounds__(256) void knn_heap_certify_kernel(int m_total, int m_per, int n_per, int k,
                                                               const int *__restrict__ tidx, const float *__restrict__ td2,
                                                               int *__restrict__ idx, float *__restrict__ dist2,
                                                               int *__restrict__ qlist, int *__restrict__ qcount)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= m_total) return;
    const float *d = td2 + (size_t)p * (k + 1);
    bool strict = d[k] < 1e10f; // the heap never takes distances >= its 1e10 initial root
    for (int s = 0; s < k; ++s) strict = strict && d[s] < d[s + 1];
    if (strict) {
        const int base = (p / m_per) * n_per; // global index of the batch's first support point
        for (int s = 0; s < k; ++s) {
            idx[(size_t)p * k + s] = base + tidx[(size_t)p * (k + 1) + s];
            dist2[(size_t)p * k + s] = d[s];
        }
    } else {
        qlist[atomicAdd(qcount, 1)] = p;
    }
}

extern "C" long long geot_knn_grid_ws_bytes(int b, int nr);
extern "C" int geot_knn_grid_eligible(int b, int nq, int nr, int k);
extern "C" int geot_knn_sorted_ws(int b, int nq, int nr, int k, const float *query, const float *ref, int *idx,
                                  float *dist2, void *workspace, long long ws_bytes, void *stream);

constexpr int KNN_CERT_MIN = 64;   // nsample from which pointops.knn's fast path is knn_select_kernel's certification

// 1 if geot_knnquery_heap_ws certifies through knn_select_kernel (its workspace: the query list and its count)
static bool knn_heap_select_eligible(int b, int nsample)
{
    return nsample >= KNN_CERT_MIN && nsample <= GEOT_KNN_KMAX_HEAP && b <= 65535 && !nn_impl_basic();
}

GEOT_EXPORT long long geot_knnquery_heap_ws_bytes(int b, int n_per, int m_per, int nsample)
{
    if (b < 0 || n_per < 0 || m_per < 0 || nsample < 0) return -1;
    const long long mt = (long long)b * m_per;
    if (nsample >= KNN_CERT_MIN) return (4 * (mt + 4) + 15) & ~15LL;
    long long bytes = geot_knn_grid_ws_bytes(b, n_per);
    bytes += 4 * (2 * mt * (nsample + 1) + mt + 4);
    return (bytes + 15) & ~15LL;
}

GEOT_EXPORT int geot_knnquery_heap_ws(int b, int n_per, int m_per, int nsample, const float *xyz,
                                      const float *new_xyz, const int *offset, const int *new_offset, int *idx,
                                      float *dist2, void *workspace, long long ws_bytes, void *stream)
{
    if (b < 0 || n_per < 0 || m_per < 0 || nsample < 0 || nsample > GEOT_KNN_KMAX_HEAP) return hipErrorInvalidValue;
    const long long mt = (long long)b * m_per;
    if (b == 0 || mt == 0 || nsample == 0) return hipSuccess;
    if (mt > 0x7fffffffLL) return hipErrorInvalidValue;
    const bool usable = workspace && ws_bytes >= geot_knnquery_heap_ws_bytes(b, n_per, m_per, nsample) &&
                        ((uintptr_t)workspace & 15) == 0;
    hipStream_t s = (hipStream_t)stream;
    if (usable && knn_heap_select_eligible(b, nsample)) {
        int *qlist = (int *)workspace;
        int *qcount = qlist + mt;
        hipError_t e = zero_words(qcount, 1, s);
        if (e != hipSuccess) return e;
        e = launch_knn_select(b, m_per, n_per, nsample + 1, new_xyz, xyz, idx, dist2, nsample, qlist, qcount, s);
        if (e != hipSuccess) return e;
        return launch_heap_any(b, (int)mt, nsample, xyz, new_xyz, offset, new_offset, qlist, qcount, idx, dist2, s);
    }
    if (!usable || nsample >= KNN_CERT_MIN || !geot_knn_grid_eligible(b, m_per, n_per, nsample + 1))
        return geot_knnquery_heap(b, (int)mt, nsample, xyz, new_xyz, offset, new_offset, idx, dist2, stream);
    const long long gbytes = geot_knn_grid_ws_bytes(b, n_per);
    int *tidx = (int *)((char *)workspace + gbytes);
    float *td2 = (float *)(tidx + mt * (nsample + 1));
    int *qlist = (int *)(td2 + mt * (nsample + 1));
    int *qcount = qlist + mt;
    hipError_t e = zero_words(qcount, 1, s);
    if (e != hipSuccess) return e;
    int rc = geot_knn_sorted_ws(b, m_per, n_per, nsample + 1, new_xyz, xyz, tidx, td2, workspace, gbytes, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(knn_heap_certify_kernel, dim3((int)((mt + 255) / 256)), dim3(256), 0, s, (int)mt, m_per, n_per,
                       nsample, tidx, td2, idx, dist2, qlist, qcount);
    return launch_heap_any(b, (int)mt, nsample, xyz, new_xyz, offset, new_offset, qlist, qcount, idx, dist2, s);
}

GEOT_EXPORT int geot_knn_sorted(int b, int nq, int nr, int k, const float *query, const float *ref,
                                int *idx, float *dist2, void *stream)
{
    if (b < 0 || nq < 0 || nr < 0 || k < 0 || k > GEOT_KNN_KMAX_SORTED) return hipErrorInvalidValue;
    if (b == 0 || nq == 0 || k == 0) return hipSuccess;
    if (b > 65535) return hipErrorInvalidValue;
    const bool basic = nn_impl_basic();
    if (k <= 64 && !basic) {
        int per_block = KW_WAVES * KW_QW;
        hipLaunchKernelGGL(knn_wave_kernel, dim3((nq + per_block - 1) / per_block, b), dim3(KW_WAVES * 64), 0,
                           (hipStream_t)stream, nq, nr, k, query, ref, idx, dist2);
        return hipGetLastError();
    }
    if (k > 256 || (k > 64 && !basic))
        return launch_knn_select(b, nq, nr, k, query, ref, idx, dist2, 0, nullptr, nullptr, (hipStream_t)stream);
    // GEOT_NN_IMPL=basic, k <= 256: the one-lane-per-query insertion kernel (A/B runs)
    size_t lds = (size_t)k * KNN_THREADS * 8;
    hipError_t e = allow_big_lds((const void *)knn_sorted_kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(knn_sorted_kernel, dim3((nq + KNN_THREADS - 1) / KNN_THREADS, b),
                       dim3(KNN_THREADS), lds, (hipStream_t)stream, nq, nr, k, query, ref, idx, dist2);
    return hipGetLastError();
}

GEOT_EXPORT int geot_knn_sorted_nd(int b, int nq, int nr, int d, int k, const float *query, const float *ref,
                                   int *idx, float *dist2, void *stream)
{
    if (b < 0 || nq < 0 || nr < 0 || d < 1 || d > KN_DMAX || k < 1 || k > 64) return hipErrorInvalidValue;
    if (b == 0 || nq == 0) return hipSuccess;
    if (b > 65535) return hipErrorInvalidValue;
    const int per_block = KW_WAVES * KW_QW;
    const dim3 grid((nq + per_block - 1) / per_block, b);
    if (d <= 8)
        hipLaunchKernelGGL(knn_wave_nd_kernel<8>, grid, dim3(KW_WAVES * 64), 0, (hipStream_t)stream, nq, nr, d, k, query, ref,
                           idx, dist2);
    else if (d <= 20)
        hipLaunchKernelGGL(knn_wave_nd_kernel<20>, grid, dim3(KW_WAVES * 64), 0, (hipStream_t)stream, nq, nr, d, k, query,
                           ref, idx, dist2);
    else
        hipLaunchKernelGGL(knn_wave_nd_kernel<32>, grid, dim3(KW_WAVES * 64), 0, (hipStream_t)stream, nq, nr, d, k, query,
                           ref, idx, dist2);
    return hipGetLastError();
}
