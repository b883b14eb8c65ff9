// Whole-scan predictions refined by the majority of their nearest vertices (geot_scan_refine): part_seg_refinement
// (train.py:57-73) on per-vertex labels as geot_scan_predict / geot_scan_vote write them, for all batch slots in six launches
// whatever the slots, their sizes and their labels, without a host synchronisation.  See include/geot_hip.h for the rules.
//
//   zero     the per-slot records of the workspace
//   census   per slot and class the member count and the first vertex index: LDS integer atomics per workgroup, then one
//            global atomicAdd / atomicMax per class and workgroup.  The first index is kept as max(~v), so that zero means "none"
//   plan     one wave per slot: the classes to refine (count < n or not allowed, more than one class present), ordered by first
//            index, each with a segment [start, start + count) of the slot's query list
//   collect  every vertex whose label is a planned class appends its index to the class's segment; ranks come from an LDS
//            counter per 256 vertices and one global cursor add per class and chunk.  The order inside a segment is arbitrary and
//            no result depends on it
//   search   waves share out all slots' queries round-robin (the counts are read from the records); one wave per query scans
//            the scan's vertices in place, 64 per step, through kg_offer with k = n + 1 -- scan_predict.hip's brute-force form --
//            and writes the k vertex indices (-1: never filled).  The search reads no labels, so one pass serves every step
//   vote     one workgroup per slot walks the planned classes in order: a thread per query counts its neighbours' current
//            labels in four packed 64-bit words (8 bits per class: counts stay <= 64), clears class i, takes the first maximum
//            and stages it in the query's own neighbour row; after a barrier the staged labels are written, after another the
//            next class starts
#include "geot_common.h"
#include "geot_hip.h"
#include "knn_grid.h"

namespace geot {

constexpr int SR_C = GEOT_NTM_MAX_C;
// one slot's record, 32-bit words
constexpr int SR_CNT = 0, SR_KEY = SR_C, SR_CUR = 2 * SR_C, SR_SEG = 3 * SR_C, SR_ORD = 4 * SR_C, SR_MISC = 5 * SR_C;
constexpr int SR_BAD = SR_MISC, SR_STEPS = SR_MISC + 1, SR_NQ = SR_MISC + 2;
constexpr int SR_REC = 5 * SR_C + 8;
constexpr int SR_THREADS = 256;
constexpr int SR_SEARCH_BLOCKS = 2048;     // x 4 waves: one round of the device at full occupancy
constexpr int SR_VOTE_THREADS = 1024;

struct SrSlot {
    long long lo, out0;
    int size;             // 0: the slot is skipped
};
// geot_scan_predict's skip rules, and room for the slot in a workspace of `cap` vertices
__device__ __forceinline__ SrSlot sr_slot(int s, int n_scans, long long total, const long long *__restrict__ offsets,
                                          const long long *__restrict__ scan_ids, const long long *__restrict__ out_offsets,
                                          long long cap)
{
    SrSlot r = {0, 0, 0};
    const long long sid = scan_ids[s];
    if (sid < 0 || sid >= n_scans) return r;
    const long long lo = offsets[sid], hi = offsets[sid + 1];
    if (lo < 0 || hi <= lo || hi > total || hi - lo > 0x7fffffffll) return r;
    const long long o = out_offsets[s];
    if (o < 0 || o > cap - (hi - lo)) return r;
    r.lo = lo;
    r.out0 = o;
    r.size = (int)(hi - lo);
    return r;
}

__global__ __launch_bounds__(SR_THREADS) void sr_census_kernel(int c, int n_scans, long long total,
                                                               const long long *__restrict__ offsets,
                                                               const long long *__restrict__ scan_ids,
                                                               const long long *__restrict__ out_offsets, long long cap,
                                                               const long long *__restrict__ pred, unsigned *__restrict__ head)
{
    __shared__ unsigned cnt[SR_C], key[SR_C], bad;
    const int s = blockIdx.y, tid = threadIdx.x;
    const SrSlot sl = sr_slot(s, n_scans, total, offsets, scan_ids, out_offsets, cap);
    if (!sl.size) return;
    if (tid < SR_C) { cnt[tid] = 0; key[tid] = 0; }
    if (tid == 0) bad = 0;
    __syncthreads();
    for (long long v = (long long)blockIdx.x * SR_THREADS + tid; v < sl.size; v += (long long)gridDim.x * SR_THREADS) {
        const long long p = pred[sl.out0 + v];
        if (p >= 0 && p < c) {
            atomicAdd(&cnt[p], 1u);
            atomicMax(&key[p], ~(unsigned)v);
        } else {
            atomicAdd(&bad, 1u);
        }
    }
    __syncthreads();
    unsigned *R = head + (size_t)s * SR_REC;
    if (tid < c && cnt[tid]) {
        atomicAdd(&R[SR_CNT + tid], cnt[tid]);
        atomicMax(&R[SR_KEY + tid], key[tid]);
    }
    if (tid == 0 && bad) atomicAdd(&R[SR_BAD], bad);
}

__global__ __launch_bounds__(64) void sr_plan_kernel(int c, int n, int n_scans, long long total,
                                                     const long long *__restrict__ offsets,
                                                     const long long *__restrict__ scan_ids,
                                                     const long long *__restrict__ out_offsets, long long cap,
                                                     const unsigned *__restrict__ allowed, unsigned *__restrict__ head)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    int *R = reinterpret_cast<int *>(head + (size_t)s * SR_REC);
    const SrSlot sl = sr_slot(s, n_scans, total, offsets, scan_ids, out_offsets, cap);
    const int cnt = sl.size && lane < c ? R[SR_CNT + lane] : 0;
    const unsigned first = lane < c ? ~(unsigned)R[SR_KEY + lane] : 0u;
    const int present = __popcll(__ballot(cnt > 0));
    const unsigned ok = allowed ? allowed[s] : 0xffffffffu;
    const bool planned = cnt > 0 && present > 1 && (cnt < n || !((ok >> (lane & 31)) & 1u));
    int rank = 0, start = 0;
    for (int j = 0; j < c; ++j) {
        const bool pj = __shfl((int)planned, j) != 0;
        const unsigned fj = (unsigned)__shfl((int)first, j);
        const int cj = __shfl(cnt, j);
        if (pj && fj < first) { ++rank; start += cj; }
    }
    if (lane < SR_C) R[SR_SEG + lane] = planned ? start : -1;
    if (planned) R[SR_ORD + rank] = lane;
    const unsigned long long pm = __ballot(planned);
    int nq = planned ? cnt : 0;
    for (int d = 32; d >= 1; d >>= 1) nq += __shfl_xor(nq, d);
    if (lane == 0) { R[SR_STEPS] = __popcll(pm); R[SR_NQ] = nq; }
}

__global__ __launch_bounds__(SR_THREADS) void sr_collect_kernel(int c, int n_scans, long long total,
                                                                const long long *__restrict__ offsets,
                                                                const long long *__restrict__ scan_ids,
                                                                const long long *__restrict__ out_offsets, long long cap,
                                                                const long long *__restrict__ pred, unsigned *__restrict__ head,
                                                                int *__restrict__ qlist)
{
    __shared__ int seg[SR_C], lcnt[SR_C], lbase[SR_C];
    const int s = blockIdx.y, tid = threadIdx.x;
    int *R = reinterpret_cast<int *>(head + (size_t)s * SR_REC);
    if (R[SR_NQ] == 0) return;            // uniform over the workgroup; a skipped slot has no queries
    const SrSlot sl = sr_slot(s, n_scans, total, offsets, scan_ids, out_offsets, cap);
    if (!sl.size) return;
    if (tid < SR_C) seg[tid] = tid < c ? R[SR_SEG + tid] : -1;
    for (long long base = (long long)blockIdx.x * SR_THREADS; base < sl.size; base += (long long)gridDim.x * SR_THREADS) {
        if (tid < SR_C) lcnt[tid] = 0;
        __syncthreads();
        const long long v = base + tid;
        int cls = -1, rank = 0;
        if (v < sl.size) {
            const long long p = pred[sl.out0 + v];
            if (p >= 0 && p < c && seg[p] >= 0) {
                cls = (int)p;
                rank = atomicAdd(&lcnt[cls], 1);
            }
        }
        __syncthreads();
        if (tid < c && lcnt[tid] > 0) lbase[tid] = atomicAdd(&R[SR_CUR + tid], lcnt[tid]);
        __syncthreads();
        if (cls >= 0) {
            const int at = seg[cls] + lbase[cls] + rank;
            if (at >= 0 && at < sl.size) qlist[sl.out0 + at] = (int)v;      // (always: the segments partition [0, queries))
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(SR_THREADS) void sr_search_kernel(int b, int k, int n_scans, long long total,
                                                               const float *__restrict__ points,
                                                               const long long *__restrict__ offsets,
                                                               const long long *__restrict__ scan_ids,
                                                               const long long *__restrict__ out_offsets, long long cap,
                                                               const unsigned *__restrict__ head, const int *__restrict__ qlist,
                                                               int *__restrict__ nbr)
{
    const int lane = lane_id();
    const long long W = (long long)gridDim.x * (SR_THREADS / GEOT_WAVE);
    const long long wid = (long long)blockIdx.x * (SR_THREADS / GEOT_WAVE) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    long long before = 0;                 // queries of the slots in front: query g of all belongs to wave g mod W
    for (int s0 = 0; s0 < b; s0 += 64) {
        const int mine = s0 + lane < b ? (int)head[(size_t)(s0 + lane) * SR_REC + SR_NQ] : 0;
        unsigned long long live = __ballot(mine > 0);
        while (live) {
            const int l = __builtin_ctzll(live);
            live &= live - 1;
            const int nq = __builtin_amdgcn_readlane(mine, l);
            long long q0 = (wid - before) % W;
            if (q0 < 0) q0 += W;
            before += nq;
            if (q0 >= nq) continue;
            const int s = s0 + l;
            const SrSlot sl = sr_slot(s, n_scans, total, offsets, scan_ids, out_offsets, cap);
            if (!sl.size || nq > sl.size) continue;
            const float *V = points + (size_t)sl.lo * 3;
            for (long long q = q0; q < nq; q += W) {
                const int v = qlist[sl.out0 + q];
                float qx = 0.f, qy = 0.f, qz = 0.f;
                if (v >= 0 && v < sl.size) { qx = V[(size_t)v * 3]; qy = V[(size_t)v * 3 + 1]; qz = V[(size_t)v * 3 + 2]; }
                KgBest B;
                B.ld = INFINITY; B.li = 0; B.tau = INFINITY; B.taui = 0;
                for (int c0 = 0; c0 < sl.size; c0 += 64) {
                    const int r = c0 + lane;
                    const bool in = r < sl.size;
                    float px = 0.f, py = 0.f, pz = 0.f;
                    if (in) { px = V[(size_t)r * 3]; py = V[(size_t)r * 3 + 1]; pz = V[(size_t)r * 3 + 2]; }
                    kg_offer(in, sqdist3(qx, qy, qz, px, py, pz), r, k, B);
                }
                // infinite distances are never inserted: an entry still at +inf was never filled
                if (lane < k) nbr[(size_t)(sl.out0 + q) * k + lane] = B.ld < INFINITY ? B.li : -1;
            }
        }
    }
}

__global__ __launch_bounds__(SR_VOTE_THREADS) void sr_vote_kernel(int c, int k, int n_scans, long long total,
                                                                  const long long *__restrict__ offsets,
                                                                  const long long *__restrict__ scan_ids,
                                                                  const long long *__restrict__ out_offsets, long long cap,
                                                                  const unsigned *__restrict__ head, const int *__restrict__ qlist,
                                                                  int *nbr, long long *pred, int *__restrict__ stats)
{
    __shared__ int changed;
    const int s = blockIdx.x, tid = threadIdx.x;
    const int *R = reinterpret_cast<const int *>(head + (size_t)s * SR_REC);
    const SrSlot sl = sr_slot(s, n_scans, total, offsets, scan_ids, out_offsets, cap);
    const int steps = sl.size ? R[SR_STEPS] : 0;
    if (tid == 0) changed = 0;
    int moved = 0;
    for (int j = 0; j < steps; ++j) {
        const int i = R[SR_ORD + j];
        if (i < 0 || i >= c) break;                   // (never: the plan wrote `steps` classes)
        const int start = R[SR_SEG + i], members = R[SR_CNT + i];
        if (start < 0 || members > sl.size - start) break;
        int *rows = nbr + (size_t)(sl.out0 + start) * k;
        for (int q = tid; q < members; q += SR_VOTE_THREADS) {
            int *row = rows + (size_t)q * k;
            unsigned long long w[4] = {0ull, 0ull, 0ull, 0ull};
            for (int e = 0; e < k; ++e) {
                const int nb = row[e];
                if (nb < 0 || nb >= sl.size) continue;
                const long long p = pred[sl.out0 + nb];
                if (p < 0 || p >= c) continue;
                const unsigned long long one = 1ull << (((int)p & 7) << 3);
                const int g = (int)p >> 3;
                w[0] += g == 0 ? one : 0ull;
                w[1] += g == 1 ? one : 0ull;
                w[2] += g == 2 ? one : 0ull;
                w[3] += g == 3 ? one : 0ull;
            }
            int best = 0, most = 0;
#pragma unroll
            for (int cls = 0; cls < SR_C; ++cls) {
                const int votes = (int)((w[cls >> 3] >> ((cls & 7) << 3)) & 0xffull);
                if (cls != i && votes > most) { most = votes; best = cls; }
            }
            row[0] = best;
        }
        __syncthreads();
        for (int q = tid; q < members; q += SR_VOTE_THREADS) {
            const int v = qlist[sl.out0 + start + q];
            const int best = rows[(size_t)q * k];
            if (v >= 0 && v < sl.size && best != i) {
                pred[sl.out0 + v] = best;
                ++moved;
            }
        }
        __syncthreads();
    }
    if (!stats) return;
    __syncthreads();
    if (moved) atomicAdd(&changed, moved);
    __syncthreads();
    if (tid == 0) {
        int *out = stats + (size_t)s * 4;
        out[0] = steps;
        out[1] = sl.size ? R[SR_NQ] : 0;
        out[2] = changed;
        out[3] = sl.size ? R[SR_BAD] : 0;
    }
}

static long long sr_head_bytes(int b) { return (((long long)b * SR_REC * 4) + 15) & ~15ll; }

} // namespace geot

using namespace geot;

GEOT_EXPORT long long geot_scan_refine_ws_bytes(int b, long long total_out, int n)
{
    if (b < 0 || b > 65535 || n < 1 || n > 63 || total_out < 0 || total_out > (1ll << 40)) return -1;
    return sr_head_bytes(b) + total_out * 4 * (n + 2);     // exact: the entry point takes its vertex capacity from the size
}

GEOT_EXPORT int geot_scan_refine(int b, int c, int n, int n_scans, long long total, const float *points, const long long *offsets,
                                 const long long *scan_ids, const long long *out_offsets, const unsigned *allowed,
                                 long long *pred, int *stats, void *ws, long long ws_bytes, void *stream)
{
    if (b < 0 || b > 65535 || c < 1 || c > GEOT_NTM_MAX_C || n < 1 || n > 63 || n_scans < 1 || total < 1)
        return hipErrorInvalidValue;
    if (!points || !offsets || !scan_ids || !out_offsets || !pred) return hipErrorInvalidValue;
    if (!ws || ((uintptr_t)ws & 15) != 0 || ws_bytes < sr_head_bytes(b)) return hipErrorInvalidValue;
    if (b == 0) return hipSuccess;
    hipStream_t s = (hipStream_t)stream;
    const int k = n + 1;
    // the workspace decides how many vertices the query list and the neighbour table hold; a slot beyond that is skipped
    const long long cap = (ws_bytes - sr_head_bytes(b)) / (4ll * (n + 2));
    unsigned *head = (unsigned *)ws;
    int *qlist = reinterpret_cast<int *>((char *)ws + sr_head_bytes(b));
    int *nbr = qlist + cap;
    hipError_t e = zero_words(head, (long long)b * SR_REC, s);
    if (e != hipSuccess) return e;
    int gx = 4096 / b;
    gx = gx < 1 ? 1 : (gx > 128 ? 128 : gx);
    hipLaunchKernelGGL(sr_census_kernel, dim3(gx, b), dim3(SR_THREADS), 0, s, c, n_scans, total, offsets, scan_ids, out_offsets,
                       cap, pred, head);
    hipLaunchKernelGGL(sr_plan_kernel, dim3(b), dim3(64), 0, s, c, n, n_scans, total, offsets, scan_ids, out_offsets, cap, allowed,
                       head);
    hipLaunchKernelGGL(sr_collect_kernel, dim3(gx, b), dim3(SR_THREADS), 0, s, c, n_scans, total, offsets, scan_ids, out_offsets,
                       cap, pred, head, qlist);
    hipLaunchKernelGGL(sr_search_kernel, dim3(SR_SEARCH_BLOCKS), dim3(SR_THREADS), 0, s, b, k, n_scans, total, points, offsets,
                       scan_ids, out_offsets, cap, head, qlist, nbr);
    hipLaunchKernelGGL(sr_vote_kernel, dim3(b), dim3(SR_VOTE_THREADS), 0, s, c, k, n_scans, total, offsets, scan_ids, out_offsets,
                       cap, head, qlist, nbr, pred, stats);
    return hipGetLastError();
}
