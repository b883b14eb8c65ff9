// Whole-scan labels split into connected pieces, stray pieces relabelled (geot_scan_islands): the connected components of
// equal-label vertices over a caller-given neighbour table, for all batch slots in a fixed number of launches (six; four in
// the components-only form) whatever the slots, their sizes and their labels, without a host synchronisation.  See
// include/geot_hip.h for the rules.  Everything is an integer and no result depends on the order of arrival.
//
//   init     size[v] = 0 and parent[v] = the lowest entry of v's own row below v that shares its label (a member of v's
//            component with a smaller index: a first link that needs no atomic), else v, for every vertex of every usable slot;
//            the per-class records and the stats zeroed: the workspace's contents on entry are irrelevant and no memset node
//            is needed
//   hook     a thread per vertex walks its row of the table and unites the two ends of every edge: lock-free union-find by
//            hooking.  A root is linked under a SMALLER vertex only, by compare-and-swap on the root's own parent word, so
//            parent[x] <= x always, the minimum of a component is never linked, and once every edge has been seen it is the
//            one root of the component.  parent[] is shared between workgroups on different XCDs inside this launch: it is
//            read with relaxed agent-scope atomic loads only (a plain load may be served stale from a per-XCD L2), and after a
//            failed compare-and-swap the walk goes on from the value the compare-and-swap returned.  A stale parent is still
//            an ancestor, so a stale read costs steps and never a wrong union: a link under a vertex that has stopped being a
//            root is still a link into the same tree under a smaller index.  The walks halve the paths behind them (atomic
//            minimum of a non-root's word with its grandparent: a word only ever decreases and always names an ancestor), which
//            is what keeps the trees shallow at 1e5 vertices; the final flattening stays a launch of its own.  Every loop ends
//            by the strict decrease of a vertex index; no thread waits for another
//   flatten  parent[v] = the root of v (the component minimum), comp[v] likewise, one count into size[root]; a root clears
//            its row of the vote table.  Equal roots inside a wave are combined by ballot first (tooth_scores.hip's form: the
//            vertex order of a scan is spatially coherent, so a wave holds a root or two); GEOT_SCAN_ISLANDS_IMPL=basic: one
//            atomic per lane
//   largest  every root: components counted, the packed (size, ~root) maximum of its class taken -- the greatest size, the
//            lowest root among equals
//   vote     whether a component is an island is a function of its root's size, its class and the class's maximum, so it is
//            evaluated where it is needed and never stored.  Every vertex of an island counts the labels of its row's
//            entries that lie in other classes and in no island (at most 32 entries: 8-bit counts in four 64-bit words) and
//            adds them to its root's vote row; roots of islands are counted
//   write    every vertex of an island reads its root's vote row -- most votes, the lowest class among equals -- and takes
//            that label; no vote at all: stranded, the label stays.  Nothing reads a label in this launch but the thread
//            that writes it, so all decisions come from the labels as they arrived
#include "geot_common.h"
#include "geot_hip.h"
#include <cstdlib>

namespace geot {

constexpr int SI_C = GEOT_NTM_MAX_C;
constexpr int SI_MAX_K = 32;
constexpr int SI_THREADS = 256;
constexpr int SI_PEEL = 2;                 // roots per wave and step combined by ballot

typedef unsigned long long si_word;

struct SiSlot {
    long long out0;
    int size;             // 0: the slot is skipped
};
// geot_scan_refine's skip rules, and room for the slot in a workspace of `cap` vertices
__device__ __forceinline__ SiSlot si_slot(int s, int n_scans, long long total, const long long *__restrict__ offsets,
                                          const long long *__restrict__ scan_ids, const long long *__restrict__ out_offsets,
                                          long long cap)
{
    SiSlot r = {0, 0};
    const long long sid = scan_ids[s];
    if (sid < 0 || sid >= n_scans) return r;
    const long long lo = offsets[sid], hi = offsets[sid + 1];
    if (lo < 0 || hi <= lo || hi > total || hi - lo > 0x7fffffffll) return r;
    const long long o = out_offsets[s];
    if (o < 0 || o > cap - (hi - lo)) return r;
    r.out0 = o;
    r.size = (int)(hi - lo);
    return r;
}

// parent[] inside the hook and flatten launches: agent scope, relaxed -- never a plain access
__device__ __forceinline__ unsigned si_load(const unsigned *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void si_store(unsigned *p, unsigned x)
{
    __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// x's ancestor that looked like a root when it was read: every step strictly decreases x
__device__ __forceinline__ unsigned si_find(const unsigned *P, unsigned x)
{
    for (;;) {
        const unsigned p = si_load(P + x);
        if (p >= x) return x;               // (p > x never happens: parent[x] <= x)
        x = p;
    }
}
// The same walk for the hook launch, halving the path behind it: a vertex that is no root is pointed at its grandparent by
// an atomic minimum, so a parent word only ever decreases and always names an ancestor.  Only words of vertices that were
// seen not to be roots are touched (a root's word changes by si_unite's compare-and-swap alone), and the walk itself goes on
// from the values it read, whatever the minimum finds in memory.
__device__ __forceinline__ unsigned si_find_halving(unsigned *P, unsigned x)
{
    for (;;) {
        const unsigned p = si_load(P + x);
        if (p >= x) return x;
        const unsigned g = si_load(P + p);
        if (g < p) __hip_atomic_fetch_min(P + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else return p;
        x = g;
    }
}
// One edge -> the root both ends were seen under.  Every turn of the loop either returns or strictly decreases a: a failed
// compare-and-swap returns a's new parent.
__device__ __forceinline__ unsigned si_unite(unsigned *P, unsigned a, unsigned b)
{
    for (;;) {
        a = si_find_halving(P, a);
        b = si_find_halving(P, b);
        if (a == b) return a;
        if (a < b) { const unsigned t = a; a = b; b = t; }
        unsigned seen = a;
        if (__hip_atomic_compare_exchange_strong(P + a, &seen, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return b;
        if (seen >= a) return b;            // (never: a word that is not its own index holds a smaller one)
        a = seen;
    }
}

__device__ __forceinline__ si_word si_pack(unsigned size, unsigned root) { return ((si_word)size << 32) | (si_word)(~root); }

struct SiRule {
    long long min_size;
    unsigned keep, allowed;
};
// Is the component of class `cls` with root `root` (slot-local) an island?  A pure function of the finished tables.
__device__ __forceinline__ bool si_island(const SiRule &rule, const unsigned *__restrict__ size, const si_word *__restrict__ best,
                                          unsigned root, int cls)
{
    const unsigned sz = size[root];
    if ((long long)sz < rule.min_size) return true;
    if (!((rule.allowed >> cls) & 1u)) return true;
    return ((rule.keep >> cls) & 1u) && best[cls] != si_pack(sz, root);
}

__global__ __launch_bounds__(SI_THREADS) void si_init_kernel(int b, int c, int k, int n_scans, long long total,
                                                             const long long *__restrict__ offsets,
                                                             const long long *__restrict__ scan_ids,
                                                             const long long *__restrict__ out_offsets, long long cap,
                                                             const int *__restrict__ nbr, const long long *__restrict__ pred,
                                                             si_word *__restrict__ best, unsigned *__restrict__ parent,
                                                             unsigned *__restrict__ size, int *__restrict__ stats)
{
    const int s = blockIdx.y, tid = threadIdx.x;
    if (blockIdx.x == 0) {                  // the slot's records, usable or not
        if (tid < c) best[(size_t)s * c + tid] = 0;
        if (stats && tid < 4) stats[(size_t)s * 4 + tid] = 0;
    }
    const SiSlot sl = si_slot(s, n_scans, total, offsets, scan_ids, out_offsets, cap);
    const long long *L = pred + sl.out0;
    for (long long v = (long long)blockIdx.x * SI_THREADS + tid; v < sl.size; v += (long long)gridDim.x * SI_THREADS) {
        // a head start that needs no atomic: the lowest entry of v's own row that shares its label and lies below v is in
        // v's component and smaller, so it may be v's first parent (each thread writes its own word only); else v itself
        unsigned first = (unsigned)v;
        const long long lv = L[v];
        if (lv >= 0 && lv < c) {
            const int *row = nbr + (size_t)(sl.out0 + v) * k;
            for (int e = 0; e < k; ++e) {
                const int u = row[e];
                if (u >= 0 && (unsigned)u < first && L[u] == lv) first = (unsigned)u;
            }
        }
        parent[sl.out0 + v] = first;
        size[sl.out0 + v] = 0;
    }
}

__global__ __launch_bounds__(SI_THREADS) void si_hook_kernel(int c, int k, int n_scans, long long total,
                                                             const long long *__restrict__ offsets,
                                                             const long long *__restrict__ scan_ids,
                                                             const long long *__restrict__ out_offsets, long long cap,
                                                             const int *__restrict__ nbr, const long long *__restrict__ pred,
                                                             unsigned *parent)
{
    const int s = blockIdx.y, tid = threadIdx.x;
    const SiSlot sl = si_slot(s, n_scans, total, offsets, scan_ids, out_offsets, cap);
    unsigned *P = parent + sl.out0;
    const long long *L = pred + sl.out0;
    for (long long v = (long long)blockIdx.x * SI_THREADS + tid; v < sl.size; v += (long long)gridDim.x * SI_THREADS) {
        const long long lv = L[v];
        if (lv < 0 || lv >= c) continue;
        const int *row = nbr + (size_t)(sl.out0 + v) * k;
        // `mine` is an ancestor of v, the last root v was seen under: the next edge starts there, and an entry whose parent
        // word names it is in v's tree already -- one load per entry once a neighbourhood has been joined
        unsigned mine = (unsigned)v;
        for (int e = 0; e < k; ++e) {
            const int u = row[e];
            if (u < 0 || u >= sl.size || u == v) continue;
            if (L[u] != lv) continue;
            const unsigned up = si_load(P + u);
            if (up != mine) mine = si_unite(P, mine, up);
        }
    }
}

template <bool BASIC>
__global__ __launch_bounds__(SI_THREADS) void si_flatten_kernel(int c, int n_scans, long long total,
                                                                const long long *__restrict__ offsets,
                                                                const long long *__restrict__ scan_ids,
                                                                const long long *__restrict__ out_offsets, long long cap,
                                                                const long long *__restrict__ pred, unsigned *parent,
                                                                unsigned *__restrict__ size, unsigned *__restrict__ votes,
                                                                int *__restrict__ comp)
{
    const int s = blockIdx.y, tid = threadIdx.x, lane = lane_id();
    const SiSlot sl = si_slot(s, n_scans, total, offsets, scan_ids, out_offsets, cap);
    unsigned *P = parent + sl.out0;
    // `base` is uniform over the workgroup: every lane of a wave reaches the ballots together
    for (long long base = (long long)blockIdx.x * SI_THREADS; base < sl.size; base += (long long)gridDim.x * SI_THREADS) {
        const long long v = base + tid;
        const bool active = v < sl.size;
        bool pending = false;
        unsigned r = 0;
        if (active) {
            const long long lv = pred[sl.out0 + v];
            pending = lv >= 0 && lv < c;
            // a label outside [0, c) never hooked: it is its own root already
            r = si_find(P, (unsigned)v);
            if (r != (unsigned)v) si_store(P + v, r);
            if (comp) comp[sl.out0 + v] = (int)r;
            if (votes && pending && r == (unsigned)v) {
                unsigned *row = votes + (size_t)(sl.out0 + v) * c;
                for (int j = 0; j < c; ++j) row[j] = 0;
            }
        }
        if constexpr (!BASIC) {
            for (int t = 0; t < SI_PEEL; ++t) {
                const unsigned long long left = __ballot(pending);
                if (left == 0) break;
                const int leader = __ffsll(left) - 1;
                const unsigned lr = (unsigned)__builtin_amdgcn_readlane((int)r, leader);
                const bool same = pending && r == lr;
                const unsigned long long group = __ballot(same);
                if (lane == leader) atomicAdd(&size[sl.out0 + lr], (unsigned)__popcll(group));
                pending = pending && !same;
            }
        }
        if (pending) atomicAdd(&size[sl.out0 + r], 1u);
    }
}

__global__ __launch_bounds__(SI_THREADS) void si_largest_kernel(int c, int n_scans, long long total,
                                                                const long long *__restrict__ offsets,
                                                                const long long *__restrict__ scan_ids,
                                                                const long long *__restrict__ out_offsets, long long cap,
                                                                const long long *__restrict__ pred,
                                                                const unsigned *__restrict__ parent,
                                                                const unsigned *__restrict__ size, si_word *__restrict__ best,
                                                                int *__restrict__ stats)
{
    const int s = blockIdx.y, tid = threadIdx.x, lane = lane_id();
    const SiSlot sl = si_slot(s, n_scans, total, offsets, scan_ids, out_offsets, cap);
    int roots = 0;                           // per wave, kept by lane 0
    for (long long base = (long long)blockIdx.x * SI_THREADS; base < sl.size; base += (long long)gridDim.x * SI_THREADS) {
        const long long v = base + tid;
        bool root = false;
        if (v < sl.size) {
            const long long lv = pred[sl.out0 + v];
            root = lv >= 0 && lv < c && parent[sl.out0 + v] == (unsigned)v;
            if (root) atomicMax(&best[(size_t)s * c + lv], si_pack(size[sl.out0 + v], (unsigned)v));
        }
        roots += __popcll(__ballot(root));
    }
    if (stats && lane == 0 && roots) atomicAdd(&stats[(size_t)s * 4], roots);
}

__global__ __launch_bounds__(SI_THREADS) void si_vote_kernel(int c, int k, int min_size, int n_scans, long long total,
                                                             const long long *__restrict__ offsets,
                                                             const long long *__restrict__ scan_ids,
                                                             const long long *__restrict__ out_offsets, long long cap,
                                                             const int *__restrict__ nbr, const unsigned *__restrict__ keep,
                                                             const unsigned *__restrict__ allowed,
                                                             const long long *__restrict__ pred,
                                                             const unsigned *__restrict__ parent,
                                                             const unsigned *__restrict__ size, const si_word *__restrict__ best,
                                                             unsigned *__restrict__ votes, int *__restrict__ stats)
{
    const int s = blockIdx.y, tid = threadIdx.x, lane = lane_id();
    const SiSlot sl = si_slot(s, n_scans, total, offsets, scan_ids, out_offsets, cap);
    const SiRule rule = {min_size, keep ? keep[s] : 0u, allowed ? allowed[s] : 0xffffffffu};
    const long long *L = pred + sl.out0;
    const unsigned *P = parent + sl.out0, *S = size + sl.out0;
    const si_word *B = best + (size_t)s * c;
    int islands = 0;
    for (long long base = (long long)blockIdx.x * SI_THREADS; base < sl.size; base += (long long)gridDim.x * SI_THREADS) {
        const long long v = base + tid;
        bool counted = false;
        if (v < sl.size) {
            const long long lv = L[v];
            if (lv >= 0 && lv < c) {
                const unsigned r = P[v];
                if (si_island(rule, S, B, r, (int)lv)) {
                    counted = r == (unsigned)v;
                    const int *row = nbr + (size_t)(sl.out0 + v) * k;
                    unsigned long long w[4] = {0ull, 0ull, 0ull, 0ull};
                    for (int e = 0; e < k; ++e) {
                        const int u = row[e];
                        if (u < 0 || u >= sl.size || u == v) continue;
                        const long long lu = L[u];
                        if (lu < 0 || lu >= c || lu == lv) continue;
                        if (si_island(rule, S, B, P[u], (int)lu)) continue;
                        const unsigned long long one = 1ull << (((int)lu & 7) << 3);
                        const int g = (int)lu >> 3;
                        w[0] += g == 0 ? one : 0ull;
                        w[1] += g == 1 ? one : 0ull;
                        w[2] += g == 2 ? one : 0ull;
                        w[3] += g == 3 ? one : 0ull;
                    }
                    if (w[0] | w[1] | w[2] | w[3]) {
                        unsigned *out = votes + (size_t)(sl.out0 + r) * c;
#pragma unroll
                        for (int cls = 0; cls < SI_C; ++cls) {
                            const unsigned n = (unsigned)((w[cls >> 3] >> ((cls & 7) << 3)) & 0xffull);
                            if (n && cls < c) atomicAdd(&out[cls], n);
                        }
                    }
                }
            }
        }
        islands += __popcll(__ballot(counted));
    }
    if (stats && lane == 0 && islands) atomicAdd(&stats[(size_t)s * 4 + 1], islands);
}

__global__ __launch_bounds__(SI_THREADS) void si_write_kernel(int c, int min_size, int n_scans, long long total,
                                                              const long long *__restrict__ offsets,
                                                              const long long *__restrict__ scan_ids,
                                                              const long long *__restrict__ out_offsets, long long cap,
                                                              const unsigned *__restrict__ keep,
                                                              const unsigned *__restrict__ allowed,
                                                              const unsigned *__restrict__ parent,
                                                              const unsigned *__restrict__ size, const si_word *__restrict__ best,
                                                              const unsigned *__restrict__ votes, long long *pred,
                                                              int *__restrict__ stats)
{
    const int s = blockIdx.y, tid = threadIdx.x, lane = lane_id();
    const SiSlot sl = si_slot(s, n_scans, total, offsets, scan_ids, out_offsets, cap);
    const SiRule rule = {min_size, keep ? keep[s] : 0u, allowed ? allowed[s] : 0xffffffffu};
    const unsigned *P = parent + sl.out0, *S = size + sl.out0;
    const si_word *B = best + (size_t)s * c;
    int changed = 0, stranded = 0;
    for (long long base = (long long)blockIdx.x * SI_THREADS; base < sl.size; base += (long long)gridDim.x * SI_THREADS) {
        const long long v = base + tid;
        bool moved = false, stuck = false;
        if (v < sl.size) {
            const long long lv = pred[sl.out0 + v];          // this thread's own vertex: nobody else writes it
            if (lv >= 0 && lv < c) {
                const unsigned r = P[v];
                if (si_island(rule, S, B, r, (int)lv)) {
                    const unsigned *row = votes + (size_t)(sl.out0 + r) * c;
                    unsigned most = 0;
                    int to = -1;
                    for (int cls = 0; cls < c; ++cls) {
                        const unsigned n = row[cls];
                        if (n > most) { most = n; to = cls; }
                    }
                    if (to >= 0) {
                        pred[sl.out0 + v] = to;
                        moved = true;
                    } else {
                        stuck = true;
                    }
                }
            }
        }
        changed += __popcll(__ballot(moved));
        stranded += __popcll(__ballot(stuck));
    }
    if (stats && lane == 0) {
        if (changed) atomicAdd(&stats[(size_t)s * 4 + 2], changed);
        if (stranded) atomicAdd(&stats[(size_t)s * 4 + 3], stranded);
    }
}

static long long si_head_bytes(int b, int c) { return (((long long)b * c * 8) + 15) & ~15ll; }

} // namespace geot

using namespace geot;

GEOT_EXPORT long long geot_scan_islands_ws_bytes(int b, long long total_out, int c)
{
    if (b < 0 || b > 65535 || c < 1 || c > GEOT_NTM_MAX_C || total_out < 0 || total_out > (1ll << 40)) return -1;
    // exact: the entry point takes its vertex capacity from the size.  Per vertex a parent, a size and c vote counts
    return si_head_bytes(b, c) + total_out * 4 * (c + 2);
}

GEOT_EXPORT int geot_scan_islands(int b, int c, int k, int min_size, int n_scans, long long total, const long long *offsets,
                                  const long long *scan_ids, const long long *out_offsets, const int *nbr, const unsigned *keep,
                                  const unsigned *allowed, long long *pred, int *comp, int *stats, void *ws, long long ws_bytes,
                                  void *stream)
{
    if (b < 0 || b > 65535 || c < 1 || c > GEOT_NTM_MAX_C || k < 1 || k > SI_MAX_K || min_size < 0 || n_scans < 1 || total < 1)
        return hipErrorInvalidValue;
    if (!offsets || !scan_ids || !out_offsets || !nbr || !pred) return hipErrorInvalidValue;
    if (!ws || ((uintptr_t)ws & 15) != 0 || ws_bytes < si_head_bytes(b, c)) return hipErrorInvalidValue;
    if (b == 0) return hipSuccess;
    hipStream_t s = (hipStream_t)stream;
    const char *e = getenv("GEOT_SCAN_ISLANDS_IMPL");       // read at every call, like the other A/B switches
    const bool basic = e && e[0] == 'b';
    // the workspace decides how many vertices the tables hold; a slot beyond that is skipped
    const long long cap = (ws_bytes - si_head_bytes(b, c)) / (4ll * (c + 2));
    si_word *best = (si_word *)ws;
    unsigned *parent = reinterpret_cast<unsigned *>((char *)ws + si_head_bytes(b, c));
    unsigned *size = parent + cap;
    unsigned *votes = size + cap;
    // nothing can be an island: the components-only form, pred is not written
    const bool clean = min_size > 1 || keep || allowed;
    // a thread per vertex where the slots are even (the walks are latency-bound: the more waves the better), a grid-stride
    // loop where they are not; at most ~2^20 threads per launch row
    long long per = cap / ((long long)b * SI_THREADS) + 1;
    const long long most = 4096 / b < 1 ? 1 : 4096 / b;
    const int gx = (int)(per > most ? most : per);
    const dim3 grid(gx, b), block(SI_THREADS);
    hipLaunchKernelGGL(si_init_kernel, grid, block, 0, s, b, c, k, n_scans, total, offsets, scan_ids, out_offsets, cap, nbr, pred, best,
                       parent, size, stats);
    hipLaunchKernelGGL(si_hook_kernel, grid, block, 0, s, c, k, n_scans, total, offsets, scan_ids, out_offsets, cap, nbr, pred,
                       parent);
    if (basic)
        hipLaunchKernelGGL((si_flatten_kernel<true>), grid, block, 0, s, c, n_scans, total, offsets, scan_ids, out_offsets, cap, pred,
                           parent, size, clean ? votes : nullptr, comp);
    else
        hipLaunchKernelGGL((si_flatten_kernel<false>), grid, block, 0, s, c, n_scans, total, offsets, scan_ids, out_offsets, cap, pred,
                           parent, size, clean ? votes : nullptr, comp);
    hipLaunchKernelGGL(si_largest_kernel, grid, block, 0, s, c, n_scans, total, offsets, scan_ids, out_offsets, cap, pred, parent,
                       size, best, stats);
    if (clean) {
        hipLaunchKernelGGL(si_vote_kernel, grid, block, 0, s, c, k, min_size, n_scans, total, offsets, scan_ids, out_offsets, cap, nbr,
                           keep, allowed, pred, parent, size, best, votes, stats);
        hipLaunchKernelGGL(si_write_kernel, grid, block, 0, s, c, min_size, n_scans, total, offsets, scan_ids, out_offsets, cap, keep,
                           allowed, parent, size, best, votes, pred, stats);
    }
    return hipGetLastError();
}
