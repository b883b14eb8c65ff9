// One-ring neighbour tables of whole-scan triangle meshes (geot_mesh_neighbours): per vertex of every batch slot the distinct
// vertices it shares a face with, ascending, in the (total_out, k) layout geot_scan_islands reads -- a fixed number of launches
// (seven) whatever the slots, their sizes and their faces, without a host synchronisation and without a spatial search.  See
// include/geot_hip.h for the rules.  Everything is an integer and no result depends on the order of arrival.
//
//   init     the raw degree of every vertex row of the workspace and the stats zeroed: the workspace's contents on entry are
//            irrelevant and no memset node is needed
//   count    a thread per face of every usable slot: a face whose three indices all lie in [0, M_s) adds 2 to the raw degree
//            of each of its corners (an integer atomic); any other face is counted as ignored and none of its indices is
//            ever used as an address.  Usable and ignored faces are combined by ballot before the stats atomic
//   scan     geot_common.h's exclusive scan of the raw degrees over all vertex rows (block-local scan, scan of the block sums,
//            add): three launches, no workgroup waits for another.  The add clears the fill cursors on its way
//   fill     a thread per face again: each corner reserves two entries of its raw row by an integer atomic on its cursor and
//            writes the face's two other corners there.  The ORDER of a raw row depends on the schedule; nothing read from
//            it does
//   tidy     per vertex the k lowest distinct values of its raw row other than the vertex itself, by repeated "smallest
//            value greater than the last one written": no sort, no private array.  A raw row of at most
//            GEOT_MESH_NEIGHBOURS_LANE_ROW entries is walked by one lane; a longer one by the whole wave, 64 entries a step,
//            the minimum taken across the lanes (the lanes that hold long rows are found by ballot and served one after
//            another: at most 64 turns).  One more round than k tells whether the vertex is truncated.  The rest of the row
//            is -1.  Truncated vertices and the longest row are combined inside the wave before the stats atomics;
//            GEOT_MESH_NEIGHBOURS_IMPL=basic: a lane per vertex whatever the row's length, one atomic per lane
// Every loop is bounded by a count known at its start.  A raw entry is only ever a VALUE (a vertex index of a usable face); the
// positions in the raw buffer come from the scan and are checked against the buffer's size before every access, so that even a
// caller who breaks the contract (overlapping slots) gets wrong rows and never an access outside the workspace.
#include "geot_common.h"
#include "geot_hip.h"
#include <climits>
#include <cstdlib>

namespace geot {

constexpr int MN_MAX_K = 32;
constexpr int MN_THREADS = 256;
constexpr int MN_LANE_ROW = GEOT_MESH_NEIGHBOURS_LANE_ROW;
constexpr long long MN_MAX_OUT = 1ll << 30;                         // vertex rows of one call (the scan counts in int)
constexpr long long MN_MAX_FACES = 0x7fffffffll / 6;                // 6 raw entries per face, addressed in int

static long long mn_raw_bytes(long long batch_faces) { return (batch_faces * 24 + 15) & ~15ll; }
// The workspace behind the raw entries, in units of 16 bytes: one per vertex row (its row start and its cursor: 8 bytes used),
// one per started SCAN_CHUNK rows (the chunk's block sum) and one for the grand total behind the last row start.  A unit per
// row and not half of one, so that the size names total_out EXACTLY: the entry point is not told total_out, takes its vertex
// capacity from ws_bytes, and a slot is refused by that capacity before a row of nbr beyond total_out could be written.
static long long mn_units(long long total_out) { return total_out + total_out / SCAN_CHUNK + 2; }
static long long mn_capacity(long long units)
{
    const long long n = units - 2;            // = cap + cap / SCAN_CHUNK
    return n - n / (SCAN_CHUNK + 1);
}

struct MnSlot {
    long long out0, face0;
    int size;             // 0: the slot is skipped
    int faces;
};
// geot_scan_islands' skip rules (room for the slot among `cap` vertex rows), and the two rules on the faces: the set's face
// range of the scan is 0 <= lo <= hi <= total_faces, and the slot's pair of face_out_offsets names a range of that length
// inside [0, batch_faces] -- so the usable slots' raw rows fit the 6 * batch_faces entries of the workspace
__device__ __forceinline__ MnSlot mn_slot(int s, int n_scans, long long total, long long total_faces,
                                          const long long *__restrict__ offsets, const long long *__restrict__ face_offsets,
                                          const long long *__restrict__ scan_ids, const long long *__restrict__ out_offsets,
                                          const long long *__restrict__ face_out_offsets, long long batch_faces, long long cap)
{
    MnSlot r = {0, 0, 0, 0};
    const long long sid = scan_ids[s];
    if (sid < 0 || sid >= n_scans) return r;
    const long long lo = offsets[sid], hi = offsets[sid + 1];
    if (lo < 0 || hi <= lo || hi > total || hi - lo > 0x7fffffffll) return r;
    const long long o = out_offsets[s];
    if (o < 0 || o > cap - (hi - lo)) return r;
    const long long flo = face_offsets[sid], fhi = face_offsets[sid + 1];
    if (flo < 0 || fhi < flo || fhi > total_faces) return r;
    const long long a = face_out_offsets[s], z = face_out_offsets[s + 1];
    if (a < 0 || z < a || z > batch_faces || z - a != fhi - flo) return r;
    r.out0 = o;
    r.face0 = flo;
    r.size = (int)(hi - lo);
    r.faces = (int)(fhi - flo);           // <= batch_faces <= MN_MAX_FACES
    return r;
}

__global__ __launch_bounds__(MN_THREADS) void mn_init_kernel(int b, long long rows, int *__restrict__ start, int *__restrict__ stats)
{
    const long long i0 = (long long)blockIdx.x * MN_THREADS + threadIdx.x, step = (long long)gridDim.x * MN_THREADS;
    if (stats)
        for (long long i = i0; i < 4ll * b; i += step) stats[i] = 0;      // every slot's record, usable or not
    for (long long i = i0; i < rows; i += step) start[i] = 0;
}

// FILL false: the raw degrees (`start` before the scan) and the face counts of the stats; true: the raw rows
template <bool FILL>
__global__ __launch_bounds__(MN_THREADS) void mn_faces_kernel(int n_scans, long long total, long long total_faces,
                                                              const int *__restrict__ faces,
                                                              const long long *__restrict__ offsets,
                                                              const long long *__restrict__ face_offsets,
                                                              const long long *__restrict__ scan_ids,
                                                              const long long *__restrict__ out_offsets,
                                                              const long long *__restrict__ face_out_offsets,
                                                              long long batch_faces, long long cap, int *start, int *cursor,
                                                              int *__restrict__ raw, int *__restrict__ stats)
{
    const int s = blockIdx.y, tid = threadIdx.x, lane = lane_id();
    const MnSlot sl = mn_slot(s, n_scans, total, total_faces, offsets, face_offsets, scan_ids, out_offsets, face_out_offsets,
                              batch_faces, cap);
    const long long raw_cap = 6 * batch_faces;
    int used = 0, ignored = 0;               // per wave, the same in every lane
    // `base` is uniform over the workgroup: every lane of a wave reaches the ballots together
    for (long long base = (long long)blockIdx.x * MN_THREADS; base < sl.faces; base += (long long)gridDim.x * MN_THREADS) {
        const long long f = base + tid;
        const bool in = f < sl.faces;
        bool ok = false;
        if (in) {
            const int *c = faces + 3 * (sl.face0 + f);
            const int c0 = c[0], c1 = c[1], c2 = c[2];
            // bounds first: an index outside the scan is never an address
            ok = (unsigned)c0 < (unsigned)sl.size && (unsigned)c1 < (unsigned)sl.size && (unsigned)c2 < (unsigned)sl.size;
            if (ok) {
                if constexpr (!FILL) {
                    atomicAdd(&start[sl.out0 + c0], 2);
                    atomicAdd(&start[sl.out0 + c1], 2);
                    atomicAdd(&start[sl.out0 + c2], 2);
                } else {
                    const int corner[3] = {c0, c1, c2}, one[3] = {c1, c2, c0}, two[3] = {c2, c0, c1};
#pragma unroll
                    for (int e = 0; e < 3; ++e) {
                        const long long p = (long long)start[sl.out0 + corner[e]] + atomicAdd(&cursor[sl.out0 + corner[e]], 2);
                        if (p >= 0 && p + 2 <= raw_cap) {
                            raw[p] = one[e];
                            raw[p + 1] = two[e];
                        }
                    }
                }
            }
        }
        if constexpr (!FILL) {
            used += __popcll(__ballot(ok));
            ignored += __popcll(__ballot(in && !ok));
        }
    }
    if constexpr (!FILL) {
        if (stats && lane == 0) {
            if (used) atomicAdd(&stats[(size_t)s * 4], used);
            if (ignored) atomicAdd(&stats[(size_t)s * 4 + 1], ignored);
        }
    }
}

template <bool BASIC>
__global__ __launch_bounds__(MN_THREADS) void mn_tidy_kernel(int k, int n_scans, long long total, long long total_faces,
                                                             const long long *__restrict__ offsets,
                                                             const long long *__restrict__ face_offsets,
                                                             const long long *__restrict__ scan_ids,
                                                             const long long *__restrict__ out_offsets,
                                                             const long long *__restrict__ face_out_offsets,
                                                             long long batch_faces, long long cap, const int *__restrict__ start,
                                                             const int *__restrict__ raw, int *__restrict__ nbr,
                                                             int *__restrict__ stats)
{
    const int s = blockIdx.y, tid = threadIdx.x, lane = lane_id();
    const MnSlot sl = mn_slot(s, n_scans, total, total_faces, offsets, face_offsets, scan_ids, out_offsets, face_out_offsets,
                              batch_faces, cap);
    const long long raw_cap = 6 * batch_faces;
    int truncated = 0, longest = 0;          // truncated: per wave; longest: per lane
    for (long long base = (long long)blockIdx.x * MN_THREADS; base < sl.size; base += (long long)gridDim.x * MN_THREADS) {
        const int v = (int)(base + tid);     // (base + tid < 2^31: sl.size is an int and the overshoot is below a workgroup)
        const bool active = base + tid < sl.size;
        int lo = 0, hi = 0;
        if (active) {
            // the raw row, clamped into the raw buffer whatever the scan holds
            const long long a = start[sl.out0 + v], z = start[sl.out0 + v + 1];
            lo = (int)(a < 0 ? 0 : a > raw_cap ? raw_cap : a);
            hi = (int)(z < lo ? lo : z > raw_cap ? raw_cap : z);
        }
        const bool wide = !BASIC && hi - lo > MN_LANE_ROW;
        int len = 0;
        bool cut = false;
        if (active && !wide) {
            int *row = nbr + (size_t)(sl.out0 + v) * k;
            int last = -1;
            for (int j = 0; j <= k; ++j) {               // k rounds write, one more tells whether anything is left
                int m = INT_MAX;
                for (int e = lo; e < hi; ++e) {
                    const int x = raw[e];
                    if (x > last && x != v && x < m) m = x;
                }
                if (m == INT_MAX) break;
                if (j == k) { cut = true; break; }
                row[j] = m;
                last = m;
                len = j + 1;
            }
            for (int j = len; j < k; ++j) row[j] = -1;
        }
        if constexpr (!BASIC) {
            // the lanes with long rows, one after another, each served by the whole wave: one bit leaves `todo` per turn
            unsigned long long todo = __ballot(wide);
            while (todo) {
                const int src = __ffsll(todo) - 1;
                todo &= todo - 1;
                const int wv = __builtin_amdgcn_readlane(v, src);
                const int wlo = __builtin_amdgcn_readlane(lo, src), whi = __builtin_amdgcn_readlane(hi, src);
                int *row = nbr + (size_t)(sl.out0 + wv) * k;
                int last = -1, n = 0;
                bool more = false;
                for (int j = 0; j <= k; ++j) {
                    int m = INT_MAX;
                    for (int e = wlo + lane; e < whi; e += GEOT_WAVE) {
                        const int x = raw[e];
                        if (x > last && x != wv && x < m) m = x;
                    }
                    m = (int)wave_min_u32((unsigned)m);   // (no candidate is negative)
                    if (m == INT_MAX) break;
                    if (j == k) { more = true; break; }
                    if (lane == 0) row[j] = m;
                    last = m;
                    n = j + 1;
                }
                for (int j = n + lane; j < k; j += GEOT_WAVE) row[j] = -1;
                if (lane == src) { len = n; cut = more; }
            }
            truncated += __popcll(__ballot(cut));
            longest = max(longest, len);
        } else if (stats) {
            if (cut) atomicAdd(&stats[(size_t)s * 4 + 2], 1);
            if (len) atomicMax(&stats[(size_t)s * 4 + 3], len);
        }
    }
    if constexpr (!BASIC) {
        if (stats) {
            longest = wave_max_i32(longest);
            if (lane == 0) {
                if (truncated) atomicAdd(&stats[(size_t)s * 4 + 2], truncated);
                if (longest) atomicMax(&stats[(size_t)s * 4 + 3], longest);
            }
        }
    }
}

} // namespace geot

using namespace geot;

GEOT_EXPORT long long geot_mesh_neighbours_ws_bytes(int b, long long total_out, long long batch_faces)
{
    if (b < 0 || b > 65535 || total_out < 0 || total_out > MN_MAX_OUT || batch_faces < 0 || batch_faces > MN_MAX_FACES) return -1;
    // exact: the entry point takes its vertex capacity from the size
    return mn_raw_bytes(batch_faces) + 16 * mn_units(total_out);
}

GEOT_EXPORT int geot_mesh_neighbours(int b, int k, int n_scans, long long total, long long total_faces, const int *faces,
                                     const long long *offsets, const long long *face_offsets, const long long *scan_ids,
                                     const long long *out_offsets, const long long *face_out_offsets, long long batch_faces, int *nbr,
                                     int *stats, void *ws, long long ws_bytes, void *stream)
{
    if (b < 0 || b > 65535 || k < 1 || k > MN_MAX_K || n_scans < 1 || total < 1 || total_faces < 0 || batch_faces < 0 ||
        batch_faces > MN_MAX_FACES)
        return hipErrorInvalidValue;
    if (!offsets || !face_offsets || !scan_ids || !out_offsets || !face_out_offsets || !nbr || (!faces && total_faces != 0))
        return hipErrorInvalidValue;
    if (!ws || ((uintptr_t)ws & 15) != 0 || ws_bytes < mn_raw_bytes(batch_faces) + 16 * mn_units(0)) return hipErrorInvalidValue;
    if (b == 0) return hipSuccess;
    hipStream_t s = (hipStream_t)stream;
    const char *e = getenv("GEOT_MESH_NEIGHBOURS_IMPL");    // read at every call, like the other A/B switches
    const bool basic = e && e[0] == 'b';
    // the workspace decides how many vertex rows the tables hold; a slot beyond that is skipped
    long long cap = mn_capacity((ws_bytes - mn_raw_bytes(batch_faces)) / 16);
    if (cap > MN_MAX_OUT) cap = MN_MAX_OUT;
    const long long rows = cap + 1;           // the scan writes the grand total behind the last row start
    int *raw = (int *)ws;
    int *bsum = reinterpret_cast<int *>((char *)ws + mn_raw_bytes(batch_faces));
    int *start = reinterpret_cast<int *>((char *)bsum + 16ll * scan_blocks(cap));
    int *cursor = start + ((rows + 3) & ~3ll);
    // a thread per vertex or face where the slots are even, a grid-stride loop where they are not (scan_islands.hip's sizing)
    const long long most = 4096 / b < 1 ? 1 : 4096 / b;
    const long long per_v = cap / ((long long)b * MN_THREADS) + 1, per_f = batch_faces / ((long long)b * MN_THREADS) + 1;
    const dim3 block(MN_THREADS), grid_v((int)(per_v > most ? most : per_v), b), grid_f((int)(per_f > most ? most : per_f), b);
    const long long blocks = (rows + MN_THREADS - 1) / MN_THREADS;
    hipLaunchKernelGGL(mn_init_kernel, dim3((int)(blocks > 4096 ? 4096 : blocks)), block, 0, s, b, rows, start, stats);
    hipLaunchKernelGGL((mn_faces_kernel<false>), grid_f, block, 0, s, n_scans, total, total_faces, faces, offsets, face_offsets,
                       scan_ids, out_offsets, face_out_offsets, batch_faces, cap, start, cursor, raw, stats);
    exclusive_scan_i32((int)cap, start, bsum, cursor, s);
    hipLaunchKernelGGL((mn_faces_kernel<true>), grid_f, block, 0, s, n_scans, total, total_faces, faces, offsets, face_offsets,
                       scan_ids, out_offsets, face_out_offsets, batch_faces, cap, start, cursor, raw, stats);
    if (basic)
        hipLaunchKernelGGL((mn_tidy_kernel<true>), grid_v, block, 0, s, k, n_scans, total, total_faces, offsets, face_offsets, scan_ids,
                           out_offsets, face_out_offsets, batch_faces, cap, start, raw, nbr, stats);
    else
        hipLaunchKernelGGL((mn_tidy_kernel<false>), grid_v, block, 0, s, k, n_scans, total, total_faces, offsets, face_offsets, scan_ids,
                           out_offsets, face_out_offsets, batch_faces, cap, start, raw, nbr, stats);
    return hipGetLastError();
}
