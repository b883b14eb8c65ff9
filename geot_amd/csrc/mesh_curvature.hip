// Per-vertex discrete Gaussian curvature of whole-scan triangle meshes (ABI 37): geot_mesh_angle_defects (faces -> one 64-bit
// integer angle defect per vertex), geot_scan_ball_sum (the sum of a 64-bit per-vertex value over the closed ball around every
// vertex of ONE scan, over knn_grid.h's uniform grid) and geot_curvature_sample (gather + per-scan min-max of |curvature|).
// See include/geot_hip.h for the rules.  Kernels only: no memset, no host synchronisation, no float atomic, nothing read back.
//
//   defects  init     the accumulators (defect_q itself) and the valence counters of the usable slots, and the stats, zeroed
//            faces    a thread per face: the three corner angles in un-contracted fp32, each atan2(|e1 x e2|, e1 . e2) from
//                     (corner, the two others) -- swapping the two others flips the sign of every cross component and commutes
//                     the dot's products, so rotating or flipping a face changes no bit; each angle quantised to
//                     llrint(angle * 2^32) and added to its corner's word by a 64-bit INTEGER atomic: the sum does not depend
//                     on the schedule.  The face classes are combined by ballot before the stats atomics
//            finish   defect_q[v] = Q2PI - sum; the vertices in no usable face are counted by ballot
//   ball sum the grid build of geot_ball_query_ws (kg_build, cell edge >= 1.0001 radius: the 3 x 3 x 3 block around a vertex's
//            cell holds its closed ball), a two-word init of the range, and the query kernel: the queries are taken in RECORD
//            order (neighbours in space are neighbours in the stream): a lane per query -- the lanes of a wave mostly sit in one
//            cell and walk the same block, so their candidate loads coincide -- or (GEOT_BALL_SUM_IMPL=basic) a wave per query
//            with a lane per candidate and a 64-bit integer wave sum, which measured 1.5 times slower on scan-sized meshes
//            (profiles/mesh_curvature_timing.txt).  Integer sums: the same bits.  |out|'s range goes through the
//            order-preserving key into one atomicMin / atomicMax pair per wave
//   sample   a workgroup per slot: out = (|cur[sel]| - min) / (max - min), the slot's flag from one __syncthreads_or
//
// mc_atan2 is written with +, -, *, correctly rounded / (and the callers' sqrtf) alone, so that a numpy float32 restatement
// (tests/_curvature_ref.py) gives its bits.  y >= 0.  t = min / max in [0, 1]; past tan(pi / 8) the second reduction
// t' = (t - 1) / (t + 1), atan t = pi / 4 + atan t', leaves |t'| <= tan(pi / 8) = 0.41421357; there the Taylor series
// t - t^3 / 3 + ... - t^19 / 19 (ten terms) is cut before t^21 / 21 <= 0.41421357^21 / 21 < 4.5e-10 -- alternating with falling
// terms, so that is the truncation error.  pi / 4, pi / 2 and pi enter as a float and the float of what it misses, the small
// part first.  Non-finite arguments and (0, 0) give 0.
#include "geot_common.h"
#include "geot_hip.h"
#include "knn_grid.h"
#include <climits>
#include <cmath>
#include <cstdlib>

namespace geot {

constexpr int MC_THREADS = 256;
constexpr int MC_SAMPLE_THREADS = 1024;
constexpr long long MC_MAX_OUT = 1ll << 30;
constexpr long long MC_MAX_FACES = 0x7fffffffll / 6;               // geot_mesh_neighbours' bound: the two calls take the same sets
constexpr int MC_MAX_SCAN = GEOT_CURVATURE_MAX_SCAN;                // vertices of one scan

constexpr float MC_PI_HI = (float)M_PI, MC_PI_LO = (float)(M_PI - (double)(float)M_PI);
constexpr float MC_PIO2_HI = 0.5f * MC_PI_HI, MC_PIO2_LO = 0.5f * MC_PI_LO;          // (powers of two: exact)
constexpr float MC_PIO4_HI = 0.25f * MC_PI_HI, MC_PIO4_LO = 0.25f * MC_PI_LO;
constexpr float MC_TAN_PIO8 = 0.41421357f;

__device__ __forceinline__ float mc_atan2(float y, float x)
{
    const float ax = x < 0.f ? -x : x;
    if (!(y < INFINITY) || !(ax < INFINITY)) return 0.f;            // NaN, overflow
    const bool steep = y > ax;
    const float lo = steep ? ax : y, hi = steep ? y : ax;
    if (hi == 0.f) return 0.f;
    float t = lo / hi;
    const bool upper = t > MC_TAN_PIO8;
    if (upper) t = (t - 1.f) / (t + 1.f);
    const float w = t * t;
    float p = -(float)(1.0 / 19.0);
    p = p * w + (float)(1.0 / 17.0);
    p = p * w - (float)(1.0 / 15.0);
    p = p * w + (float)(1.0 / 13.0);
    p = p * w - (float)(1.0 / 11.0);
    p = p * w + (float)(1.0 / 9.0);
    p = p * w - (float)(1.0 / 7.0);
    p = p * w + (float)(1.0 / 5.0);
    p = p * w - (float)(1.0 / 3.0);
    float r = t + (t * w) * p;
    if (upper) r = MC_PIO4_HI + (MC_PIO4_LO + r);
    if (steep) r = MC_PIO2_HI - (r - MC_PIO2_LO);
    if (x < 0.f) r = MC_PI_HI - (r - MC_PI_LO);
    return r;
}

// the angle at corner a of the face (a, b, c), quantised
__device__ __forceinline__ long long mc_corner_q(const float *a, const float *b, const float *c)
{
    const float ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const float vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const float cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    const float n = sqrtf((cx * cx + cy * cy) + cz * cz);
    const float d = (ux * vx + uy * vy) + uz * vz;
    return llrint((double)mc_atan2(n, d) * 4294967296.0);
}

struct McSlot {
    long long out0, face0, vert0;
    int size;             // 0: the slot is skipped
    int faces;
};
// geot_mesh_neighbours' skip rules with total_out told, and a scan of more than MC_MAX_SCAN vertices skipped too
__device__ __forceinline__ McSlot mc_slot(int s, int n_scans, long long total, long long total_faces,
                                          const long long *__restrict__ offsets, const long long *__restrict__ face_offsets,
                                          const long long *__restrict__ scan_ids, const long long *__restrict__ out_offsets,
                                          const long long *__restrict__ face_out_offsets, long long batch_faces, long long total_out)
{
    McSlot r = {0, 0, 0, 0, 0};
    const long long sid = scan_ids[s];
    if (sid < 0 || sid >= n_scans) return r;
    const long long lo = offsets[sid], hi = offsets[sid + 1];
    if (lo < 0 || hi <= lo || hi > total || hi - lo > MC_MAX_SCAN) return r;
    const long long o = out_offsets[s];
    if (o < 0 || o > total_out - (hi - lo)) return r;
    const long long flo = face_offsets[sid], fhi = face_offsets[sid + 1];
    if (flo < 0 || fhi < flo || fhi > total_faces) return r;
    const long long a = face_out_offsets[s], z = face_out_offsets[s + 1];
    if (a < 0 || z < a || z > batch_faces || z - a != fhi - flo) return r;
    r.out0 = o;
    r.face0 = flo;
    r.vert0 = lo;
    r.size = (int)(hi - lo);
    r.faces = (int)(fhi - flo);           // <= batch_faces <= MC_MAX_FACES
    return r;
}

#define MC_SLOT_PARAMS                                                                                                           \
    int n_scans, long long total, long long total_faces, const long long *__restrict__ offsets,                                  \
        const long long *__restrict__ face_offsets, const long long *__restrict__ scan_ids,                                      \
        const long long *__restrict__ out_offsets, const long long *__restrict__ face_out_offsets, long long batch_faces,        \
        long long total_out
#define MC_SLOT_ARGS n_scans, total, total_faces, offsets, face_offsets, scan_ids, out_offsets, face_out_offsets, batch_faces, total_out

// FINISH false: the usable slots' accumulators and valence counters and every slot's stats zeroed; true: defect = Q2PI - sum
template <bool FINISH>
__global__ __launch_bounds__(MC_THREADS) void mc_vertex_kernel(MC_SLOT_PARAMS, long long q2pi, long long *__restrict__ defect_q,
                                                               int *__restrict__ valence, int *__restrict__ stats)
{
    const int s = blockIdx.y, tid = threadIdx.x, lane = lane_id();
    const McSlot sl = mc_slot(s, MC_SLOT_ARGS);
    if constexpr (!FINISH) {
        if (stats && blockIdx.x == 0 && tid < 4) stats[(size_t)s * 4 + tid] = 0;      // a skipped slot's record too
    }
    int lonely = 0;                          // per wave, the same in every lane
    for (long long base = (long long)blockIdx.x * MC_THREADS; base < sl.size; base += (long long)gridDim.x * MC_THREADS) {
        const long long v = base + tid;
        const bool in = v < sl.size;
        if constexpr (!FINISH) {
            if (in) {
                defect_q[sl.out0 + v] = 0;
                valence[sl.out0 + v] = 0;
            }
        } else {
            if (in) defect_q[sl.out0 + v] = q2pi - defect_q[sl.out0 + v];
            lonely += __popcll(__ballot(in && valence[in ? sl.out0 + v : 0] == 0));
        }
    }
    if constexpr (FINISH) {
        if (stats && lane == 0 && lonely) atomicAdd(&stats[(size_t)s * 4 + 3], lonely);
    }
}

__global__ __launch_bounds__(MC_THREADS) void mc_faces_kernel(MC_SLOT_PARAMS, const float *__restrict__ points,
                                                              const int *__restrict__ faces, long long *defect_q, int *valence,
                                                              int *__restrict__ stats)
{
    const int s = blockIdx.y, tid = threadIdx.x, lane = lane_id();
    const McSlot sl = mc_slot(s, MC_SLOT_ARGS);
    int used = 0, ignored = 0, flat = 0;     // per wave, the same in every lane
    // `base` is uniform over the workgroup: every lane of a wave reaches the ballots together
    for (long long base = (long long)blockIdx.x * MC_THREADS; base < sl.faces; base += (long long)gridDim.x * MC_THREADS) {
        const long long f = base + tid;
        const bool in = f < sl.faces;
        bool ok = false, degenerate = false;
        if (in) {
            const int *c = faces + 3 * (sl.face0 + f);
            const int c0 = c[0], c1 = c[1], c2 = c[2];
            // bounds first: an index outside the scan is never an address
            ok = (unsigned)c0 < (unsigned)sl.size && (unsigned)c1 < (unsigned)sl.size && (unsigned)c2 < (unsigned)sl.size &&
                 c0 != c1 && c1 != c2 && c0 != c2;
            if (ok) {
                float p[3][3];
                const int corner[3] = {c0, c1, c2};
                bool finite = true;
#pragma unroll
                for (int e = 0; e < 3; ++e)
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        p[e][a] = points[3 * (sl.vert0 + corner[e]) + a];
                        finite = finite && fabsf(p[e][a]) < INFINITY;
                    }
                const bool same01 = p[0][0] == p[1][0] && p[0][1] == p[1][1] && p[0][2] == p[1][2];
                const bool same12 = p[1][0] == p[2][0] && p[1][1] == p[2][1] && p[1][2] == p[2][2];
                const bool same02 = p[0][0] == p[2][0] && p[0][1] == p[2][1] && p[0][2] == p[2][2];
                degenerate = !finite || same01 || same12 || same02;
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    if (!degenerate) {
                        const long long q = mc_corner_q(p[e], p[(e + 1) % 3], p[(e + 2) % 3]);
                        atomicAdd(reinterpret_cast<unsigned long long *>(&defect_q[sl.out0 + corner[e]]), (unsigned long long)q);
                    }
                    atomicAdd(&valence[sl.out0 + corner[e]], 1);
                }
            }
        }
        used += __popcll(__ballot(ok));
        ignored += __popcll(__ballot(in && !ok));
        flat += __popcll(__ballot(degenerate));
    }
    if (stats && lane == 0) {
        if (used) atomicAdd(&stats[(size_t)s * 4], used);
        if (ignored) atomicAdd(&stats[(size_t)s * 4 + 1], ignored);
        if (flat) atomicAdd(&stats[(size_t)s * 4 + 2], flat);
    }
}

// ---- ball sum ---------------------------------------------------------------------------------------------------------------------
__global__ void bs_init_kernel(uint32_t *__restrict__ absminmax)
{
    if (threadIdx.x == 0) absminmax[0] = 0xFFFFFFFFu;
    if (threadIdx.x == 1) absminmax[1] = 0u;
}

struct BsRows {            // lane < 9: the records of row (y, z) of the 3 x 3 x 3 block, contiguous over its x cells
    int rs, re;
};
__device__ __forceinline__ BsRows bs_rows(const KgGrid &g, const int *__restrict__ start, float qx, float qy, float qz, int row)
{
    BsRows r = {0, 0};
    const int cx = kg_cell1(qx, g.lo[0], g.inv_h, g.dim[0]);
    const int cy = kg_cell1(qy, g.lo[1], g.inv_h, g.dim[1]);
    const int cz = kg_cell1(qz, g.lo[2], g.inv_h, g.dim[2]);
    const int y = cy + row % 3 - 1, z = cz + row / 3 - 1;
    if (row < 9 && y >= 0 && y < g.dim[1] && z >= 0 && z < g.dim[2]) {
        const int base = (z * g.dim[1] + y) * g.dim[0];
        r.rs = start[base + max(cx - 1, 0)];
        r.re = start[base + min(cx + 1, g.dim[0] - 1) + 1];
    }
    return r;
}

__device__ __forceinline__ unsigned long long bs_member(const float4 &q, const float4 &p, float r2, int m,
                                                        const long long *__restrict__ value)
{
    const int id = __float_as_int(p.w);
    if (sqdist3(q.x, q.y, q.z, p.x, p.y, p.z) <= r2 && (unsigned)id < (unsigned)m) return (unsigned long long)value[id];
    return 0ull;
}

__device__ __forceinline__ uint32_t bs_write(unsigned long long sum, int id, int m, float *__restrict__ out)
{
    const float o = (float)((double)(long long)sum * (1.0 / 4294967296.0));
    if ((unsigned)id < (unsigned)m) out[id] = o;
    return f2ord(fabsf(o));
}

template <bool WAVE>
__global__ __launch_bounds__(MC_THREADS) void bs_kernel(int m, float radius, float min_h, const uint32_t *__restrict__ ws,
                                                        size_t off_rec, const long long *__restrict__ value,
                                                        float *__restrict__ out, uint32_t *absminmax)
{
    const int lane = lane_id();
    const KgGrid g = kg_grid(ws, 1, min_h);
    const int *start = reinterpret_cast<const int *>(ws + KG_HDR);
    const float4 *rec = reinterpret_cast<const float4 *>(ws + off_rec);
    const float r2 = radius * radius;
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
    if constexpr (WAVE) {
        const int waves = MC_THREADS / GEOT_WAVE;
        const int first = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * waves + (threadIdx.x >> 6)));
        for (long long j = first; j < m; j += (long long)gridDim.x * waves) {           // uniform over the wave
            const float4 q = rec[j];
            const BsRows rows = bs_rows(g, start, q.x, q.y, q.z, lane);
            unsigned long long sum = 0;
            for (int row = 0; row < 9; ++row) {
                const int a = __builtin_amdgcn_readlane(rows.rs, row), e = __builtin_amdgcn_readlane(rows.re, row);
                for (int c0 = a; c0 < e; c0 += GEOT_WAVE)
                    if (c0 + lane < e) sum += bs_member(q, rec[c0 + lane], r2, m, value);
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
            if (lane == 0) {
                const uint32_t key = bs_write(sum, __float_as_int(q.w), m, out);
                kmin = min(kmin, key);
                kmax = max(kmax, key);
            }
        }
    } else {
        for (long long j = (long long)blockIdx.x * MC_THREADS + threadIdx.x; j < m; j += (long long)gridDim.x * MC_THREADS) {
            const float4 q = rec[j];
            unsigned long long sum = 0;
            for (int row = 0; row < 9; ++row) {
                const BsRows rows = bs_rows(g, start, q.x, q.y, q.z, row);
                for (int c = rows.rs; c < rows.re; ++c) sum += bs_member(q, rec[c], r2, m, value);
            }
            const uint32_t key = bs_write(sum, __float_as_int(q.w), m, out);
            kmin = min(kmin, key);
            kmax = max(kmax, key);
        }
    }
    kmin = wave_min_u32(kmin);
    kmax = wave_max_u32(kmax);
    if (lane == 0 && kmin <= kmax) {          // (a wave without a query keeps the identities)
        atomicMin(&absminmax[0], kmin);
        atomicMax(&absminmax[1], kmax);
    }
}

// ---- sample -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_SAMPLE_THREADS) void cs_kernel(int m, int n_scans, long long total,
                                                               const float *__restrict__ curvature,
                                                               const uint32_t *__restrict__ absminmax,
                                                               const long long *__restrict__ offsets,
                                                               const long long *__restrict__ scan_ids,
                                                               const long long *__restrict__ sel_all, float *__restrict__ out_all,
                                                               int *__restrict__ bad)
{
    const int slot = blockIdx.x;
    const PnScan sc = pnb_scan(slot, n_scans, total, offsets, scan_ids);
    const long long *sel = sel_all + (size_t)slot * m;
    float *out = out_all + (size_t)slot * m;
    float lo = 0.f, hi = 0.f;
    if (sc.n) {
        const long long sid = scan_ids[slot];
        lo = ord2f(absminmax[2 * sid]);
        hi = ord2f(absminmax[2 * sid + 1]);
    }
    const bool spread = hi > lo;             // max == min (and a table that was never filled): 0 everywhere
    const float span = hi - lo;
    int flag = 0;
    for (int i = threadIdx.x; i < m; i += MC_SAMPLE_THREADS) {
        float o = 0.f;
        if (sc.n) {                          // an unusable slot (flag 2): nothing is read
            const long long s = sel[i];
            if (s < 0 || s >= sc.n) flag = 1;               // never an address
            else if (spread) o = (fabsf(curvature[sc.base + s]) - lo) / span;
        }
        out[i] = o;
    }
    flag = __syncthreads_or(flag);
    if (threadIdx.x == 0) bad[slot] = sc.n ? (flag ? 1 : 0) : 2;
}

static bool mc_ball_basic()
{
    const char *e = getenv("GEOT_BALL_SUM_IMPL");          // read at every call, like the other A/B switches
    return e && e[0] == 'b';
}

} // namespace geot

using namespace geot;

GEOT_EXPORT long long geot_mesh_angle_defects_ws_bytes(long long total_out)
{
    if (total_out < 0 || total_out > MC_MAX_OUT) return -1;
    return ((4 * total_out + 15) & ~15ll) + 16;             // the valence counters (never empty)
}

GEOT_EXPORT int geot_mesh_angle_defects(int b, int n_scans, long long total, long long total_faces, const float *points,
                                        const int *faces, const long long *offsets, const long long *face_offsets,
                                        const long long *scan_ids, const long long *out_offsets, const long long *face_out_offsets,
                                        long long batch_faces, long long total_out, long long *defect_q, int *stats, void *ws,
                                        long long ws_bytes, void *stream)
{
    if (b < 0 || b > 65535 || n_scans < 1 || total < 1 || total_faces < 0 || batch_faces < 0 || batch_faces > MC_MAX_FACES ||
        total_out < 0 || total_out > MC_MAX_OUT)
        return hipErrorInvalidValue;
    if (!points || !offsets || !face_offsets || !scan_ids || !out_offsets || !face_out_offsets || !defect_q ||
        (!faces && total_faces != 0))
        return hipErrorInvalidValue;
    if (!ws || ((uintptr_t)ws & 15) != 0 || ws_bytes < geot_mesh_angle_defects_ws_bytes(total_out)) return hipErrorInvalidValue;
    if (b == 0) return hipSuccess;
    hipStream_t s = (hipStream_t)stream;
    int *valence = (int *)ws;
    const long long q2pi = llrint(2.0 * M_PI * 4294967296.0);
    // a thread per vertex or face where the slots are even, a grid-stride loop where they are not (mesh_neighbours.hip's sizing)
    const long long most = 4096 / b < 1 ? 1 : 4096 / b;
    const long long per_v = total_out / ((long long)b * MC_THREADS) + 1, per_f = batch_faces / ((long long)b * MC_THREADS) + 1;
    const dim3 block(MC_THREADS), grid_v((int)(per_v > most ? most : per_v), b), grid_f((int)(per_f > most ? most : per_f), b);
    hipLaunchKernelGGL((mc_vertex_kernel<false>), grid_v, block, 0, s, n_scans, total, total_faces, offsets, face_offsets, scan_ids,
                       out_offsets, face_out_offsets, batch_faces, total_out, q2pi, defect_q, valence, stats);
    hipLaunchKernelGGL(mc_faces_kernel, grid_f, block, 0, s, n_scans, total, total_faces, offsets, face_offsets, scan_ids,
                       out_offsets, face_out_offsets, batch_faces, total_out, points, faces, defect_q, valence, stats);
    hipLaunchKernelGGL((mc_vertex_kernel<true>), grid_v, block, 0, s, n_scans, total, total_faces, offsets, face_offsets, scan_ids,
                       out_offsets, face_out_offsets, batch_faces, total_out, q2pi, defect_q, valence, stats);
    return hipGetLastError();
}

GEOT_EXPORT long long geot_scan_ball_sum_ws_bytes(int m)
{
    if (m < 1 || m > MC_MAX_SCAN) return -1;
    return (long long)(kg_layout(m).per_cloud_words * 4);   // the grid's own size
}

GEOT_EXPORT int geot_scan_ball_sum(int m, float radius, const float *points, const long long *value, float *out,
                                   unsigned *absminmax, void *ws, long long ws_bytes, void *stream)
{
    if (m < 1 || m > MC_MAX_SCAN || !(radius > 0.f) || !(radius < INFINITY)) return hipErrorInvalidValue;
    if (!points || !value || !out || !absminmax) return hipErrorInvalidValue;
    if (!ws || ((uintptr_t)ws & 15) != 0 || ws_bytes < geot_scan_ball_sum_ws_bytes(m)) return hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const KgLayout L = kg_layout(m);
    uint32_t *grid = (uint32_t *)ws;
    const float min_h = radius * 1.0001f;                   // geot_ball_query_ws' margin
    kg_build(1, m, 1, 0, min_h, points, grid, s);
    hipLaunchKernelGGL(bs_init_kernel, dim3(1), dim3(GEOT_WAVE), 0, s, absminmax);
    if (!mc_ball_basic()) {     // a lane per vertex: neighbours in the record stream walk the same block, so a wave's loads coincide
        const int blocks = (m + MC_THREADS - 1) / MC_THREADS;
        hipLaunchKernelGGL((bs_kernel<false>), dim3(blocks > 4096 ? 4096 : blocks), dim3(MC_THREADS), 0, s, m, radius, min_h, grid,
                           L.off_rec, value, out, absminmax);
    } else {
        const int waves = MC_THREADS / GEOT_WAVE, blocks = (m + waves - 1) / waves;
        hipLaunchKernelGGL((bs_kernel<true>), dim3(blocks > 4096 ? 4096 : blocks), dim3(MC_THREADS), 0, s, m, radius, min_h, grid,
                           L.off_rec, value, out, absminmax);
    }
    return hipGetLastError();
}

GEOT_EXPORT int geot_curvature_sample(int s, int m, int n_scans, long long total, const float *curvature,
                                      const unsigned *absminmax, const long long *offsets, const long long *scan_ids,
                                      const long long *sel, float *out, int *bad, void *stream)
{
    if (s < 0 || s > 65535 || m < 1 || n_scans < 1 || total < 1) return hipErrorInvalidValue;
    if (!curvature || !absminmax || !offsets || !scan_ids || !sel || !out || !bad) return hipErrorInvalidValue;
    if (s == 0) return hipSuccess;
    hipLaunchKernelGGL(cs_kernel, dim3(s), dim3(MC_SAMPLE_THREADS), 0, (hipStream_t)stream, m, n_scans, total, curvature, absminmax,
                       offsets, scan_ids, sel, out, bad);
    return hipGetLastError();
}
