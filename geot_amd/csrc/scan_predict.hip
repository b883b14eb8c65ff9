// Whole-scan prediction and validation counts from device-resident scans (geot_scan_predict): for every vertex of every
// batch slot's scan -- read in place from the concatenated set -- the three nearest sampled points, get_pred_whole's
// inverse-distance interpolation of the class probabilities, the arg-max, and then the per-vertex label and / or the
// confusion counts of seg_metrics.hip.  One launch over all slots (after the grid build of the sampled points, five launches
// for all slots together); neither the neighbour indices nor the distances nor a (c, M) table reach memory.
//
// One wave per vertex, as in knn_grid_kernel: the wave loads 64 consecutive vertices (and their labels) with one
// coalesced access each, then takes them one at a time: the ring search over the slot's grid ends with the three best
// (d2, index) pairs in lanes 0..2; they are broadcast, lane l < c forms class l's interpolated value (three independent
// gathers per lane), and the first maximum (first NaN) is found with two ballots.  Lane j keeps vertex j's class, so the
// prediction is stored coalesced and the 64 (label, class) pairs go through sm_count into the wave's LDS histogram.
// The vertices are shared out by a work table made on the host from the scans' sizes: one workgroup per entry
// (slot, first vertex, vertex count), each of its waves a contiguous quarter of the entry, so ragged scans load the device
// evenly and the entry size decides how many waves a launch has (a wave is serial over its vertices).
// Without a grid (fewer than SP_MIN_REF sampled points, GEOT_NN_IMPL=basic|wave) the wave scans all n sampled points, 64
// per step, through the same insertion: the same (d2, index) order, the same bits.
//
// geot_scan_vote is the same kernel with one difference: the interpolated class values are not arg-maxed on the spot but
// stored in (GEOT_VOTE_SET) or added to a caller-owned vertex-major accumulator acc (sum of the slots' vertices, c), and with
// GEOT_VOTE_FINISH the arg-max is taken of the sum.  One writer per element, votes added in call order, no float atomics.
// Two forms of the accumulator access (GEOT_VOTE_IMPL=row|tile, read at every call; profiles/scan_vote_timing.txt):
//   row   the wave that finished vertex j adds its c values into the vertex's row: lanes < c, one 4 c-byte read (issued in
//         front of the search, which hides it) and one write;
//   tile  the values of the wave's 64 vertices go into a wave-private LDS tile [64][c | 1] (dynamic LDS, sized by c), then
//         the 64 c contiguous floats are read, added and written coalesced; with FINISH lane j arg-maxes row j of the summed
//         tile (the odd row stride keeps the 32 lanes of a half on 32 banks).
#include "geot_common.h"
#include "geot_hip.h"
#include "knn_grid.h"
#include "scan_finish.h"
#include "seg_metrics.h"
#include <cstdlib>

namespace geot {

constexpr int SP_THREADS = 256;
constexpr int SP_WAVES = SP_THREADS / GEOT_WAVE;
constexpr int SP_MIN_REF = 2048;        // geot_knn_grid_eligible's bound on the reference cloud

// all n sampled points against one query, 64 per step
__device__ __forceinline__ void sp_brute(const float *__restrict__ K, int n, float qx, float qy, float qz, KgBest &B)
{
    const int lane = lane_id();
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int r = c0 + lane;
        const bool in = r < n;
        float px = 0.f, py = 0.f, pz = 0.f;
        if (in) { px = K[(size_t)r * 3]; py = K[(size_t)r * 3 + 1]; pz = K[(size_t)r * 3 + 2]; }
        kg_offer(in, sqdist3(qx, qy, qz, px, py, pz), r, 3, B);
    }
}

// sm_interp_argmax (seg_metrics.hip) with the classes spread over the lanes, in two halves.  The interpolation: the same
// statements per class; lane l < c returns class l's value, the others 0.
__device__ __forceinline__ float sp_interp(const float *__restrict__ prob, int c, int n, const KgBest &B)
{
    const int lane = lane_id();
    const int i0 = __builtin_amdgcn_readlane(B.li, 0), i1 = __builtin_amdgcn_readlane(B.li, 1), i2 = __builtin_amdgcn_readlane(B.li, 2);
    const float d0 = read_lane_f(B.ld, 0), d1 = read_lane_f(B.ld, 1), d2 = read_lane_f(B.ld, 2);
    const float r0 = 1.0f / (sqrtf(d0) + 1e-8f), r1 = 1.0f / (sqrtf(d1) + 1e-8f), r2 = 1.0f / (sqrtf(d2) + 1e-8f);
    const float norm = (r0 + r2) + r1;
    const float w0 = r0 / norm, w1 = r1 / norm, w2 = r2 / norm;
    float v = 0.f;
    if (lane < c) {
        const float *P = prob + (size_t)lane * n;
        const float p0 = P[i0], p1 = P[i1], p2 = P[i2];
        v = p0 * w0 + p1 * w1 + p2 * w2;
    }
    return v;
}

// torch.argmax's rule over the values of lanes < c -- the first NaN if there is one, else the first maximum.  Wave-uniform.
__device__ __forceinline__ int sp_argmax(float v, int c)
{
    const bool in = lane_id() < c;
    const unsigned long long nan = __ballot(in && v != v);
    if (nan) return __builtin_ctzll(nan);
    const float mx = wave_max_f32(in ? v : -INFINITY);
    return __builtin_ctzll(__ballot(in && v == mx));     // c >= 1: lane 0 is in, so the ballot is not empty
}

// (the same rule over one row of a summed tile, and the wave's LDS ordering: scan_finish.h)

constexpr int SP_PREDICT = 0, SP_VOTE_ROW = 1, SP_VOTE_TILE = 2;     // what a kernel does with the interpolated values

template <bool GRID, int FORM>
__global__ __launch_bounds__(SP_THREADS) void scan_predict_kernel(
    int b, int c, int n, int gtarget, long long total, const float *__restrict__ points, const int *__restrict__ labels,
    const long long *__restrict__ offsets, int n_scans, const long long *__restrict__ scan_ids,
    const float *__restrict__ known, const float *__restrict__ prob, const int4 *__restrict__ work,
    const uint32_t *__restrict__ ws, size_t per_cloud, size_t off_rec, const long long *__restrict__ out_offsets,
    long long *__restrict__ pred, unsigned long long *__restrict__ counts, float *__restrict__ acc, int mode)
{
    __shared__ unsigned h[SP_WAVES * SM_MAX_SLOTS];
    extern __shared__ float tiles[];             // SP_VOTE_TILE: SP_WAVES tiles of 64 rows of c | 1 floats
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
        for (int i = threadIdx.x; i < SP_WAVES * slots; i += SP_THREADS) h[i] = 0;
        __syncthreads();
    }
    const float *V = points + (size_t)lo * 3;
    const float *K = known + (size_t)s * n * 3;
    const float *P = prob + (size_t)s * c * n;
    const uint32_t *W = ws + (size_t)s * per_cloud;
    KgGrid g = {};
    const int *start = nullptr;
    const float4 *rec = nullptr;
    if constexpr (GRID) {
        g = kg_grid(W, gtarget);
        start = reinterpret_cast<const int *>(W + KG_HDR);
        rec = reinterpret_cast<const float4 *>(W + off_rec);
    }
    const long long out0 = (FORM != SP_PREDICT || pred) ? out_offsets[s] : 0;
    // votes: SET stores where the others add; the arg-max is taken with FINISH, and only for someone who reads it
    const bool set = (mode & GEOT_VOTE_SET) != 0;
    const bool finish = (mode & GEOT_VOTE_FINISH) != 0 && (pred || counts);
    const int cs = c | 1;
    float *tile = tiles + (FORM == SP_VOTE_TILE ? wave * 64 * cs : 0);

    // the entry's vertices in SP_WAVES contiguous runs, one per wave; a wave takes its run 64 vertices at a time
    const long long per = ((long long)(end - first) + SP_WAVES - 1) / SP_WAVES;
    const long long w0 = first + wave * per, w1 = w0 + per < end ? w0 + per : end;
    for (long long base = w0; base < w1; base += 64) {
        const int cnt = w1 - base < 64 ? (int)(w1 - base) : 64;
        const bool active = lane < cnt;
        const long long v = base + lane;
        float vx = 0.f, vy = 0.f, vz = 0.f;
        if (active) { vx = V[(size_t)v * 3]; vy = V[(size_t)v * 3 + 1]; vz = V[(size_t)v * 3 + 2]; }
        int cls = 0;
        for (int j = 0; j < cnt; ++j) {
            const float qx = read_lane_f(vx, j), qy = read_lane_f(vy, j), qz = read_lane_f(vz, j);
            KgBest B;
            B.ld = INFINITY; B.li = 0; B.tau = INFINITY; B.taui = 0;
            float *row = nullptr;
            float old = 0.f;
            if constexpr (FORM == SP_VOTE_ROW) {     // the vertex's row so far: read here, needed after the search
                row = acc + (size_t)(out0 + base + j) * c;
                if (!set && lane < c) old = row[lane];
            }
            if constexpr (GRID) {
                const int cx = kg_cell1(qx, g.lo[0], g.inv_h, g.dim[0]);
                const int cy = kg_cell1(qy, g.lo[1], g.inv_h, g.dim[1]);
                const int cz = kg_cell1(qz, g.lo[2], g.inv_h, g.dim[2]);
                const int rmax = max(max(max(cx, g.dim[0] - 1 - cx), max(cy, g.dim[1] - 1 - cy)), max(cz, g.dim[2] - 1 - cz));
                kg_rings(g, start, rec, qx, qy, qz, cx, cy, cz, rmax, 3, B);
            } else {
                sp_brute(K, n, qx, qy, qz, B);
            }
            const float val = sp_interp(P, c, n, B);
            if constexpr (FORM == SP_PREDICT) {
                const int a = sp_argmax(val, c);
                if (lane == j) cls = a;
            } else if constexpr (FORM == SP_VOTE_ROW) {
                const float sum = set ? val : old + val;
                if (lane < c) row[lane] = sum;
                if (finish) {
                    const int a = sp_argmax(sum, c);
                    if (lane == j) cls = a;
                }
            } else {
                if (lane < c) tile[j * cs + lane] = val;
            }
        }
        if constexpr (FORM == SP_VOTE_TILE) {       // the wave's cnt rows are contiguous in acc: one coalesced read-add-write
            sp_wave_lds_sync();
            float *A = acc + (size_t)(out0 + base) * c;
            for (int i = lane; i < cnt * c; i += 64) {
                const int r = i / c;
                float *t = tile + r * cs + (i - r * c);
                const float sum = set ? *t : A[i] + *t;
                A[i] = sum;
                *t = sum;
            }
            sp_wave_lds_sync();
            if (finish && active) cls = sp_argmax_row(tile + lane * cs, c);
            sp_wave_lds_sync();
        }
        if (pred && active) pred[out0 + v] = cls;
        if (counts) {
            const int key = active ? sm_slot(labels[lo + v], cls, c) : 0;
            sm_count(hw, key, active);
        }
    }
    if (counts) {
        __syncthreads();
        for (int i = threadIdx.x; i < slots; i += SP_THREADS) {
            unsigned t = 0;
#pragma unroll
            for (int w = 0; w < SP_WAVES; ++w) t += h[w * slots + i];
            if (t) atomicAdd(&counts[(size_t)s * slots + i], (unsigned long long)t);
        }
    }
}

static bool sp_use_grid(int n)
{
    const char *e = getenv("GEOT_NN_IMPL");     // read at every call, as geot_knn_grid_eligible does
    if (e && (e[0] == 'b' || e[0] == 'w')) return false;
    return n >= SP_MIN_REF;
}

} // namespace geot

using namespace geot;

GEOT_EXPORT long long geot_scan_predict_ws_bytes(int b, int n)
{
    if (b < 1 || b > 65535 || n < 1) return -1;
    return geot_knn_grid_ws_bytes(b, n);
}

// The argument checks and launches both entry points share.  form: what the kernel does with the interpolated values.
static int sp_run(int form, int b, int c, int n, int n_scans, long long total, const float *points, const int *labels,
                  const long long *offsets, const long long *scan_ids, const float *known, const float *prob, int n_work,
                  const int *work, const long long *out_offsets, float *acc, int mode, long long *pred, long long *counts,
                  void *ws, long long ws_bytes, void *stream)
{
    if (b < 0 || b > 65535 || c < 1 || c > GEOT_NTM_MAX_C || n < 1 || n_scans < 1 || total < 1 || n_work < 0)
        return hipErrorInvalidValue;
    if (!points || !offsets || !scan_ids || !known || !prob || (counts && !labels)) return hipErrorInvalidValue;
    if (form == SP_PREDICT) {
        if ((!pred && !counts) || (pred && !out_offsets)) return hipErrorInvalidValue;
    } else {
        if (!acc || !out_offsets || (mode & ~(GEOT_VOTE_SET | GEOT_VOTE_FINISH)) != 0) return hipErrorInvalidValue;
        if ((pred || counts) && !(mode & GEOT_VOTE_FINISH)) return hipErrorInvalidValue;
    }
    if (b == 0 || n_work == 0) return hipSuccess;
    if (!work || ((uintptr_t)work & 15) != 0) return hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *out = reinterpret_cast<unsigned long long *>(counts);
    const int4 *jobs = reinterpret_cast<const int4 *>(work);
    const bool grid = sp_use_grid(n);
    const uint32_t *W = nullptr;
    size_t per_cloud = 0, off_rec = 0;
    int G = 0;
    if (grid) {
        if (!ws || ((uintptr_t)ws & 15) != 0 || ws_bytes < geot_knn_grid_ws_bytes(b, n)) return hipErrorInvalidValue;
        const KgLayout L = kg_layout(n);
        G = kg_target(n, 3);
        kg_build(b, n, G, 0, 0.f, known, (uint32_t *)ws, s);
        W = (const uint32_t *)ws;
        per_cloud = L.per_cloud_words;
        off_rec = L.off_rec;
    }
    const size_t lds = form == SP_VOTE_TILE ? (size_t)SP_WAVES * 64 * (c | 1) * sizeof(float) : 0;
#define SP_LAUNCH(GRID, FORM)                                                                                                  \
    hipLaunchKernelGGL((scan_predict_kernel<GRID, FORM>), dim3(n_work), dim3(SP_THREADS), lds, s, b, c, n, G, total, points,    \
                       labels, offsets, n_scans, scan_ids, known, prob, jobs, W, per_cloud, off_rec, out_offsets, pred, out, acc, \
                       mode)
    if (form == SP_PREDICT) {
        if (grid) SP_LAUNCH(true, SP_PREDICT); else SP_LAUNCH(false, SP_PREDICT);
    } else if (form == SP_VOTE_ROW) {
        if (grid) SP_LAUNCH(true, SP_VOTE_ROW); else SP_LAUNCH(false, SP_VOTE_ROW);
    } else {
        if (grid) SP_LAUNCH(true, SP_VOTE_TILE); else SP_LAUNCH(false, SP_VOTE_TILE);
    }
#undef SP_LAUNCH
    return hipGetLastError();
}

GEOT_EXPORT int geot_scan_predict(int b, int c, int n, int n_scans, long long total, const float *points, const int *labels,
                                  const long long *offsets, const long long *scan_ids, const float *known, const float *prob,
                                  int n_work, const int *work, const long long *out_offsets, long long *pred,
                                  long long *counts, void *ws, long long ws_bytes, void *stream)
{
    return sp_run(SP_PREDICT, b, c, n, n_scans, total, points, labels, offsets, scan_ids, known, prob, n_work, work, out_offsets,
                  nullptr, 0, pred, counts, ws, ws_bytes, stream);
}

GEOT_EXPORT int geot_scan_vote(int b, int c, int n, int n_scans, long long total, const float *points, const int *labels,
                               const long long *offsets, const long long *scan_ids, const float *known, const float *prob,
                               int n_work, const int *work, const long long *out_offsets, float *acc, int mode, long long *pred,
                               long long *counts, void *ws, long long ws_bytes, void *stream)
{
    const char *e = getenv("GEOT_VOTE_IMPL");      // read at every call; the default is the form that measured faster
    const int form = e && e[0] == 't' ? SP_VOTE_TILE : SP_VOTE_ROW;
    return sp_run(form, b, c, n, n_scans, total, points, labels, offsets, scan_ids, known, prob, n_work, work, out_offsets, acc,
                  mode, pred, counts, ws, ws_bytes, stream);
}
