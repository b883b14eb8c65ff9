// knn_grid.h -- the uniform grid of knn_grid.hip for other translation units: workspace layout, cell arithmetic, the
// wave's best-k list and the ring search of one query (knn_grid_kernel's general loop), and the host-side build.
#pragma once
#include "geot_common.h"
#include <cmath>

namespace geot {

constexpr int KG_GMAX = 32;                           // cells per axis at most
constexpr int KG_CELLS = KG_GMAX * KG_GMAX * KG_GMAX; // counters per cloud (+1)
constexpr int KG_HDR = 16;                            // header words per cloud

// workspace per cloud: [header 16 words][cell_start KG_CELLS+1 ints][tmp nr x 2 ints][records nr x 4 words]
struct KgLayout {
    size_t per_cloud_words;
    size_t off_cells, off_tmp, off_rec;
};
static inline KgLayout kg_layout(int nr)
{
    KgLayout L;
    L.off_cells = KG_HDR;
    L.off_tmp = L.off_cells + (size_t)KG_CELLS + 1;
    L.off_tmp = (L.off_tmp + 3) & ~(size_t)3;
    L.off_rec = L.off_tmp + 2 * (size_t)nr;
    L.off_rec = (L.off_rec + 3) & ~(size_t)3; // 16-byte aligned records
    L.per_cloud_words = (L.off_rec + 4 * (size_t)nr + 3) & ~(size_t)3;
    return L;
}

// order-preserving float <-> uint (for atomicMin / atomicMax on floats of either sign)
__device__ __forceinline__ uint32_t f2ord(float f)
{
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t u)
{
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

struct KgGrid {
    float lo[3];
    float h, inv_h;
    int dim[3];
};

// header words: 0-2 min (ordered), 3-5 max (ordered); grid parameters are recomputed from them by everyone
// min_h > 0 (ball query): as many cells per axis as keep the cell edge >= min_h, instead of `gtarget`
__device__ __forceinline__ KgGrid kg_grid(const uint32_t *hdr, int gtarget, float min_h = 0.f)
{
    KgGrid g;
    float ext[3], mx = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = ord2f(hdr[a]);
        ext[a] = ord2f(hdr[3 + a]) - g.lo[a];
        if (!(ext[a] >= 0.f)) ext[a] = 0.f; // empty cloud / NaN
        mx = fmaxf(mx, ext[a]);
    }
    const bool ok = mx > 0.f && mx < INFINITY;
    if (min_h > 0.f) {
        const float f = ok ? mx / min_h : 1.f;
        gtarget = f >= (float)KG_GMAX ? KG_GMAX : (f >= 1.f ? (int)f : 1);
    }
    g.h = ok ? mx / (float)gtarget : INFINITY;
    g.inv_h = ok ? (float)gtarget / mx : 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        int d = ok ? (int)(ext[a] * g.inv_h) + 1 : 1;
        g.dim[a] = d < 1 ? 1 : (d > gtarget ? gtarget : d);
    }
    return g;
}
__device__ __forceinline__ int kg_cell1(float p, float lo, float inv_h, int dim)
{
    float f = (p - lo) * inv_h;
    int c = (f >= 0.f) ? (int)fminf(f, (float)(dim - 1)) : 0; // NaN -> 0
    return c;
}

constexpr int KG_WAVES = 4;
constexpr int KG_SLOTS = 12;    // 64-record register slots of the select fast path
constexpr int KG_SEL_KMIN = 8;  // short lists are cheap to build by insertion
constexpr int KG_SEL_KMAX = 48; // beyond that the window k <= count <= 64 is too narrow to be worth probing
constexpr int KG_DPP_WAVE_SHR1 = 0x138;
__device__ __forceinline__ float kg_shr1(float v)
{
    return __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp((int)__float_as_uint(v), (int)__float_as_uint(v),
                                                                 KG_DPP_WAVE_SHR1, 0xF, 0xF, false));
}
__device__ __forceinline__ int kg_shr1(int v) { return __builtin_amdgcn_update_dpp(v, v, KG_DPP_WAVE_SHR1, 0xF, 0xF, false); }

__device__ __forceinline__ float read_lane_f(float v, int l)
{
    return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), l));
}

struct KgBest { // the wave's best-k list: lane i = i-th smallest by (d2, index); lanes >= k stay (+inf, 0)
    float ld;
    int li;
    float tau; // entry k-1, wave-uniform
    int taui;
};

// One candidate per lane (`in`: this lane has one) into the wave's best-k list, ordered by (d2, index) explicitly
__device__ __forceinline__ void kg_offer(bool in, float d, int pi, int k, KgBest &B)
{
    const int lane = lane_id();
    unsigned long long mask = __ballot(in && (d < B.tau || (d == B.tau && pi < B.taui)));
    while (mask) {
        const int l = __builtin_ctzll(mask);
        mask &= mask - 1;
        const float dc = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(d), l));
        const int ic = __builtin_amdgcn_readlane(pi, l);
        if (!(dc < B.tau || (dc == B.tau && ic < B.taui))) continue; // the threshold may have dropped
        const int pos = __popcll(__ballot(B.ld < dc || (B.ld == dc && B.li < ic)));
        const float sd = kg_shr1(B.ld);
        const int si = kg_shr1(B.li);
        B.ld = lane > pos ? sd : (lane == pos ? dc : B.ld);
        B.li = lane > pos ? si : (lane == pos ? ic : B.li);
        B.tau = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(B.ld), k - 1));
        B.taui = __builtin_amdgcn_readlane(B.li, k - 1);
    }
}

// records [s, e): 64 per step
__device__ __forceinline__ void kg_range(const float4 *__restrict__ rec, int s, int e, float qx, float qy, float qz,
                                         int k, KgBest &B)
{
    const int lane = lane_id();
    for (int c0 = s; c0 < e; c0 += 64) {
        const int r = c0 + lane;
        const bool in = r < e;
        float4 p = in ? rec[r] : make_float4(0.f, 0.f, 0.f, 0.f);
        kg_offer(in, sqdist3(qx, qy, qz, p.x, p.y, p.z), __float_as_int(p.w), k, B);
    }
}

// The ring search of one query by one wave (see knn_grid.hip's header): on return lane i of B holds the i-th smallest
// reference point by (d2, index), lanes >= k (and entries never filled) stay (+inf, 0).  B must come in initialised to
// ld = tau = +inf, li = taui = 0: "d == inf && index < 0" never holds, so infinite distances are never inserted -- as in
// the brute-force kernel, whose test is d < tau.
__device__ __forceinline__ void kg_rings(const KgGrid &g, const int *__restrict__ start, const float4 *__restrict__ rec, float qx,
                                         float qy, float qz, int cx, int cy, int cz, int rmax, int k, KgBest &B)
{
    const int lane = lane_id();
    const int dx = g.dim[0], dy = g.dim[1], dz = g.dim[2];
    for (int r = 1;; ++r) {
        // rows (y, z) of the ring: r == 1 takes the whole 3x3x3 block (rings 0 and 1); r >= 2 only the shell
        const int side = 2 * r + 1, nrows = side * side;
        for (int row0 = 0; row0 < nrows; row0 += 64) {
            // lane = row.  For the first (3 x 3) block the rows are taken nearest-first (centre, the four
            // edge neighbours, the four corners) so that the k-th distance tightens before the far rows are
            // looked at; every row also carries a lower bound of the squared distance from the query to its
            // cells, and is skipped when that already exceeds the current k-th distance.
            int row = row0 + lane;
            if (r == 1) row = (int)((0xF862075314ull >> (4 * min(lane, 9))) & 15ull); // lanes >= 9 -> row 15: skipped below
            int s0 = 0, e0 = 0, s1 = 0, e1 = 0;
            float rlb = 0.f;
            if (row < nrows) {
                const int oy = row % side - r, oz = row / side - r;
                const int y = cy + oy, z = cz + oz;
                if (y >= 0 && y < dy && z >= 0 && z < dz) {
                    const int base = (z * dy + y) * dx;
                    const bool frame = r == 1 || abs(oy) == r || abs(oz) == r;
                    if (frame) {
                        const int x0 = max(cx - r, 0), x1 = min(cx + r, dx - 1);
                        s0 = start[base + x0];
                        e0 = start[base + x1 + 1];
                    } else {
                        if (cx - r >= 0) { s0 = start[base + cx - r]; e0 = start[base + cx - r + 1]; }
                        if (cx + r < dx) { s1 = start[base + cx + r]; e1 = start[base + cx + r + 1]; }
                    }
                    // distance from the query to the row's slab in y and z (x is not used: the row spans it)
                    const float y0 = g.lo[1] + (float)y * g.h, z0 = g.lo[2] + (float)z * g.h;
                    const float ey = fmaxf(fmaxf(y0 - qy, qy - (y0 + g.h)), 0.f);
                    const float ez = fmaxf(fmaxf(z0 - qz, qz - (z0 + g.h)), 0.f);
                    const float el = fmaxf(sqrtf(ey * ey + ez * ez) * 0.99999f - g.h * 1e-3f, 0.f);
                    rlb = el * el * 0.99999f;
                    if (!(rlb >= 0.f)) rlb = 0.f; // NaN query: never skip
                }
            }
            unsigned long long live = __ballot(e0 > s0 || e1 > s1);
            while (live) {
                const int l = __builtin_ctzll(live);
                live &= live - 1;
                if (read_lane_f(rlb, l) > B.tau) continue; // strictly farther than the k-th: cannot enter, not even as a tie
                const int a0 = __builtin_amdgcn_readlane(s0, l), b0 = __builtin_amdgcn_readlane(e0, l);
                kg_range(rec, a0, b0, qx, qy, qz, k, B);
                const int a1 = __builtin_amdgcn_readlane(s1, l), b1 = __builtin_amdgcn_readlane(e1, l);
                kg_range(rec, a1, b1, qx, qy, qz, k, B);
            }
        }
        if (r >= rmax) break; // the block covers the grid
        // nearest block face that still has cells behind it
        float bound = INFINITY;
        if (cx - r > 0) bound = fminf(bound, qx - (g.lo[0] + (float)(cx - r) * g.h));
        if (cx + r < dx - 1) bound = fminf(bound, (g.lo[0] + (float)(cx + r + 1) * g.h) - qx);
        if (cy - r > 0) bound = fminf(bound, qy - (g.lo[1] + (float)(cy - r) * g.h));
        if (cy + r < dy - 1) bound = fminf(bound, (g.lo[1] + (float)(cy + r + 1) * g.h) - qy);
        if (cz - r > 0) bound = fminf(bound, qz - (g.lo[2] + (float)(cz - r) * g.h));
        if (cz + r < dz - 1) bound = fminf(bound, (g.lo[2] + (float)(cz + r + 1) * g.h) - qz);
        bound = fmaxf(bound - g.h * 1e-3f, 0.f);
        if (B.tau < bound * bound * 0.99999f) break; // NaN bound (NaN query) never breaks early: full scan
    }
}

static inline int kg_target(int nr, int k)
{
    double g = std::sqrt(3.0 * (double)nr / (5.0 * (double)(k < 1 ? 1 : k)));
    int G = (int)g;
    return G < 1 ? 1 : (G > KG_GMAX ? KG_GMAX : G);
}

// The five build kernels for b clouds of nr reference points each (b <= 65535), queued on s; ws: kg_layout(nr) per cloud.
// morton / min_h as kg_count_kernel takes them.
void kg_build(int b, int nr, int gtarget, int morton, float min_h, const float *ref, uint32_t *ws, hipStream_t s);

} // namespace geot
