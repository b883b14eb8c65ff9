// The batchers' vertex sample drawn on the GPU: what the reference draws per item on the host with
//   np.random.choice(N, m, replace=N < m)        openpoints/dataset/tooth_semi/tooth_dataset.py:134-135, 340-341
// (a permutation of the whole scan to keep m indices), for every slot of a batch in ONE launch.  Not numpy's stream: a
// counter-based generator, so an index depends on (seed, draw id, position) alone -- no state, no workspace, no atomics,
// no dependence on arrival order; every thread computes one output element on its own.
//
//   Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), key = (seed lo, seed hi).
//   n >= m  without replacement: sel[j] = pi_d(j), pi_d a keyed bijection on [0, 2^b) -- eight alternating unbalanced
//           Feistel rounds whose round function is word 0 of Philox on (half, round, d lo, d hi) -- walked back into
//           [0, n): while the value is >= n, pi_d is applied again (cycle walking; the walk stays on j's cycle, which
//           holds j < n itself, so it ends).  b = max(10, bits of n - 1): fewer than two applications expected from
//           n = 512 on; the floor of 10 bits is there for the small scans, whose natural width mixes too little.
//   n <  m  with replacement: sel[j] = mulhi64(w0 | w1 << 32, n), (w0, w1) of Philox on (j, 0xFFFFFFFF, d lo, d hi) --
//           the Feistel rounds use the second counter word 0..7, so the two branches never share a counter.
// geot_sample_draw_cover walks the same bijection for every n >= 1 from position pass * m + j (mod n): the passes of one
// draw id are consecutive windows of one permutation, so ceil(n / m) of them name every vertex.
// Integer arithmetic only.  tests/_sample_draw_ref.py restates all of it in numpy (tests/_scan_cover_ref.py the cover).
#include <hip/hip_runtime.h>

#include "geot_common.h"
#include "geot_hip.h"
#include "philox.h"

namespace geot {

typedef unsigned long long u64;

constexpr int SD_THREADS = 256, SD_ROUNDS = 8, SD_MIN_BITS = 10;

// pi_d on [0, 2^(lb + rb)): x = (L << rb) | R
__device__ __forceinline__ uint32_t sd_permute(uint32_t x, int rb, uint32_t mask_l, uint32_t mask_r, uint32_t d_lo, uint32_t d_hi,
                                               uint32_t k0, uint32_t k1)
{
    uint32_t left = x >> rb, right = x & mask_r;
#pragma unroll
    for (int r = 0; r < SD_ROUNDS; r += 2) {
        left ^= philox4x32_10(right, (uint32_t)r, d_lo, d_hi, k0, k1).w[0] & mask_l;
        right ^= philox4x32_10(left, (uint32_t)r + 1u, d_lo, d_hi, k0, k1).w[0] & mask_r;
    }
    return (left << rb) | right;
}

// sigma_d(x), x < n: pi_d on b = max(SD_MIN_BITS, bit length of n - 1) bits, applied again while the value is >= n
__device__ __forceinline__ uint32_t sd_sigma(uint32_t x, uint32_t n, uint32_t d_lo, uint32_t d_hi, uint32_t k0, uint32_t k1)
{
    int b = 32 - __clz((int)(n - 1u));   // bit length of n - 1 (n = 1: __clz(0) = 32 -> 0)
    b = b < SD_MIN_BITS ? SD_MIN_BITS : b;
    const int lb = b >> 1, rb = b - lb;
    const uint32_t mask_l = (1u << lb) - 1u, mask_r = (1u << rb) - 1u;
    do x = sd_permute(x, rb, mask_l, mask_r, d_lo, d_hi, k0, k1);
    while (x >= n);
    return x;
}

// grid (ceil(m / SD_THREADS), s): blockIdx.y = batch slot, one thread per output element
__global__ __launch_bounds__(SD_THREADS) void sample_draw_kernel(int m, int n_scans, long long total,
                                                                const long long *__restrict__ offsets,
                                                                const long long *__restrict__ scan_ids, u64 seed, u64 draw_base,
                                                                long long *__restrict__ sel, int *__restrict__ bad)
{
    const int slot = blockIdx.y;
    const uint32_t j = blockIdx.x * SD_THREADS + threadIdx.x;
    if (j >= (uint32_t)m) return;
    const PnScan sc = pnb_scan(slot, n_scans, total, offsets, scan_ids);
    if (j == 0) bad[slot] = sc.n ? 0 : 2;
    long long *out = sel + (size_t)slot * m;
    if (!sc.n) {                         // unusable slot (flag 2): a row of zeros
        out[j] = 0;
        return;
    }
    const u64 d = draw_base + (u64)slot;
    const uint32_t d_lo = (uint32_t)d, d_hi = (uint32_t)(d >> 32), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const uint32_t n = (uint32_t)sc.n;
    if (sc.n < m) {
        const Philox4 p = philox4x32_10(j, 0xFFFFFFFFu, d_lo, d_hi, k0, k1);
        out[j] = (long long)__umul64hi((u64)p.w[0] | ((u64)p.w[1] << 32), (u64)n);
        return;
    }
    out[j] = (long long)sd_sigma(j, n, d_lo, d_hi, k0, k1);
}

// The covering form: position q = pass * m + j of slot i's permutation, wrapped into [0, n) -- sigma_d for every n >= 1, so
// consecutive passes are consecutive windows of ONE permutation of the scan.  (pass * m + j) mod n = ((pass * m mod n) + j)
// mod n, and the inner sum stays below 2^32 (n, m < 2^31).
__global__ __launch_bounds__(SD_THREADS) void sample_draw_cover_kernel(int m, int n_scans, long long total,
                                                                      const long long *__restrict__ offsets,
                                                                      const long long *__restrict__ scan_ids, u64 seed,
                                                                      u64 draw_base, int pass, long long *__restrict__ sel,
                                                                      int *__restrict__ bad)
{
    const int slot = blockIdx.y;
    const uint32_t j = blockIdx.x * SD_THREADS + threadIdx.x;
    if (j >= (uint32_t)m) return;
    const PnScan sc = pnb_scan(slot, n_scans, total, offsets, scan_ids);
    if (j == 0) bad[slot] = sc.n ? 0 : 2;
    long long *out = sel + (size_t)slot * m;
    if (!sc.n) {                         // unusable slot (flag 2): a row of zeros
        out[j] = 0;
        return;
    }
    const u64 d = draw_base + (u64)slot;
    const uint32_t n = (uint32_t)sc.n;
    const uint32_t first = (uint32_t)(((u64)pass * (u64)m) % (u64)n);
    out[j] = (long long)sd_sigma((first + j) % n, n, (uint32_t)d, (uint32_t)(d >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}

} // namespace geot

using namespace geot;

GEOT_EXPORT int geot_sample_draw(int s, int m, int n_scans, long long total, const long long *offsets, const long long *scan_ids,
                                 unsigned long long seed, unsigned long long draw_base, long long *sel, int *bad, void *stream)
{
    if (s < 1 || s > 65535 || m < 1 || n_scans < 1 || total < 1 || !offsets || !sel || !bad) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_draw_kernel, dim3(((unsigned)m + SD_THREADS - 1) / SD_THREADS, (unsigned)s), dim3(SD_THREADS), 0,
                       (hipStream_t)stream, m, n_scans, total, offsets, scan_ids, seed, draw_base, sel, bad);
    return hipGetLastError();
}

GEOT_EXPORT int geot_sample_draw_cover(int s, int m, int n_scans, long long total, const long long *offsets,
                                       const long long *scan_ids, unsigned long long seed, unsigned long long draw_base, int pass,
                                       long long *sel, int *bad, void *stream)
{
    if (s < 1 || s > 65535 || m < 1 || n_scans < 1 || total < 1 || pass < 0 || !offsets || !sel || !bad) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_draw_cover_kernel, dim3(((unsigned)m + SD_THREADS - 1) / SD_THREADS, (unsigned)s), dim3(SD_THREADS), 0,
                       (hipStream_t)stream, m, n_scans, total, offsets, scan_ids, seed, draw_base, pass, sel, bad);
    return hipGetLastError();
}
