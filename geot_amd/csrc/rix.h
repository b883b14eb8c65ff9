// rix.h -- the reverse index of an index gather: the pairs (source e, slot t) of idx (b, L, nt) grouped by target, the
// pairs of a list in ascending pair id.  One builder behind the channels-first list walk and geot_rix_build
// (csrc/gather_group.hip) and the EdgeConv gradient (csrc/edgeconv.hip): zero, count with rank, exclusive scan, pair ids
// into the lists (no atomics in the fill: the count pass already handed out the ranks).  Each caller then places its own
// payload with rix_sorted_position (geot_common.h), which turns the arrival order of a list into the ascending one.
#pragma once
#include "geot_common.h"

namespace geot {

// The L sources of a batch are cut into Q parts of `partlen` (Q = 1, partlen = L: one part); pairs are grouped by
// (batch, part, target), so that a workgroup holding the rows of ONE part in LDS finds exactly its entries.
// remap (b, m), Q == 1 only: the number under which a target is filed (the point-major walk's target order)
static __global__ __launch_bounds__(256) void rix_count_kernel(long long total, long long per_batch, int m, int nt, int Q,
                                                               int partlen, const int *__restrict__ idx,
                                                               int *__restrict__ cnt, int *__restrict__ rank,
                                                               const int *__restrict__ remap)
{
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x >= total) return;
    const int bi = (int)((unsigned)x / (unsigned)per_batch);                       // (pair ids fit 31 bits: rix_build_lists)
    const int part = Q > 1 ? (int)(x - (long long)bi * per_batch) / nt / partlen : 0;   // (one part: no further division)
    const int j = remap ? remap[(size_t)bi * m + idx[x]] : idx[x];
    rank[x] = atomicAdd(&cnt[((size_t)bi * Q + part) * m + j], 1);
}
// tmp[off[list] + rank] = pair id: the lists' members in arrival order, what rix_sorted_position counts over
static __global__ __launch_bounds__(256) void rix_fill_kernel(long long total, long long per_batch, int m, int nt, int Q,
                                                              int partlen, const int *__restrict__ idx,
                                                              const int *__restrict__ off, const int *__restrict__ rank,
                                                              int *__restrict__ tmp, const int *__restrict__ remap)
{
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x >= total) return;
    const int bi = (int)((unsigned)x / (unsigned)per_batch);                       // (pair ids fit 31 bits: rix_build_lists)
    const int part = Q > 1 ? (int)(x - (long long)bi * per_batch) / nt / partlen : 0;   // (one part: no further division)
    const int j = remap ? remap[(size_t)bi * m + idx[x]] : idx[x];
    tmp[off[((size_t)bi * Q + part) * m + j] + rank[x]] = (int)x;
}

// off [b Q m + 1]: the lists' offsets;  rank [pairs]: a pair's arrival number in its list;  bsum: scan_blocks(b Q m) ints
// of scratch;  tmp [pairs]: the pair ids by list, or null for callers that keep the arrival order (their place kernels
// then take rank as the position).  pairs = b * L * nt <= 0x7ffffff0 and b Q m <= 0x7ffffff0 are the caller's checks.
static inline hipError_t rix_build_lists(int b, long long L, int m, int nt, int Q, int partlen, const int *idx,
                                         const int *remap, int *off, int *bsum, int *rank, int *tmp, hipStream_t s)
{
    const long long t = (long long)b * Q * m, pairs = (long long)b * L * nt;
    hipError_t e = zero_words(off, t + 1, s);
    if (e != hipSuccess || pairs == 0) return e;
    const dim3 grid((unsigned)((pairs + 255) / 256));
    hipLaunchKernelGGL(rix_count_kernel, grid, dim3(256), 0, s, pairs, L * nt, m, nt, Q, partlen, idx, off, rank, remap);
    exclusive_scan_i32((int)t, off, bsum, nullptr, s);
    if (tmp) hipLaunchKernelGGL(rix_fill_kernel, grid, dim3(256), 0, s, pairs, L * nt, m, nt, Q, partlen, idx, off, rank, tmp, remap);
    return hipGetLastError();
}

} // namespace geot
