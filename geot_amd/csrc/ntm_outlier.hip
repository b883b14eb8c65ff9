// Class anchors behind cfg.filter_outlier (geot_ntm_filtered_anchors; examples/segmentation/train.py:510-526): per class the
// q-quantile of its probabilities over the unlabelled batch by an exact radix select, then the arg-max over the values below
// it and the anchor's soft-max row with the reference's in-place filtering.  Two launches of c workgroups x 1024 threads, no
// sort, no workspace beyond the (c) thresholds, LDS integer atomics only, nothing read back.  See include/geot_hip.h for the
// rules.
//
// Why two launches: row cc filters its columns 0..cc by THEIR thresholds (the reference edits eta in place class after class),
// so the rows need every threshold; a grid-wide wait inside one kernel would buy one launch of ~2 us for a protocol.
// Launch 1, outlier_select_kernel: order statistic `lo` of one class's M = b * n values.  The floats are mapped to unsigned
//   keys of the same order; four passes, most significant byte first, each a 256-bin histogram of the keys that still match the
//   prefix found so far, a scan of the bins, and the bin that holds the rank becomes the next byte of the prefix.  After the
//   last pass the prefix IS s[lo], the ranks passed over give the count below it and the last bin the count equal to it;
//   s[hi] (hi = lo + 1 at most) equals s[lo] when those counts cover hi, else it is the smallest key above -- one more pass,
//   taken only then.  Up to M = 48 x 1024 (the step's 2 x 24 000 points) a thread keeps its 48 keys in registers: the class
//   is read once, every load in flight together, and the passes run on chip.  Above that every pass reads the class's M
//   floats again (L2-resident after the first), 16 loads per thread in flight.
//   What bounds it: one workgroup per class is 16 waves on 4 SIMDs, so every instruction spent per value costs
//   M / 1024 x 16 cycles (0.21 us at M = 32 000) -- the instruction count, not the loads: holding the keys in registers bought
//   8 - 14 us of 75 - 109, taking the division f / n out of the per-value path (FoCursor) and two of four ballot rounds out
//   of the histogram bought 30 - 48 us, and 188 of 418 us when streaming 8 x 24 000 (profiles/filter_outlier_timing.txt).
//   Histogram form: one private histogram per wave (16 x 256 words of LDS), and within a wave equal digits are counted by
//   ballot before the atomic -- up to FO_PEEL distinct digits per wave-instruction cost one add each, whatever the number of
//   lanes; only the lanes left after that add one by one.  Probabilities make this the common case, not the exception: the top
//   byte of a key is the sign and seven exponent bits, so a whole soft-max output falls into a handful of bins, and a
//   saturated teacher's thousands of exact 1.0f (or the background class, half of all points) share every byte of all four
//   passes.  Plain per-lane atomics would send those 64 lanes to one LDS word, which serialises them (not measured here).
// Launch 2, outlier_anchor_kernel: class_anchor_kernel's scan (csrc/ntm.hip) over f = eta >= thresh[cc] ? 0 : eta, first
//   maximum in flattened (b, n) order, then the row with columns k <= cc filtered by thresh[k].
// M <= 2^24 (flat indices and counts are 32-bit; fl32(M - 1) is exact, which the rank arithmetic needs).
#include "geot_common.h"
#include "geot_hip.h"

namespace geot {

constexpr int FO_THREADS = 1024;
constexpr int FO_WAVES = FO_THREADS / GEOT_WAVE;
constexpr int FO_BINS = 256;
constexpr int FO_UNROLL = 16;       // loads in flight per thread and sweep of the streaming loops
constexpr int FO_REG = 48;          // keys per thread the select kernel holds in registers (119 VGPRs of the 128 a
                                    // 1024-thread workgroup may use; 80 and more spill to scratch)
constexpr int FO_PEEL = 2;          // distinct digits per wave-instruction counted by ballot
constexpr long long FO_MAX_POINTS = 1LL << 24;
constexpr unsigned FO_NONE = 0xffffffffu;

// the usual order-preserving map of an IEEE fp32 bit pattern (any float, -0 below +0), and back
__device__ __forceinline__ unsigned fo_key(float v)
{
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fo_value(unsigned key)
{
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// value f (flat (b, n) index, f < b * n) of the class whose first cloud starts at `src`; eta is (b, c, n)
__device__ __forceinline__ float fo_load(const float *__restrict__ src, unsigned n, unsigned cloud_stride, unsigned f)
{
    return src[(size_t)f + (size_t)(f / n) * cloud_stride];
}

// One thread's walk over its elements f = tid, tid + 1024, ... of a class, with the element's offset from the class's first
// value and no division per element: one workgroup per class is bound by its instruction count (16 waves on 4 SIMDs), and
// f / n costs about as many instructions as everything else done with a value that is only scanned.
struct FoCursor {
    unsigned f, off;            // flat (b, n) index; offset = f + (f / n) * cloud_stride
    unsigned nn, n, rs, step_off, wrap_off;
    __device__ __forceinline__ FoCursor(unsigned tid, unsigned n_, unsigned cloud_stride)
    {
        const unsigned bb = tid / n_, qs = FO_THREADS / n_;
        f = tid, n = n_, nn = tid - bb * n_, off = tid + bb * cloud_stride;
        rs = FO_THREADS - qs * n_, step_off = FO_THREADS + qs * cloud_stride, wrap_off = cloud_stride;
    }
    __device__ __forceinline__ void next()
    {
        f += FO_THREADS, off += step_off, nn += rs;
        if (nn >= n) { nn -= n; off += wrap_off; }
    }
};

// one count per active lane into this wave's own histogram; every lane of the wave calls it together
__device__ __forceinline__ void fo_count(unsigned *wh, int lane, bool active, unsigned digit)
{
    unsigned long long todo = __ballot(active);
    for (int it = 0; it < FO_PEEL && todo; ++it) {
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned dl = (unsigned)__builtin_amdgcn_readlane((int)digit, leader);
        const unsigned long long same = __ballot(active && digit == dl);
        if (lane == leader) atomicAdd(&wh[dl], (unsigned)__popcll(same));
        active = active && digit != dl;
        todo &= ~same;
    }
    if (active) atomicAdd(&wh[digit], 1u);
}

// every key of the class to body(valid, key), all threads together (uniform trip counts: body may hold ballots).  R > 0: the
// keys sit in registers, slot i = flat index i * 1024 + tid; R == 0: they are streamed from memory again
template <int R, class F>
__device__ __forceinline__ void fo_each_key(const unsigned (&reg)[R > 0 ? R : 1], const float *__restrict__ src, unsigned n,
                                            unsigned stride, unsigned total, int tid, F body)
{
    if constexpr (R > 0) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
            if ((unsigned)(i * FO_THREADS) >= total) break;
            body((unsigned)(i * FO_THREADS + tid) < total, reg[i]);
        }
    } else {
        FoCursor at(tid, n, stride);
        for (unsigned base = 0; base < total; base += FO_THREADS * FO_UNROLL) {
            float v[FO_UNROLL];
#pragma unroll
            for (int u = 0; u < FO_UNROLL; ++u) {
                v[u] = at.f < total ? src[at.off] : 0.f;
                at.next();
            }
#pragma unroll
            for (int u = 0; u < FO_UNROLL; ++u) body(base + u * FO_THREADS + tid < total, fo_key(v[u]));
        }
    }
}

// R: keys per thread held in registers across the passes (b * n <= R * 1024), 0: every pass reads the class again
template <int R>
__global__ __launch_bounds__(FO_THREADS) void outlier_select_kernel(int n, int c, unsigned total, unsigned lo, unsigned hi,
                                                                    float w, const float *__restrict__ eta,
                                                                    float *__restrict__ thresh)
{
    __shared__ unsigned hist[FO_WAVES * FO_BINS];
    __shared__ unsigned tot[FO_BINS];
    __shared__ unsigned sel[3];         // the chosen bin, the rank inside it, its count
    __shared__ unsigned wmin[FO_WAVES];
    const int cc = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *src = eta + (size_t)cc * n;
    const unsigned stride = (unsigned)(c - 1) * (unsigned)n;
    unsigned reg[R > 0 ? R : 1];
    if constexpr (R > 0) {      // all loads of the class in flight at once: one memory latency, not one per sweep and pass
        FoCursor at(tid, n, stride);
#pragma unroll
        for (int i = 0; i < R; ++i) {
            reg[i] = at.f < total ? fo_key(src[at.off]) : 0u;
            at.next();
        }
    } else {
        reg[0] = 0u;
    }
    unsigned *wh = hist + wave * FO_BINS;
    for (int e = tid; e < FO_WAVES * FO_BINS; e += FO_THREADS) hist[e] = 0u;
    if (tid == 0) { sel[0] = 0u; sel[1] = lo; sel[2] = 0u; }
    __syncthreads();
    unsigned prefix = 0u, r = lo, eq = 0u;      // workgroup-uniform: r = rank of s[lo] among the keys that match the prefix
    for (int shift = 24; shift >= 0; shift -= 8) {
        const unsigned mask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
        fo_each_key<R>(reg, src, n, stride, total, tid, [&](bool valid, unsigned key) {
            fo_count(wh, lane, valid && ((key ^ prefix) & mask) == 0u, (key >> shift) & 255u);
        });
        __syncthreads();
        if (tid < FO_BINS) {
            unsigned s = 0u;
            for (int k = 0; k < FO_WAVES; ++k) s += hist[k * FO_BINS + tid];
            tot[tid] = s;
        }
        __syncthreads();
        for (int e = tid; e < FO_WAVES * FO_BINS; e += FO_THREADS) hist[e] = 0u;      // for the next pass
        if (wave == 0) {        // four bins per lane, scanned across the wave: the one bin with  below <= r < below + count
            const unsigned b0 = tot[4 * lane], b1 = tot[4 * lane + 1], b2 = tot[4 * lane + 2], b3 = tot[4 * lane + 3];
            const unsigned s = b0 + b1 + b2 + b3;
            unsigned inc = s;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned o = __shfl_up(inc, d);
                if (lane >= d) inc += o;
            }
            const unsigned below = inc - s;
            if (r >= below && r < inc) {
                unsigned rr = r - below, d = 0u, cnt = b0;
                if (rr >= b0) {
                    rr -= b0; d = 1u; cnt = b1;
                    if (rr >= b1) {
                        rr -= b1; d = 2u; cnt = b2;
                        if (rr >= b2) { rr -= b2; d = 3u; cnt = b3; }
                    }
                }
                sel[0] = 4u * lane + d;
                sel[1] = rr;
                sel[2] = cnt;
            }
        }
        __syncthreads();
        prefix |= sel[0] << shift;
        r = sel[1];
        eq = sel[2];
    }
    // prefix = the key of s[lo]; lo - r keys lie below it, eq equal it
    const bool above = hi != lo && hi >= lo - r + eq;
    unsigned m = FO_NONE;
    if (above) {        // s[hi] = the smallest key above s[lo]
        fo_each_key<R>(reg, src, n, stride, total, tid, [&](bool valid, unsigned key) {
            if (valid && key > prefix) m = min(m, key);
        });
        m = wave_min_u32(m);
        if (lane == 0) wmin[wave] = m;
        __syncthreads();
    }
    if (tid == 0) {
        if (above)
            for (int k = 0; k < FO_WAVES; ++k) m = min(m, wmin[k]);
        // torch.quantile's linear interpolation (lerp), un-contracted fp32
        const float s_lo = fo_value(prefix), s_hi = above ? fo_value(m) : s_lo, d = s_hi - s_lo;
        thresh[cc] = w < 0.5f ? s_lo + w * d : s_hi - d * (1.f - w);
    }
}

__global__ __launch_bounds__(FO_THREADS) void outlier_anchor_kernel(int n, int c, unsigned total,
                                                                    const float *__restrict__ eta,
                                                                    const float *__restrict__ thresh,
                                                                    float *__restrict__ class_T, float *__restrict__ v_star)
{
    __shared__ float sv[FO_WAVES];
    __shared__ unsigned si[FO_WAVES];
    __shared__ unsigned win;
    const int cc = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *src = eta + (size_t)cc * n;
    const unsigned stride = (unsigned)(c - 1) * (unsigned)n;
    const float th = thresh[cc];
    float bv = 0.f;
    unsigned bi = FO_NONE;      // flat (b, n) index; a NaN never wins over a number (outside the contract, as in class_anchor_kernel)
    FoCursor at(tid, n, stride);
    for (unsigned base = 0; base < total; base += FO_THREADS * FO_UNROLL) {
        float v[FO_UNROLL];
#pragma unroll
        for (int u = 0; u < FO_UNROLL; ++u) {
            v[u] = at.f < total ? src[at.off] : 0.f;
            at.next();
        }
#pragma unroll
        for (int u = 0; u < FO_UNROLL; ++u) {
            const unsigned f = base + u * FO_THREADS + tid;
            const float fv = v[u] >= th ? 0.f : v[u];       // filtered values count as 0, they are not skipped
            if (f < total && (bi == FO_NONE || fv > bv)) { bv = fv; bi = f; }     // ascending f per thread: the first maximum
        }
    }
    // wave reduce by (value desc, index asc)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const unsigned oi = __shfl_xor(bi, o);
        const bool take = oi != FO_NONE && (bi == FO_NONE || ov > bv || (ov == bv && oi < bi));
        bv = take ? ov : bv;
        bi = take ? oi : bi;
    }
    if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        float v = sv[0];
        unsigned i = si[0];
        for (int k = 1; k < FO_WAVES; ++k) {
            const bool take = si[k] != FO_NONE && (i == FO_NONE || sv[k] > v || (sv[k] == v && si[k] < i));
            v = take ? sv[k] : v;
            i = take ? si[k] : i;
        }
        win = i;
        if (v_star) v_star[cc] = v;
    }
    __syncthreads();
    const unsigned f = win;
    if (tid < c && f < total) {     // the row after the reference's in-place edits of classes 0..cc
        const float e = fo_load(eta + (size_t)tid * n, n, stride, f);
        class_T[cc * c + tid] = (tid <= cc && e >= thresh[tid]) ? 0.f : e;
    }
}

} // namespace geot

using namespace geot;

GEOT_EXPORT int geot_ntm_filtered_anchors(int b, int n, int c, double q, const float *eta, float *class_T, float *v_star,
                                          float *thresh, void *stream)
{
    if (b < 1 || n < 1 || c < 1 || c > GEOT_NTM_MAX_C || !(q >= 0.0 && q <= 1.0) || !eta || !class_T || !thresh)
        return hipErrorInvalidValue;
    const long long total = (long long)b * n;
    if (total > FO_MAX_POINTS) return hipErrorInvalidValue;
    // torch.quantile's rank arithmetic, in fp32 as it runs there: q and M - 1 as floats, one rounded product
    const float rank = (float)q * (float)(total - 1);
    const float below = floorf(rank);
    const unsigned lo = (unsigned)below;
    const unsigned top = (unsigned)(total - 1), above = (unsigned)ceilf(rank), hi = above < top ? above : top;
    auto select = total <= FO_REG * FO_THREADS ? outlier_select_kernel<FO_REG> : outlier_select_kernel<0>;
    hipLaunchKernelGGL(select, dim3(c), dim3(FO_THREADS), 0, (hipStream_t)stream, n, c, (unsigned)total, lo, hi, rank - below,
                       eta, thresh);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(outlier_anchor_kernel, dim3(c), dim3(FO_THREADS), 0, (hipStream_t)stream, n, c, (unsigned)total, eta,
                       thresh, class_T, v_star);
    return hipGetLastError();
}
