// ntm_generic.hip -- the per-point transition-matrix kernels for ANY class count 2 <= C <= 32.
//
// The reference builds `nclasses` Linear(2C -> C) heads for whatever nclasses the config names
// (openpoints/models/backbone/transformer.py:1104-1110) and its losses take num_classes as an argument
// (utils/insT_loss.py:62-67).  ntm.hip holds the kernels specialised for the configured tooth label set
// (C = 17: MFMA tiles of 289 columns, LDS tiles of 32 x 289 floats); this file serves every other count with
// one mapping that needs no compile-time C:
//
//     one wave per point, a half-wave (32 lanes) per matrix row, lane = column  (C <= 32)
//
// so the L1 norms / dot products over a row are five xor-shuffles inside the half-wave, a row of T_i is one
// contiguous 4C-byte access of the half-wave (two adjacent rows per wave instruction), and nothing goes
// through shared memory except the read-only weights.  Lane efficiency is C/32; these are streaming kernels
// over (B*N, C, C) and stay HBM-bound from C ~ 12 up.  Same arithmetic, same operation order per element as the
// specialised kernels (one reciprocal per row).
#include "geot_common.h"
#include "ntm_generic.h"

namespace geot {

__device__ __forceinline__ float half_sum(float v)   // sum over the 32 lanes of this lane's half-wave
{
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- sig_t_mean forward / d raw ---------------------------------------------------------------------------
// raw[kk][o] = sum_j p_j W[kk][o][j] + sum_j cm[kk][j] W[kk][o][C+j];  clamp to [1e-5, 1-1e-5];  L1-normalise over o.
// BACKWARD: out = d raw = [raw inside the clamp] * (g - sum_o g tn) / den   (the d/dW GEMM is the caller's).
template <bool BACKWARD>
__global__ __launch_bounds__(256) void gen_sig_t_mean_kernel(int total_pts, int n, int c, const float *__restrict__ p,
                                                             const float *__restrict__ W, const float *__restrict__ cm,
                                                             const float *__restrict__ grad_out, float *__restrict__ out)
{
    extern __shared__ float gen_lds[];
    const int cc = c * c;
    float *Wl = gen_lds;          // [j][kk*c + o] = W[kk][o][j]   (lanes o read consecutive words)
    float *bias = Wl + c * cc;    // [kk*c + o]
    for (int e = threadIdx.x; e < c * cc; e += 256) {
        const int j = e / cc, col = e - j * cc;
        Wl[e] = W[(size_t)col * 2 * c + j];
    }
    for (int col = threadIdx.x; col < cc; col += 256) {
        const int kk = col / c;
        float acc = 0.f;
        for (int j = 0; j < c; ++j) acc += cm[kk * c + j] * W[(size_t)col * 2 * c + c + j];
        bias[col] = acc;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, o = lane & 31, h = lane >> 5;
    const bool live_o = o < c;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < total_pts; i += gridDim.x * 4) {
        const int b = i / n, ni = i - b * n;
        const float pl = lane < c ? p[((size_t)b * c + lane) * n + ni] : 0.f;   // lane j holds p_j
        for (int k0 = 0; k0 < c; k0 += 2) {
            const int kk = k0 + h;
            const bool live = live_o && kk < c;
            const int col = live ? kk * c + o : 0;
            float raw = live ? bias[col] : 0.f;
            for (int j = 0; j < c; ++j) {
                const float pj = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(pl), j));
                raw = fmaf(pj, live ? Wl[j * cc + col] : 0.f, raw);
            }
            const float cl = live ? fminf(fmaxf(raw, 1e-5f), 1.f - 1e-5f) : 0.f;   // clamped values are positive
            const float rden = 1.f / fmaxf(half_sum(cl), 1e-12f);
            if (!BACKWARD) {
                if (live) out[(size_t)i * cc + col] = cl * rden;
            } else {
                const float g = live ? grad_out[(size_t)i * cc + col] : 0.f;
                const float dot = half_sum(g * (cl * rden));
                const bool inside = raw >= 1e-5f && raw <= 1.f - 1e-5f;
                if (live) out[(size_t)i * cc + col] = inside ? (g - dot) * rden : 0.f;
            }
        }
    }
}

// ---- sig_t_mean, second form: lane = point ------------------------------------------------------------------------
// The wave-per-point kernel above reads a weight from LDS for every multiply and leaves C/32 of its lanes idle
// (0.5 TB/s at C = 16).  Here a wave takes 64 consecutive points, one per lane: the point's probabilities sit in CP
// registers (CP = C rounded up to 8, a template parameter so that the arrays are statically indexed), the weights are
// wave-uniform and come through the SCALAR path (s_load), the clamp / L1 norm / dot product of a row are lane-local --
// no shuffles -- and a row of 64 x C results crosses a wave-private LDS tile so that global memory sees 4C-byte
// segments instead of one 4-byte store per lane.  d raw (BACKWARD) takes its incoming gradient through the same tile.
template <int CP, bool BACKWARD>
__global__ __launch_bounds__(256) void gen_sig_t_mean_rows_kernel(int total_pts, int n, int c, const float *__restrict__ p,
                                                                  const float *__restrict__ W, const float *__restrict__ cm,
                                                                  const float *__restrict__ grad_out, float *__restrict__ out)
{
    extern __shared__ float gen_lds[];
    const int cc = c * c, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *bias = gen_lds;                                           // [kk*c + o] = sum_j cm[kk][j] W[kk][o][c + j]
    float *tile = gen_lds + ((cc + 3) & ~3) + wave * 64 * (CP + 1);  // [point][CP + 1]: odd stride, conflict-free rows
    for (int col = threadIdx.x; col < cc; col += 256) {
        const int kk = col / c;
        float acc = 0.f;
        for (int j = 0; j < c; ++j) acc += cm[kk * c + j] * W[(size_t)col * 2 * c + c + j];
        bias[col] = acc;
    }
    __syncthreads();
    const int jmax = 2 * c - 1;                                      // last valid column of a weight row (padded reads stay inside it)
    for (long long i0 = ((long long)blockIdx.x * 4 + wave) * 64; i0 < total_pts; i0 += (long long)gridDim.x * 256) {
        const long long i = i0 + lane;
        const bool ok = i < total_pts;
        const int b = ok ? (int)(i / n) : 0, ni = ok ? (int)(i - (long long)b * n) : 0;
        float pv[CP];
#pragma unroll
        for (int j = 0; j < CP; ++j) pv[j] = (ok && j < c) ? p[((size_t)b * c + j) * n + ni] : 0.f;
        const int cnt = (int)min((long long)64, total_pts - i0);    // points of this wave's tile
        for (int kk = 0; kk < c; ++kk) {
            float *gdst = out + (size_t)i0 * cc + (size_t)kk * c;    // + point * cc + o
            float g[CP];
            if (BACKWARD) {
                // incoming gradient of row kk: coalesced segments -> tile -> one row per lane
                const float *gsrc = grad_out + (size_t)i0 * cc + (size_t)kk * c;
                int pt = lane / c, o = lane - pt * c;
                const int dp = 64 / c, dq = 64 - dp * c;
                for (int e = lane; e < cnt * c; e += 64) {
                    tile[pt * (CP + 1) + o] = gsrc[(size_t)pt * cc + o];
                    pt += dp; o += dq;
                    if (o >= c) { o -= c; ++pt; }
                }
                __builtin_amdgcn_wave_barrier();
                __threadfence_block();
#pragma unroll
                for (int o2 = 0; o2 < CP; ++o2) g[o2] = (o2 < c) ? tile[lane * (CP + 1) + o2] : 0.f;
                __builtin_amdgcn_wave_barrier();
                __threadfence_block();
            }
            float raw[CP], s = 0.f;
#pragma unroll
            for (int o = 0; o < CP; ++o) {
                raw[o] = 0.f;
                if (o < c) {                                         // wave-uniform
                    const float *wrow = W + ((size_t)kk * c + o) * 2 * c;
                    float acc = bias[kk * c + o];
#pragma unroll
                    for (int j = 0; j < CP; ++j) acc = fmaf(pv[j], wrow[min(j, jmax)], acc);   // pv[j] = 0 beyond c
                    raw[o] = acc;
                    s += fminf(fmaxf(acc, 1e-5f), 1.f - 1e-5f);      // clamped values are positive
                }
            }
            const float rden = 1.f / fmaxf(s, 1e-12f);
            if (!BACKWARD) {
#pragma unroll
                for (int o = 0; o < CP; ++o)
                    if (o < c) tile[lane * (CP + 1) + o] = fminf(fmaxf(raw[o], 1e-5f), 1.f - 1e-5f) * rden;
            } else {
                float dot = 0.f;
#pragma unroll
                for (int o = 0; o < CP; ++o)
                    if (o < c) dot += g[o] * (fminf(fmaxf(raw[o], 1e-5f), 1.f - 1e-5f) * rden);
#pragma unroll
                for (int o = 0; o < CP; ++o)
                    if (o < c) {
                        const bool inside = raw[o] >= 1e-5f && raw[o] <= 1.f - 1e-5f;
                        tile[lane * (CP + 1) + o] = inside ? (g[o] - dot) * rden : 0.f;
                    }
            }
            __builtin_amdgcn_wave_barrier();
            __threadfence_block();
            {
                int pt = lane / c, o = lane - pt * c;
                const int dp = 64 / c, dq = 64 - dp * c;
                for (int e = lane; e < cnt * c; e += 64) {
                    gdst[(size_t)pt * cc + o] = tile[pt * (CP + 1) + o];
                    pt += dp; o += dq;
                    if (o >= c) { o -= c; ++pt; }
                }
            }
            __builtin_amdgcn_wave_barrier();
            __threadfence_block();
        }
    }
}

// ---- sig_t_mean, third form: the heads on the matrix cores, any C <= 32 ---------------------------------------------
// The lane-per-point kernel above spends C^2 scalar-fed FMAs per point and head on the vector pipe and refetches 8 C^3
// bytes of weights through the scalar cache per wave tile (C = 20: 0.8 TB/s).  The heads are a GEMM with K = C:
//     raw[kk][o][pt] = bias[kk][o] + sum_j W[kk][o][j] p[pt][j]
// done as v_mfma_f32_32x32x2_f32 tiles with the WEIGHTS on the row side and 32 POINTS on the column side, so that in the
// result a lane owns one point (column = lane & 31) and 16 of a tile's 32 rows: clamp, L1 norm and the backward's dot
// product over o are 16 in-lane steps plus one exchange with lane ^ 32 -- no workgroup barrier in the loop.
// A row tile holds 32 / CPAD heads of CPAD rows (CPAD = 8, 16, 32 >= C), the bias starts the accumulator, the weight
// fragments of every (row tile, 4 K steps) sit in LDS in fragment order (one ds_read_b128 per 4 MFMAs), each wave walks its
// own point tiles.  In that layout neighbouring lanes hold neighbouring POINTS (4 C^2 bytes apart): written from there, every
// 16-byte piece is a memory request of its own and the address path bounds the kernel (knock-outs at C = 32: stores 100 of
// 290 us, not overlapping the MFMAs' 100 -- profiles/r05_ntm_generic.txt).  So a row tile's results cross a wave-private LDS
// tile ([32 points][32 rows + 4]) and leave in the order of the output: 8 lanes per 128 contiguous bytes; the backward's
// incoming gradient takes the same way in.  A workgroup serves one of `ksplit` ranges of row tiles (its weights: 1 / ksplit
// of C^3 floats; 16 waves x 4.5 KB of tiles), the point tiles are dealt over the workgroups of a range.
// Memory operations of a wave retire in order (one vmcnt counter for loads and stores), so a load issued behind a tile's stores
// waits for them: the forward fetches the NEXT point tile's fragments before the first store of this one, the backward the
// NEXT row tile's gradient pieces (a counted wait then leaves one row tile of stores in flight).
typedef float gen_f32x16 __attribute__((ext_vector_type(16)));
typedef float gen_f32x4 __attribute__((ext_vector_type(4)));
typedef float gen_f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte piece at 4-byte alignment (one dwordx4 access)
constexpr int GEN_MT = 1024, GEN_MW = GEN_MT / 64;
constexpr int GEN_RS = 36;        // floats per point in a wave's tile: 32 rows (NG heads of CPAD) + 4, so that rows start 4 banks apart
constexpr int GEN_NI = 4;         // 16-byte pieces per lane of a tile's dense image: 32 points x <= 8 pieces over 64 lanes

// TAILS: C is not a multiple of 4 -- pieces of the dense image straddle heads and the last one of a point is partial
template <int CPAD, bool BACKWARD, bool TAILS>
__global__ __launch_bounds__(GEN_MT) void gen_sig_t_mean_mfma_kernel(int total_pts, int n, int c, int ksplit, const float *__restrict__ p,
                                                                     const float *__restrict__ W, const float *__restrict__ cm,
                                                                     const float *__restrict__ grad_out, float *__restrict__ out)
{
    constexpr int NG = 32 / CPAD, QPG = CPAD / 8, KSMAX = CPAD / 2;   // heads per row tile, 8-row blocks per head, K steps
    constexpr bool AHEAD = BACKWARD && !TAILS;                        // (the TAILS forms have no registers for the second set of pieces)
    extern __shared__ float gen_lds[];
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cc = c * c, nkt = (c + NG - 1) / NG, ng = (c + 7) / 8;   // row tiles; groups of 4 K steps (8 inputs)
    const int part = blockIdx.x % ksplit, wb = blockIdx.x / ksplit, nb = gridDim.x / ksplit;
    const int kt0 = nkt * part / ksplit, kt1 = nkt * (part + 1) / ksplit, nktmax = (nkt + ksplit - 1) / ksplit;
    float *Af = gen_lds;                         // [kt1 - kt0][ng][64][4]: lane (row, half), element e holds W[kk][o][2 (4 g + e) + half]
    float *Bt = Af + (size_t)nktmax * ng * 256;  // [kt1 - kt0][32]: bias of the tile's rows
    float *tile = Bt + nktmax * 32 + wave * (32 * GEN_RS);
    // (every workgroup builds both from W: coalesced reads in W's own order, scattered LDS writes; the padding is zeroed first)
    for (int e = tid; e < (kt1 - kt0) * ng * 64; e += GEN_MT) reinterpret_cast<gen_f32x4 *>(Af)[e] = gen_f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    const int kk0 = kt0 * NG, kk1 = min(c, kt1 * NG);
    for (int e = tid; e < (kk1 - kk0) * cc; e += GEN_MT) {
        const int col = kk0 * c + e / c, j = e % c, kk = col / c, o = col - kk * c;
        const int kt = kk / NG - kt0, row = (kk % NG) * CPAD + o, st = j >> 1;
        Af[(((kt * ng + (st >> 2)) * 64) + (j & 1) * 32 + row) * 4 + (st & 3)] = W[(size_t)col * 2 * c + j];
    }
    for (int e = tid; e < (kt1 - kt0) * 32; e += GEN_MT) {              // (ascending j, as the other two forms: same bits)
        const int row = e & 31, kk = (kt0 + (e >> 5)) * NG + row / CPAD, o = row % CPAD;
        float acc = 0.f;
        if (kk < c && o < c) {
            const float *wr = W + ((size_t)kk * c + o) * 2 * c + c, *cr = cm + kk * c;
            for (int j0 = 0; j0 < c; j0 += 8) {                         // 16 loads in flight per round
                float a[8], w[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    a[j] = cr[min(j0 + j, c - 1)];
                    w[j] = wr[min(j0 + j, c - 1)];
                }
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (j0 + j < c) acc += a[j] * w[j];
            }
        }
        Bt[e] = acc;
    }
    __syncthreads();

    // The dense image of a (point tile, row tile): per point NG c contiguous floats (heads kt NG .. of the point's C x C block),
    // as ceil(NG c / 4) pieces.  Lane `lane` moves pieces lane + 64 i: point, first dense element, address in the LDS tile.
    const int seg = NG * c, pieces = (seg + 3) >> 2;
    unsigned ppt[GEN_NI], pd0[GEN_NI], plo[GEN_NI];
#pragma unroll
    for (int i = 0; i < GEN_NI; ++i) {
        const int f = lane + 64 * i, pt = min(f / pieces, 31), d0 = (f - (f / pieces) * pieces) * 4;
        const int g = TAILS ? 0 : d0 / c;                              // (whole pieces: inside one head)
        ppt[i] = f < 32 * pieces ? pt : 32u;                            // 32: no piece
        pd0[i] = d0;
        plo[i] = pt * GEN_RS + g * CPAD + (d0 - g * c);
    }
    auto lds_of = [&](int pt, int d) {       // TAILS: element d of a point's dense image -> its place in the tile
        const int g = (NG > 1 && d >= c ? 1 : 0) + (NG > 2 && d >= 2 * c ? 1 : 0) + (NG > 2 && d >= 3 * c ? 1 : 0);
        return pt * GEN_RS + g * CPAD + (d - g * c);
    };
    const long long tiles = ((long long)total_pts + 31) / 32, tstride = (long long)nb * GEN_MW;
    const unsigned last4 = (unsigned)total_pts * (unsigned)cc - 4u;     // (gen_sig_plan: 4 <= B N C^2 < 2^30)
    long long t = (long long)wb * GEN_MW + wave;
    if (t >= tiles || kt1 <= kt0) return;
    auto point = [&](long long tl, bool &ok, unsigned &pbase) {
        const long long i = tl * 32 + r;
        ok = i < total_pts;
        const long long ic = ok ? i : (long long)total_pts - 1;
        const int b = (int)(ic / n), ni = (int)(ic - (long long)b * n);
        pbase = (unsigned)(b * c * n + ni);  // 32-bit element offsets: uniform base + lane offset
    };
    auto fetch_p = [&](float (&dst)[KSMAX], unsigned pbase) {           // column side: lane (point, half) holds p[point][2 s + half]
#pragma unroll
        for (int s = 0; s < KSMAX; ++s) dst[s] = p[pbase + (unsigned)(min(2 * s + h, c - 1) * n)];
    };
    // the pieces of (point tile tl, row tile kt) of the incoming gradient: unconditional loads, clamped into the buffer
    auto fetch_g = [&](gen_f32x4u (&dst)[GEN_NI], long long tl, int kt) {
        const unsigned base = (unsigned)(tl * 32) * (unsigned)cc + (unsigned)(kt * NG * c);
#pragma unroll
        for (int i = 0; i < GEN_NI; ++i) {
            const unsigned off = base + min(ppt[i], 31u) * (unsigned)cc + pd0[i];
            dst[i] = *reinterpret_cast<const gen_f32x4u *>(grad_out + min(off, last4));
        }
    };
    bool ok;
    unsigned pbase;
    point(t, ok, pbase);
    float bf[KSMAX], bfn[KSMAX];
    gen_f32x4u g4[GEN_NI], g4n[GEN_NI];
    fetch_p(bf, pbase);
    if (AHEAD) fetch_g(g4, t, kt0);
    while (true) {
        const long long tn = t + tstride;
        const bool more = tn < tiles;
        bool okn;
        unsigned pbasen;
        point(more ? tn : t, okn, pbasen);
        if (!BACKWARD) fetch_p(bfn, pbasen);
        const int npts = (int)min((long long)32, (long long)total_pts - t * 32);
        const unsigned tbase = (unsigned)(t * 32) * (unsigned)cc;
        for (int kt = kt0; kt < kt1; ++kt) {
            const int segk = min(NG, c - kt * NG) * c;                 // valid floats of a point's image in this row tile
            const unsigned kbase = tbase + (unsigned)(kt * NG * c);
            float gv[16];
            if (BACKWARD) {
                // this row tile's gradient pieces -> tile -> the result's layout; then the next row tile's pieces take off
                if (!AHEAD) fetch_g(g4, t, kt);
#pragma unroll
                for (int i = 0; i < GEN_NI; ++i) {
                    if (ppt[i] < 32u) {
                        if (!TAILS) *reinterpret_cast<gen_f32x4 *>(tile + plo[i]) = g4[i];
                        else {
                            const unsigned off = kbase + ppt[i] * (unsigned)cc + pd0[i];
                            const int sh = (int)(off - min(off, last4));        // the clamped load began sh elements early
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float x = sh == 0 ? g4[i][e] : (sh == 1 ? g4[i][(e + 1) & 3] : (sh == 2 ? g4[i][(e + 2) & 3] : g4[i][3]));
                                if ((int)pd0[i] + e < seg) tile[lds_of((int)ppt[i], (int)pd0[i] + e)] = x;
                            }
                        }
                    }
                }
                const bool last = kt + 1 == kt1;
                if (AHEAD) fetch_g(g4n, last ? (more ? tn : t) : t, last ? kt0 : kt + 1);
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const gen_f32x4 v = *reinterpret_cast<const gen_f32x4 *>(tile + r * GEN_RS + (q / QPG) * CPAD + 8 * (q % QPG) + 4 * h);
#pragma unroll
                    for (int e = 0; e < 4; ++e) gv[4 * q + e] = v[e];
                }
            }
            gen_f32x16 acc;
#pragma unroll
            for (int q = 0; q < 4; ++q) {    // result rows 8 q + 4 half + (0..3)
                const gen_f32x4 v = *reinterpret_cast<const gen_f32x4 *>(Bt + (kt - kt0) * 32 + 8 * q + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[4 * q + e] = v[e];
            }
            // the weight fragments of 4 K steps per 16-byte read, the next group's read in flight under this group's MFMAs
            // (a K step past C inside the last group multiplies zeros)
            const gen_f32x4 *af = reinterpret_cast<const gen_f32x4 *>(Af + (size_t)(kt - kt0) * ng * 256) + lane;
            gen_f32x4 a4 = af[0];
#pragma unroll
            for (int g = 0; g < KSMAX / 4; ++g) {
                if (g < ng) {
                    gen_f32x4 nx = a4;
                    if (g + 1 < KSMAX / 4 && g + 1 < ng) nx = af[(g + 1) * 64];
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], (ok && 2 * (4 * g + e) + h < c) ? bf[4 * g + e] : 0.f, acc, 0, 0, 0);
                    a4 = nx;
                }
            }
            // clamp in place; a value is inside the clamp iff the clamp left it alone
            float sum[NG], rden[NG], dot[NG];
            unsigned inside = 0;
#pragma unroll
            for (int g = 0; g < NG; ++g) sum[g] = dot[g] = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (8 * (q % QPG) < c) {     // (wave-uniform: 8-row blocks past C hold padding)
                    const int o0 = 8 * (q % QPG) + 4 * h;
                    float part4 = 0.f;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float a = acc[4 * q + e], cl = fminf(fmaxf(a, 1e-5f), 1.f - 1e-5f);   // positive
                        if (BACKWARD) inside |= (a == cl ? 1u : 0u) << (4 * q + e);
                        acc[4 * q + e] = cl;
                        part4 += (!TAILS || o0 + e < c) ? cl : 0.f;
                    }
                    sum[q / QPG] += (TAILS || o0 < c) ? part4 : 0.f;
                }
            }
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                sum[g] += __shfl_xor(sum[g], 32);                      // the rows of the other half
                rden[g] = 1.f / fmaxf(sum[g], 1e-12f);
            }
            if (BACKWARD) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (8 * (q % QPG) < c) {
                        const int kk = kt * NG + q / QPG, o0 = 8 * (q % QPG) + 4 * h;
                        float part4 = 0.f;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            gv[4 * q + e] = (kk < c && o0 + e < c) ? gv[4 * q + e] : 0.f;   // padding carries no gradient
                            part4 += gv[4 * q + e] * (acc[4 * q + e] * rden[q / QPG]);
                        }
                        dot[q / QPG] += part4;
                    }
                }
#pragma unroll
                for (int g = 0; g < NG; ++g) dot[g] += __shfl_xor(dot[g], 32);
            }
            // results -> tile (the gradient reads above are done: LDS serves a wave in order)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int g = q / QPG;
                if (8 * (q % QPG) < c) {
                    gen_f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (!BACKWARD) v[e] = acc[4 * q + e] * rden[g];
                        else v[e] = ((inside >> (4 * q + e)) & 1u) ? (gv[4 * q + e] - dot[g]) * rden[g] : 0.f;
                    }
                    *reinterpret_cast<gen_f32x4 *>(tile + r * GEN_RS + g * CPAD + 8 * (q % QPG) + 4 * h) = v;
                }
            }
            __builtin_amdgcn_wave_barrier();
            // tile -> the output, in the output's order
#pragma unroll
            for (int i = 0; i < GEN_NI; ++i) {
                if ((int)ppt[i] < npts && (int)pd0[i] < segk) {
                    float *dst = out + (kbase + ppt[i] * (unsigned)cc + pd0[i]);
                    if (!TAILS) *reinterpret_cast<gen_f32x4u *>(dst) = *reinterpret_cast<const gen_f32x4 *>(tile + plo[i]);
                    else {
                        gen_f32x4u v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = tile[lds_of((int)ppt[i], min((int)pd0[i] + e, seg - 1))];
                        if ((int)pd0[i] + 4 <= segk) *reinterpret_cast<gen_f32x4u *>(dst) = v;
                        else {
#pragma unroll
                            for (int e = 0; e < 3; ++e)
                                if ((int)pd0[i] + e < segk) dst[e] = v[e];
                        }
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            if (AHEAD) {
#pragma unroll
                for (int i = 0; i < GEN_NI; ++i) g4[i] = g4n[i];
            }
        }
        if (!more) break;
        t = tn;
        ok = okn;
        if (BACKWARD) fetch_p(bf, pbasen);
        else {
#pragma unroll
            for (int s = 0; s < KSMAX; ++s) bf[s] = bfn[s];
        }
    }
}

// ---- logit correction (train.py:549-552) --------------------------------------------------------------------
// v = lam*E + (1-lam)*T_i;  tn = v / max(sum_c |v|, eps);  out[c] = sum_r logit[r] * tn[r][c]
__global__ __launch_bounds__(256) void gen_correct_fwd_kernel(int total_pts, int n, int c, float lam,
                                                              const float *__restrict__ logits,
                                                              const float *__restrict__ insT, const float *__restrict__ E,
                                                              float *__restrict__ out)
{
    const int cc = c * c;
    const int lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < total_pts; i += gridDim.x * 4) {
        const int b = i / n, ni = i - b * n;
        float acc = 0.f;
        for (int r0 = 0; r0 < c; r0 += 2) {
            const int r = r0 + h;
            const bool live = col < c && r < c;
            const float v = live ? lam * E[r * c + col] + (1.f - lam) * insT[(size_t)i * cc + r * c + col] : 0.f;
            const float s = half_sum(fabsf(v));
            const float l = r < c ? logits[((size_t)b * c + r) * n + ni] : 0.f;
            acc = fmaf(l / fmaxf(s, 1e-12f), v, acc);
        }
        acc += __shfl_xor(acc, 32);     // even rows + odd rows
        if (lane < c) out[((size_t)b * c + lane) * n + ni] = acc;
    }
}

// Backward: grad_logits[r] = sum_c tn[r][c] go[c];  d v = (l go - sign(v) l gl) / den;  grad_T = (1-lam) d v;
// grad_E += lam * sum_points d v -- accumulated per wave in its own LDS copy (plain read-modify-write: a lane
// always meets the same address), folded into grad_E with one atomic per entry and workgroup.
__global__ __launch_bounds__(256) void gen_correct_bwd_kernel(int total_pts, int n, int c, float lam,
                                                              const float *__restrict__ logits,
                                                              const float *__restrict__ insT, const float *__restrict__ E,
                                                              const float *__restrict__ grad_out,
                                                              float *__restrict__ grad_logits, float *__restrict__ grad_insT,
                                                              float *__restrict__ grad_E)
{
    extern __shared__ float gen_lds[];
    const int cc = c * c;
    float *eacc = gen_lds + (threadIdx.x >> 6) * cc;      // [4 waves][cc]
    for (int e = threadIdx.x; e < 4 * cc; e += 256) gen_lds[e] = 0.f;
    __syncthreads();
    const int lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < total_pts; i += gridDim.x * 4) {
        const int b = i / n, ni = i - b * n;
        const float go = col < c ? grad_out[((size_t)b * c + col) * n + ni] : 0.f;
        for (int r0 = 0; r0 < c; r0 += 2) {
            const int r = r0 + h;
            const bool live = col < c && r < c;
            const float v = live ? lam * E[r * c + col] + (1.f - lam) * insT[(size_t)i * cc + r * c + col] : 0.f;
            const float s = half_sum(fabsf(v));
            const float rden = 1.f / fmaxf(s, 1e-12f);
            const float l = r < c ? logits[((size_t)b * c + r) * n + ni] : 0.f;
            const float gl = half_sum((v * rden) * go);
            if (col == 0 && r < c) grad_logits[((size_t)b * c + r) * n + ni] = gl;
            const float sg = v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f);
            const float dv = s > 1e-12f ? (l * go - sg * (l * gl)) * rden : l * go * rden;
            if (live) {
                grad_insT[(size_t)i * cc + r * c + col] = (1.f - lam) * dv;
                eacc[r * c + col] += lam * dv;
            }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < cc; e += 256)
        atomicAdd(grad_E + e, (gen_lds[e] + gen_lds[cc + e]) + (gen_lds[2 * cc + e] + gen_lds[3 * cc + e]));
}

// ---- the launch plan ---------------------------------------------------------------------------------------------------
// Every launch decision of gen_sig_t_mean and of the two gen_correct_* launches, in one place: the launchers below and the
// host-only query geot_ntm_generic_plan (ntm.hip) both read it, so the query cannot drift from what runs.
int gen_blocks(long long total_pts)
{
    long long blocks = (total_pts + 3) / 4;
    return (int)(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks));   // 8 workgroups per CU, grid-stride beyond
}

static inline int gen_cpad(int c) { return c <= 8 ? 8 : (c <= 16 ? 16 : 32); }

// the lane-per-point form: CP = C rounded up to 8, 256 points per workgroup, 8 workgroups per CU and grid-stride beyond
static GenSigPlan plan_sig_rows(long long total_pts, int c, long long cus)
{
    GenSigPlan pl = {GEN_FORM_ROWS, (c + 7) / 8 * 8, 0, 1, 0, 0};
    pl.lds = (size_t)(((c * c + 3) & ~3) + 4 * 64 * (pl.cp + 1)) * sizeof(float);    // <= 38 KB
    pl.blocks = (total_pts + 255) / 256;
    const long long cap = 8LL * cus;
    if (pl.blocks > cap) pl.blocks = cap;
    return pl;
}

// the matrix-core form; form GEN_FORM_REFUSED where no split fits (fewer CUs than ranges)
static GenSigPlan plan_sig_mfma(long long total_pts, int c, long long cus)
{
    GenSigPlan pl = {GEN_FORM_MFMA, gen_cpad(c), (c & 3) != 0 ? 1 : 0, 1, 0, 0};
    const int NG = 32 / pl.cp;
    const int nkt = (c + NG - 1) / NG, ng = (c + 7) / 8;
    const long long tiles = (total_pts + 31) / 32;
    // ranges of row tiles (a workgroup stages the weights of one): the fewest whose weights fit beside the 16 waves' tiles and
    // that leave the last round of a range's waves >= 85 % full (one workgroup per CU: 88+ registers x 1024 threads)
    auto lds_of = [&](int ks) {
        const int per = (nkt + ks - 1) / ks;
        return ((size_t)per * ng * 256 + (size_t)per * 32 + (size_t)GEN_MW * 32 * GEN_RS) * sizeof(float);
    };
    int ksplit = 1;
    for (; ksplit < nkt; ++ksplit) {
        if (lds_of(ksplit) > 160 * 1024) continue;
        const long long waves = cus / ksplit * GEN_MW, rounds = (tiles + waves - 1) / (waves > 0 ? waves : 1);
        if (waves > 0 && (tiles <= waves || tiles * 100 >= rounds * waves * 85 || ksplit >= 4)) break;
    }
    pl.ksplit = ksplit;
    pl.lds = lds_of(ksplit);
    if (pl.lds > 160 * 1024 || cus < ksplit) {
        pl.form = GEN_FORM_REFUSED;
        return pl;
    }
    long long nb = cus / ksplit;             // workgroups per range
    if (nb > (tiles + GEN_MW - 1) / GEN_MW) nb = (tiles + GEN_MW - 1) / GEN_MW;
    pl.blocks = nb * ksplit;
    return pl;
}

// the wave-per-point form: persistent workgroups, as many per CU as the staged weights ((C+1) C^2 floats each) leave room
// for in LDS: the inner loop is a chain of LDS reads, it needs waves to hide behind (2 per SIMD measured 0.23 TB/s at C = 16)
static GenSigPlan plan_sig_wave(long long total_pts, int c, long long cus)
{
    GenSigPlan pl = {GEN_FORM_WAVE, 0, 0, 1, 0, 0};
    pl.lds = (size_t)(c + 1) * c * c * sizeof(float);        // 135 KB at C = 32
    pl.blocks = (total_pts + 3) / 4;
    long long per_cu = (160 * 1024) / (long long)(pl.lds + 512);
    per_cu = per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu);
    const long long cap = per_cu * cus;
    if (pl.blocks > cap) pl.blocks = cap;
    return pl;
}

GenSigPlan gen_sig_plan(int b, int n, int c, int cus)
{
    const long long total_pts = (long long)b * n, elems = total_pts * c * c;
    if (total_pts <= 0 || c < 1 || c > GEN_MAXC) return GenSigPlan{GEN_FORM_NONE, 0, 0, 0, 0, 0};
    if (cus <= 0) cus = device_cus();
    const char *impl = getenv("GEOT_NTM_GENERIC");      // A/B tests: "mfma" / "rows" = the lane-per-point kernel / "wave" = the wave-per-point kernel
    const bool small = elems < 0x7fffffffLL * 4LL;
    // the MFMA form from C = 6 up (kernel times at 8 x 24000 points, C = 5: 18 / 32 us against the lane-per-point form's
    // 17 / 30; C = 7: 20 / 41 against 33 / 64 -- profiles/r05_ntm_generic.txt)
    const bool want_mfma = impl && impl[0] == 'm' ? true : (impl && (impl[0] == 'r' || impl[0] == 'w') ? false : c >= 6);
    // (the kernel clamps its gradient loads to the buffer's last four elements: it needs four)
    if (want_mfma && elems < (1LL << 30) && elems >= 4) return plan_sig_mfma(total_pts, c, cus);
    if (!(impl && impl[0] == 'w') && small) return plan_sig_rows(total_pts, c, cus);
    return plan_sig_wave(total_pts, c, cus);
}

template <int CP>
static hipError_t launch_sig_rows(const GenSigPlan &pl, bool backward, int b, int n, int c, const float *p, const float *W,
                                  const float *cm, const float *grad_out, float *out, hipStream_t s)
{
    if (backward)
        hipLaunchKernelGGL((gen_sig_t_mean_rows_kernel<CP, true>), dim3((int)pl.blocks), dim3(256), pl.lds, s, b * n, n, c, p, W, cm,
                           grad_out, out);
    else
        hipLaunchKernelGGL((gen_sig_t_mean_rows_kernel<CP, false>), dim3((int)pl.blocks), dim3(256), pl.lds, s, b * n, n, c, p, W, cm,
                           grad_out, out);
    return hipGetLastError();
}

template <int CPAD>
static hipError_t launch_sig_mfma(const GenSigPlan &pl, bool backward, int b, int n, int c, const float *p, const float *W,
                                  const float *cm, const float *grad_out, float *out, hipStream_t s)
{
    const bool tails = pl.tails != 0;
    const void *fn = backward ? (tails ? (const void *)gen_sig_t_mean_mfma_kernel<CPAD, true, true> : (const void *)gen_sig_t_mean_mfma_kernel<CPAD, true, false>)
                              : (tails ? (const void *)gen_sig_t_mean_mfma_kernel<CPAD, false, true> : (const void *)gen_sig_t_mean_mfma_kernel<CPAD, false, false>);
    hipError_t e = allow_big_lds(fn, pl.lds);
    if (e != hipSuccess) return e;
    const int ksplit = pl.ksplit;
#define GEOT_GEN_SIG(BW, TL)                                                                                                   \
    hipLaunchKernelGGL((gen_sig_t_mean_mfma_kernel<CPAD, BW, TL>), dim3((int)pl.blocks), dim3(GEN_MT), pl.lds, s, b * n, n, c, ksplit, p, W, \
                       cm, grad_out, out)
    if (backward) { if (tails) GEOT_GEN_SIG(true, true); else GEOT_GEN_SIG(true, false); }
    else { if (tails) GEOT_GEN_SIG(false, true); else GEOT_GEN_SIG(false, false); }
#undef GEOT_GEN_SIG
    return hipGetLastError();
}

hipError_t gen_sig_t_mean(bool backward, int b, int n, int c, const float *p, const float *W, const float *cm,
                          const float *grad_out, float *out, hipStream_t s)
{
    const GenSigPlan pl = gen_sig_plan(b, n, c, 0);
    if (pl.form == GEN_FORM_NONE) return hipSuccess;
    if (pl.form == GEN_FORM_REFUSED) return hipErrorInvalidValue;
    if (pl.form == GEN_FORM_MFMA) {
        if (pl.cp == 8) return launch_sig_mfma<8>(pl, backward, b, n, c, p, W, cm, grad_out, out, s);
        if (pl.cp == 16) return launch_sig_mfma<16>(pl, backward, b, n, c, p, W, cm, grad_out, out, s);
        return launch_sig_mfma<32>(pl, backward, b, n, c, p, W, cm, grad_out, out, s);
    }
    if (pl.form == GEN_FORM_ROWS) {
        if (pl.cp == 8) return launch_sig_rows<8>(pl, backward, b, n, c, p, W, cm, grad_out, out, s);
        if (pl.cp == 16) return launch_sig_rows<16>(pl, backward, b, n, c, p, W, cm, grad_out, out, s);
        if (pl.cp == 24) return launch_sig_rows<24>(pl, backward, b, n, c, p, W, cm, grad_out, out, s);
        return launch_sig_rows<32>(pl, backward, b, n, c, p, W, cm, grad_out, out, s);
    }
    const void *fn = backward ? (const void *)gen_sig_t_mean_kernel<true> : (const void *)gen_sig_t_mean_kernel<false>;
    hipError_t e = allow_big_lds(fn, pl.lds);
    if (e != hipSuccess) return e;
    if (backward)
        hipLaunchKernelGGL(gen_sig_t_mean_kernel<true>, dim3((int)pl.blocks), dim3(256), pl.lds, s, b * n, n, c, p, W, cm, grad_out, out);
    else
        hipLaunchKernelGGL(gen_sig_t_mean_kernel<false>, dim3((int)pl.blocks), dim3(256), pl.lds, s, b * n, n, c, p, W, cm, grad_out, out);
    return hipGetLastError();
}

hipError_t gen_correct_fwd(int b, int n, int c, float lam, const float *logits, const float *insT, const float *E,
                           float *out, hipStream_t s)
{
    hipLaunchKernelGGL(gen_correct_fwd_kernel, dim3(gen_blocks((long long)b * n)), dim3(256), 0, s, b * n, n, c, lam, logits,
                       insT, E, out);
    return hipGetLastError();
}

hipError_t gen_correct_bwd(int b, int n, int c, float lam, const float *logits, const float *insT, const float *E,
                           const float *grad_out, float *grad_logits, float *grad_insT, float *grad_E, hipStream_t s)
{
    hipLaunchKernelGGL(gen_correct_bwd_kernel, dim3(gen_blocks((long long)b * n)), dim3(256), (size_t)4 * c * c * sizeof(float), s,
                       b * n, n, c, lam, logits, insT, E, grad_out, grad_logits, grad_insT, grad_E);
    return hipGetLastError();
}

} // namespace geot
