// The draws of geot_view_draw (view_draw.hip): record layouts, the plan test and every drawn quantity as a host / device
// function, so that the same text runs in the kernel, in the entry point and in a host program.  Contract: include/geot_hip.h.
//
// Arithmetic.  Every statement is ONE correctly rounded fp32 operation -- add, subtract, multiply, divide, square root --
// written as a plain operator: the library is compiled with -ffp-contract=off (build.py), so nothing is fused, and a host
// compiler without -ffast-math does the same.  No math-library function is called: the logarithm is the integer exponent
// plus a polynomial on the mantissa, sine and cosine are an exact quadrant reduction of a fraction of a turn plus two
// polynomials on [-pi/4, pi/4] (an octant either side of the axis).  tests/_view_draw_ref.py restates all of it in numpy
// float32 and the results agree bit for bit.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "geot_hip.h"
#include "philox.h"

namespace geot {

// ---- record layouts.  VdJob is the job record of geot_view_program (view_program.hip VpJob; that file is not included
// here because it holds the kernel), the kinds are its VpKind values.
enum VdOpKind {
    VDO_SCALE = 1, VDO_TRANSLATE = 4, VDO_SCALE_TRANSLATE = 5, VDO_JITTER = 6, VDO_SCALE_JITTER = 7, VDO_ROTATE = 8, VDO_FLIP = 9,
    VDO_ZERO = 10, VDO_MASK = 11, VDO_STORE_X = 12
};
struct VdOp {
    int kind, arg;
    float f[12];
};
struct VdJob {
    int src_row, out_row, n_ops, noise_row, mask_row, reserved[3];
    VdOp op[GEOT_VIEW_MAX_OPS];
};
static_assert(sizeof(VdJob) == GEOT_VIEW_PROGRAM_JOB_WORDS * 4, "job record layout");

enum VdStepKind { VD_SCALE = 1, VD_SHIFT = 2, VD_NOISE = 3, VD_ROTATE = 4, VD_FLIP = 5, VD_DROP = 6, VD_PERMASK = 7, VD_KINDS = 8 };
// the quantity byte of the tag word: one Philox call per (step, quantity[, element]), its four words used in order
enum VdQuantity { VQ_SCALE = 0, VQ_MIRROR = 1, VQ_SHIFT = 2, VQ_ROTATE = 3, VQ_FLIP = 4, VQ_DROP = 5, VQ_NOISE = 6, VQ_PERMASK = 7 };
struct VdStep {
    int kind, op, pos, flags;
    float c[8];
};
struct VdPlan {          // GEOT_VIEW_DRAW_PLAN_WORDS words
    int view, slot, n_steps, store_op, reserved[4];
    VdStep step[GEOT_VIEW_DRAW_MAX_STEPS];
};
static_assert(sizeof(VdPlan) == GEOT_VIEW_DRAW_PLAN_WORDS * 4, "plan record layout");

constexpr int VD_MAX_POS = 4096;
constexpr float VD_MAX_ANGLE = 1024.f;   // |turns| stays far below 2^22, where the reduction is exact

// second counter word: bit 30 set and bit 31 clear, so it is none of geot_sample_draw's (0..7, 0xFFFFFFFF)
GEOT_HD uint32_t vd_tag(int view, int pos, int quantity)
{
    return 0x40000000u | ((uint32_t)view << 24) | ((uint32_t)pos << 8) | (uint32_t)quantity;
}

// a step's op of the template, or nullptr: index in range and kind one of (a, b, c)
GEOT_HD const VdOp *vd_op(const VdJob &t, int op, int a, int b = 0, int c = 0)
{
    if (op < 0 || op >= t.n_ops) return nullptr;
    const int k = t.op[op].kind;
    return (k == a || k == b || k == c) && k != 0 ? &t.op[op] : nullptr;
}

GEOT_HD bool vd_finite_in(float v, float lo, float hi) { return v >= lo && v <= hi; }     // false for NaN

// is this (template, plan) pair safe to draw?  The same test on the host (the entry point) and in the kernel.
GEOT_HD bool vd_plan_ok(const VdPlan &p, const VdJob &t, int n_noise, int n_mask)
{
    if (t.n_ops < 0 || t.n_ops > GEOT_VIEW_MAX_OPS) return false;
    if (p.view < 0 || p.view > 2 || p.slot < 0 || p.n_steps < 0 || p.n_steps > GEOT_VIEW_DRAW_MAX_STEPS) return false;
    if (p.store_op != -1 && !vd_op(t, p.store_op, VDO_STORE_X)) return false;
    for (int s = 0; s < p.n_steps; ++s) {
        const VdStep &st = p.step[s];
        if (st.kind < 1 || st.kind >= VD_KINDS || st.pos < 0 || st.pos >= VD_MAX_POS || st.flags < 0) return false;
        if (st.kind == VD_SCALE) {
            if (!vd_op(t, st.op, VDO_SCALE, VDO_SCALE_TRANSLATE, VDO_SCALE_JITTER) || ((st.flags >> 4) & 3) > 2) return false;
        } else if (st.kind == VD_SHIFT) {
            if (!vd_op(t, st.op, VDO_TRANSLATE, VDO_SCALE_TRANSLATE)) return false;
        } else if (st.kind == VD_NOISE) {
            const VdOp *o = vd_op(t, st.op, VDO_JITTER, VDO_SCALE_JITTER);
            if (!o || o->arg < 0 || t.noise_row < 0 || (long long)t.noise_row + o->arg >= n_noise) return false;
        } else if (st.kind == VD_ROTATE) {
            if (!vd_op(t, st.op, VDO_ROTATE)) return false;
            for (int k = 0; k < 3; ++k)
                if (!vd_finite_in(st.c[k], -VD_MAX_ANGLE, VD_MAX_ANGLE)) return false;
        } else if (st.kind == VD_FLIP) {
            const VdOp *a = vd_op(t, st.op, VDO_FLIP), *b = vd_op(t, st.op + 1, VDO_FLIP);
            if (!a || !b || a->arg < 0 || a->arg > 2 || b->arg < 0 || b->arg > 2) return false;
        } else if (st.kind == VD_DROP) {
            if (st.op == -1 ? p.store_op == -1 : !vd_op(t, st.op, VDO_ZERO)) return false;
        } else {                                             // VD_PERMASK: a MASK op's row, or the row of the STORE_X op
            int row;
            if (st.op == -1) {
                if (p.store_op == -1 || (t.op[p.store_op].arg & 3) != 2) return false;
                row = t.op[p.store_op].arg >> 2;
            } else {
                const VdOp *o = vd_op(t, st.op, VDO_MASK);
                if (!o) return false;
                row = o->arg;
            }
            if (row < 0 || t.mask_row < 0 || (long long)t.mask_row + row >= n_mask) return false;
        }
    }
    return true;
}

// the mask row (of the job) a PERMASK step multiplies into; the plan has passed vd_plan_ok
GEOT_HD int vd_mask_row(const VdPlan &p, const VdJob &t, const VdStep &st)
{
    return st.op == -1 ? t.op[p.store_op].arg >> 2 : t.op[st.op].arg;
}

// ---- uniforms
GEOT_HD float vd_uniform(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }             // [0, 1), exact
GEOT_HD float vd_uniform_open(uint32_t w) { return (float)((w >> 8) + 1u) * 0x1p-24f; }  // (0, 1], exact

// ---- ln(n 2^-24) for n in [1, 2^24]: n = 2^e f, f in [1, 2) exactly; f above sqrt(2) is halved; with s = (f - 1) / (f + 1),
// |s| <= 0.1716, ln f = 2 atanh s = 2 (s + s (w / 3 + w^2 / 5 + ... + w^5 / 11)), w = s^2 (the next term is below 2e-11)
GEOT_HD float vd_log_u24(uint32_t n)
{
    if (n >= (1u << 24)) return 0.f;
    int e = 31 - __builtin_clz(n);
    union {
        uint32_t u;
        float f;
    } bits;
    bits.u = 0x3F800000u | ((n << (23 - e)) & 0x7FFFFFu);
    float f = bits.f;
    if (f > 1.41421354f) {
        f = f * 0.5f;
        e += 1;
    }
    const float s = (f - 1.f) / (f + 1.f);
    const float w = s * s;
    float p = w * 0.0909090936f + 0.111111112f;
    p = w * p + 0.142857149f;
    p = w * p + 0.200000003f;
    p = w * p + 0.333333343f;
    p = w * p;
    const float lnf = (s + s * p) * 2.f;
    return (float)(e - 24) * 0.693147182f + lnf;
}

// the Box-Muller radius sqrt(-2 ln u1), u1 = ((w >> 8) + 1) 2^-24 in (0, 1]: at most 5.7682.  (0 - ln) * 2, not ln * -2:
// u1 = 1 then gives +0, not the square root of -0
GEOT_HD float vd_radius(uint32_t w) { return __builtin_sqrtf((0.f - vd_log_u24((w >> 8) + 1u)) * 2.f); }

// ---- cos and sin of t turns, |t| <= 2^20.  y = 4 t (exact); n = the nearest integer, by adding and taking off 1.5 2^23;
// r = y - n exactly, |r| <= 1/2; a = r pi / 2 in [-pi/4, pi/4]; Taylor polynomials to a^9 / a^10 (next terms below 2e-9);
// the quadrant n mod 4 swaps and negates.  A negation is 0 - v, so t = 0 gives (1, +0) and a quarter turn (+0, 1).
GEOT_HD void vd_sincos_turns(float t, float &c, float &s)
{
    const float y = t * 4.f;
    const float n = (y + 12582912.f) - 12582912.f;
    const float r = y - n;
    const int q = (int)n & 3;
    const float a = r * 1.57079637f;
    const float w = a * a;
    float ps = w * 2.75573188e-06f + -0.000198412701f;
    ps = w * ps + 0.00833333377f;
    ps = w * ps + -0.166666672f;
    ps = w * ps;
    const float sn = a + a * ps;
    float pc = w * -2.75573188e-07f + 2.48015876e-05f;
    pc = w * pc + -0.00138888892f;
    pc = w * pc + 0.0416666679f;
    pc = w * pc + -0.5f;
    const float cs = w * pc + 1.f;
    c = q == 0 ? cs : (q == 1 ? 0.f - sn : (q == 2 ? 0.f - cs : sn));
    s = q == 0 ? sn : (q == 1 ? cs : (q == 2 ? 0.f - sn : 0.f - cs));
}

// ---- per-point quantities.  Three normals of one point from ONE Philox call: (w0, w1) give two, (w2, w3) the third.
GEOT_HD void vd_noise3(const Philox4 &p, float std_, float clip, float (&out)[3])
{
    float c0, s0, c1, s1;
    vd_sincos_turns(vd_uniform(p.w[1]), c0, s0);
    vd_sincos_turns(vd_uniform(p.w[3]), c1, s1);
    const float r0 = vd_radius(p.w[0]), r1 = vd_radius(p.w[2]);
    const float z[3] = {r0 * c0, r0 * s0, r1 * c1};
    const float lo = 0.f - clip;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float v = z[k] * std_;
        v = v < lo ? lo : v;
        out[k] = v > clip ? clip : v;
    }
}

// ---- scalar quantities
// PointCloudScaling / ScaleAndTranslate / ScaleAndJitter._draw_scale.  flags: bit 0 anisotropic, bits 1-3 scale_xyz,
// bits 4-5 mirror form (0 none, 1 `(u > mirror) * 2 - 1`, 2 `round(u) * 2 - 1` weighted: m * mirror + (1 - mirror)).
// c[0] = lo, c[1] = hi - lo, c[2..4] = mirror
GEOT_HD void vd_scale(const VdStep &st, const Philox4 &ps, const Philox4 &pm, float (&out)[3])
{
    const bool aniso = st.flags & 1;
    const int form = (st.flags >> 4) & 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float v = vd_uniform(ps.w[aniso ? k : 0]) * st.c[1] + st.c[0];
        if (form) {
            const float u = vd_uniform(pm.w[k]), mk = st.c[2 + k];
            float mir;
            if (form == 1) mir = u > mk ? 1.f : -1.f;
            else mir = (u > 0.5f ? 1.f : -1.f) * mk + (1.f - mk);
            v = v * mir;
        }
        // anisotropic=False draws ONE value; scale[0] = 1 on it (scale_xyz[0] unset) sets all three
        out[k] = ((st.flags >> (1 + (aniso ? k : 0))) & 1) ? v : 1.f;
    }
}

// PointCloudTranslation: u * shift; PointCloudScaleAndTranslate (flags bit 0): (u - 0.5) * 2 * shift.  c[0..2] = shift
GEOT_HD void vd_shift(const VdStep &st, const Philox4 &p, float (&out)[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float u = vd_uniform(p.w[k]);
        out[k] = (st.flags & 1) ? ((u - 0.5f) * 2.f) * st.c[k] : u * st.c[k];
    }
}

// PointCloudRotation: per axis t = angle (2u - 1) / 2 turns (angle in units of pi: theta = angle pi (2u - 1)), the axis
// rotation matrices in the order perm[(w3 >> 8) * 6 >> 24], R = (A B) C, every entry (a0 b0 + a1 b1) + a2 b2
GEOT_HD void vd_matmul(const float (&a)[9], const float (&b)[9], float (&o)[9])
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}

GEOT_HD void vd_rotation(const VdStep &st, const Philox4 &p, float (&R)[9])
{
    float mat[3][9];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const float v = vd_uniform(p.w[ax]) * 2.f - 1.f;
        float c, s;
        vd_sincos_turns((st.c[ax] * v) * 0.5f, c, s);
        const float ns = 0.f - s;
        float(&mm)[9] = mat[ax];
#pragma unroll
        for (int k = 0; k < 9; ++k) mm[k] = (k % 4 == 0) ? 1.f : 0.f;
        if (ax == 0) mm[4] = c, mm[5] = ns, mm[7] = s, mm[8] = c;
        else if (ax == 1) mm[0] = c, mm[2] = s, mm[6] = ns, mm[8] = c;
        else mm[0] = c, mm[1] = ns, mm[3] = s, mm[4] = c;
    }
    const uint32_t o = ((p.w[3] >> 8) * 6u) >> 24;                   // 0..5
    const int first = (int)(o >> 1), rest = (int)(o & 1u);
    const int second = rest ? (first == 2 ? 1 : 2) : (first == 0 ? 1 : 0);     // the six orders, lexicographic
    const int third = 3 - first - second;
    // (the three factors by selection, element by element: a run-time index would put the matrices in scratch)
    float a[9], b[9], c[9], ab[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        a[k] = first == 0 ? mat[0][k] : (first == 1 ? mat[1][k] : mat[2][k]);
        b[k] = second == 0 ? mat[0][k] : (second == 1 ? mat[1][k] : mat[2][k]);
        c[k] = third == 0 ? mat[0][k] : (third == 1 ? mat[1][k] : mat[2][k]);
    }
    vd_matmul(a, b, ab);
    vd_matmul(ab, c, R);
}

// ---- a job: its scalars into the record, its points into the rows
struct VdKey {
    uint32_t d_lo, d_hi, k0, k1;
    int view;
};

GEOT_HD Philox4 vd_philox(const VdKey &k, uint32_t element, int pos, int quantity)
{
    return philox4x32_10(element, vd_tag(k.view, pos, quantity), k.d_lo, k.d_hi, k.k0, k.k1);
}

GEOT_HD void vd_unit_scale(VdOp &op)
{
    op.kind = VDO_SCALE;
    op.arg = 0;
    op.f[0] = op.f[1] = op.f[2] = 1.f;
}

// one step's scalars into the job's record (the template has been copied there)
GEOT_HD void vd_draw_step(const VdPlan &pl, const VdStep &st, const VdKey &key, VdJob &job)
{
    if (st.kind == VD_SCALE) {
        float v[3];
        vd_scale(st, vd_philox(key, 0u, st.pos, VQ_SCALE), vd_philox(key, 0u, st.pos, VQ_MIRROR), v);
        VdOp &op = job.op[st.op];
        op.f[0] = v[0], op.f[1] = v[1], op.f[2] = v[2];
    } else if (st.kind == VD_SHIFT) {
        float v[3];
        vd_shift(st, vd_philox(key, 0u, st.pos, VQ_SHIFT), v);
        VdOp &op = job.op[st.op];
        const int at = op.kind == VDO_SCALE_TRANSLATE ? 3 : 0;
        op.f[at] = v[0], op.f[at + 1] = v[1], op.f[at + 2] = v[2];
    } else if (st.kind == VD_ROTATE) {
        float R[9];
        vd_rotation(st, vd_philox(key, 0u, st.pos, VQ_ROTATE), R);
        VdOp &op = job.op[st.op];
#pragma unroll
        for (int k = 0; k < 9; ++k) op.f[k] = R[k];
    } else if (st.kind == VD_FLIP) {
        // random() < aug_prob, then random() < 0.5 per horizontal axis (all three are drawn: a counter costs nothing)
        const Philox4 p = vd_philox(key, 0u, st.pos, VQ_FLIP);
        const bool any = vd_uniform(p.w[0]) < st.c[0];
        if (!(any && vd_uniform(p.w[1]) < 0.5f)) vd_unit_scale(job.op[st.op]);
        if (!(any && vd_uniform(p.w[2]) < 0.5f)) vd_unit_scale(job.op[st.op + 1]);
    } else if (st.kind == VD_DROP) {
        const bool drop = vd_uniform(vd_philox(key, 0u, st.pos, VQ_DROP).w[0]) < st.c[0];
        if (st.op == -1) {
            if (drop) job.op[pl.store_op].arg = 1;       // x = 0, whatever else the list does to x (several steps: same value)
        } else if (!drop) {
            vd_unit_scale(job.op[st.op]);
        }
    }
}

// point i of every noise and mask row of the job (the plan has passed vd_plan_ok)
GEOT_HD void vd_draw_point(const VdPlan &pl, const VdJob &tj, const VdKey &key, uint32_t i, int m, float *noise, float *mask)
{
    for (int s = 0; s < pl.n_steps; ++s) {
        const VdStep &st = pl.step[s];
        if (st.kind == VD_NOISE) {
            float v[3];
            vd_noise3(vd_philox(key, i, st.pos, VQ_NOISE), st.c[0], st.c[1], v);
            float *row = noise + ((size_t)(tj.noise_row + tj.op[st.op].arg) * m + i) * 3;
            row[0] = v[0], row[1] = v[1], row[2] = v[2];
        } else if (st.kind == VD_PERMASK) {
            // the row is the product of every PERMASK step that names it; the first of them writes it
            const int row = vd_mask_row(pl, tj, st);
            bool first = true;
            for (int e = 0; e < s; ++e) first = first && !(pl.step[e].kind == VD_PERMASK && vd_mask_row(pl, tj, pl.step[e]) == row);
            if (!first) continue;
            float keep = 1.f;
            for (int e = s; e < pl.n_steps; ++e) {
                const VdStep &se = pl.step[e];
                if (se.kind != VD_PERMASK || vd_mask_row(pl, tj, se) != row) continue;
                keep = keep * (vd_uniform(vd_philox(key, i, se.pos, VQ_PERMASK).w[0]) > se.c[0] ? 1.f : 0.f);
            }
            mask[(size_t)(tj.mask_row + row) * m + i] = keep;
        }
    }
}

} // namespace geot
