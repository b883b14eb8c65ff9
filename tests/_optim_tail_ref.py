"""fp64 numpy restatement of the fused tail of an iteration (include/geot_hip.h "ABI 25", geot_amd/optim_tail.py): the gradient
clip of torch.nn.utils.clip_grad_norm_ (norm_type 2, error_if_nonfinite=False), torch.optim.AdamW's step and the teacher's
exponential moving average, written from their definitions: nothing of geot_amd is imported.

    tail(records, groups, max_norm, decay, drop=(), u=U, chain=ANY_CHAIN)
        records: list of dicts -- kind "adamw": p, g, m, v (arrays), step (the count BEFORE the call), group, clipped, t or
        None; kind "ema": p, t; kind "int": p, t.  groups: list of dicts lr, betas, eps, weight_decay.
        -> (list of result dicts with the new p, m, v, t, step and the absolute bounds E_p, E_m, E_v, E_t, total_norm, coef)
    drop: terms left out, for the test that the bounds are not vacuous: "wd", "bc1", "bc2", "eps", "clip", "ema".
    norm: the gradient norm, when the records hold a sample of the elements only (computed in fp64 from all of them).

Error bounds.  u = 2^-24 (fp32 unit roundoff), first order in u; every term is a count of roundings of an implementation
that evaluates the documented expressions in fp32 with correctly rounded + - * / sqrt, from the SAME fp32 inputs, whatever
the order inside a commutative pair; hyper-parameters are fp32 roundings of the python floats (u each) except the powers
b^step and what is formed from them in double (lr / bc1, sqrt(bc2): one rounding to fp32 each).  None is fitted.
    norm    the sum of squares: one rounding per square and one per addition on the longest chain of additions a partial sum
            sees; sqrt halves it and rounds once, the conversion of the double sum rounds once: e_n = ((1 + chain) / 2 + 2) u.
            The kernel's chain is counted: 15 additions in a thread, 6 shuffle levels, 3 across the waves (KERNEL_CHAIN = 24;
            the final sum over the slots is in double).  torch's reduction is not ours to count: ANY_CHAIN = 64 is an
            allowance for it, used wherever one bound has to hold the kernel and the torch composite alike.
    coef    max_norm / (norm + 1e-6): max_norm, the sum, the quotient, 1e-6 as fp32: e_c = e_n + 4 u (0 where coef = 1 on
            both sides of e_n, and for records that are not clipped)
    g'      coef g: (e_c + u) |g'|
    p1      p - (lr wd) p, or p (1 - lr wd): 4 u lr wd |p| + 2 u |p1|
    m'      m + (1 - b1)(g' - m): (1 - b1) E_g + 3 u (1 - b1) |g' - m| + u |m'|
    v'      b2 v + ((1 - b2) g') g': 2 u b2 v + (2 (e_c + u) + 3 u)(1 - b2) g'^2 + u v'
    denom   sqrt(v') / sqrt(bc2) + eps: E_s = E_v / (2 sqrt v') + u sqrt v'; E_q = E_s / sqrt(bc2) + 2 u q;
            E_d = E_q + u eps + u denom
    r       ((lr / bc1) m') / denom: E_num = ss E_m + 3 u |ss m'|; E_r = E_num / denom + |r| E_d / denom + u |r|
    p'      p1 - r: E_p1 + E_r + u |p'|
    t'      d t + (1 - d) p', or t + (1 - d)(p' - t): 2 u d |t| + (1 - d) E_p + 3 u (1 - d)(|p'| + |t|) + u |t'|
    int     a copy: 0.
    slot    one workgroup's sum of squares, before the sqrt and the sum over the slots: (1 + chain) u of the slot (slot_error).
"""
import math

import numpy as np

U = 2.0 ** -24
KERNEL_CHAIN = 15 + 6 + 3
ANY_CHAIN = 64

REFERENCE_HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)       # cfgs/tooth_semi/default.yaml:66-68
EXAGGERATED_HP = dict(lr=0.1, betas=(0.5, 0.75), eps=1e-3, weight_decay=0.1)


def total_norm(grads):
    return math.sqrt(sum(float((np.asarray(g, dtype=np.float64) ** 2).sum()) for g in grads))


def clip_coef(norm, max_norm):
    x = max_norm / (norm + 1e-6)
    return x if (x < 1.0 or x != x) else 1.0


def norm_error(chain, u=U):
    """Relative bound of total_norm for this chain of additions."""
    return ((1 + chain) / 2 + 2) * u


def slot_error(chain, u=U):
    """Relative bound of ONE workgroup's fp32 sum of squares (a slot of the norm sweep) against its fp64 value, counted as
    norm_error counts: every term is rounded once as a square and passes through at most `chain` additions, and all terms
    are non-negative, so the sum's relative error is at most its worst term's: (1 + chain) u."""
    return (1 + chain) * u


def tail(records, groups, max_norm=None, decay=None, drop=(), u=U, chain=ANY_CHAIN, norm=None):
    given, norm, coef, e_c = norm, 0.0, 1.0, 0.0
    if max_norm is not None:
        with np.errstate(all="ignore"):
            norm = given if given is not None else total_norm([r["g"] for r in records if r["kind"] == "adamw" and r["clipped"]])
            coef = clip_coef(norm, max_norm)
        e_n = norm_error(chain, u)
        if not (coef == 1.0 and clip_coef(norm * (1 + e_n), max_norm) == 1.0):
            e_c = e_n + 4 * u
    if "clip" in drop:
        coef = 1.0
    out = []
    with np.errstate(all="ignore"):
        for r in records:
            f64 = lambda k: np.asarray(r[k], dtype=np.float64)      # noqa: E731
            res = {"kind": r["kind"]}
            if r["kind"] == "int":
                res["t"], res["E_t"] = np.array(r["p"]), np.zeros(np.shape(r["p"]))
                out.append(res)
                continue
            e_p = 0.0
            p_new = f64("p")
            if r["kind"] == "adamw":
                hp = groups[r["group"]]
                lr, (b1, b2), eps, wd = hp["lr"], hp["betas"], hp["eps"], hp["weight_decay"]
                if "wd" in drop:
                    wd = 0.0
                if "eps" in drop:
                    eps = 0.0
                p, g, m, v = f64("p"), f64("g"), f64("m"), f64("v")
                step = r["step"] + 1
                bc1 = 1.0 if "bc1" in drop else 1.0 - b1 ** step
                bc2 = 1.0 if "bc2" in drop else 1.0 - b2 ** step
                clipped = r["clipped"] and max_norm is not None
                g1 = coef * g if clipped else g
                e_g = (e_c + u) if clipped else 0.0
                p1 = p - lr * wd * p
                m1 = m + (1 - b1) * (g1 - m)
                v1 = b2 * v + (1 - b2) * g1 * g1
                sq = np.sqrt(v1)
                q = sq / math.sqrt(bc2)
                denom = q + eps
                ss = lr / bc1
                rr = ss * m1 / denom
                p_new = p1 - rr
                E_g = e_g * np.abs(g1)
                E_p1 = 4 * u * lr * wd * np.abs(p) + 2 * u * np.abs(p1)
                E_m = (1 - b1) * E_g + 3 * u * (1 - b1) * np.abs(g1 - m) + u * np.abs(m1)
                E_v = 2 * u * b2 * v + (2 * e_g + 3 * u) * (1 - b2) * g1 * g1 + u * v1
                E_s = np.where(v1 > 0, E_v / (2 * np.where(v1 > 0, sq, 1.0)), 0.0) + u * sq
                E_q = E_s / math.sqrt(bc2) + 2 * u * q
                E_d = E_q + u * eps + u * denom
                E_num = ss * E_m + 3 * u * np.abs(ss * m1)
                E_r = E_num / denom + np.abs(rr) * E_d / denom + u * np.abs(rr)
                e_p = E_p1 + E_r + u * np.abs(p_new)
                res.update(p=p_new, m=m1, v=v1, step=step, E_p=e_p, E_m=E_m, E_v=E_v)
            if r.get("t") is not None:
                t = f64("t")
                if "ema" in drop or decay is None:
                    res["t"], res["E_t"] = t, np.zeros(t.shape)
                else:
                    t1 = decay * t + (1 - decay) * p_new
                    res["t"] = t1
                    res["E_t"] = (2 * u * decay * np.abs(t) + (1 - decay) * e_p + 3 * u * (1 - decay) * (np.abs(p_new) + np.abs(t))
                                  + u * np.abs(t1))
            out.append(res)
    return out, norm, coef


def ratio(got, want, bound):
    """Largest |got - want| / bound; where the bound is 0 an exact match is demanded; a non-finite `want` must be matched in
    kind (NaN by NaN, an infinity by the same infinity)."""
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), np.shape(want)).ravel()
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    if got.size == 0:
        return 0.0
    fin = np.isfinite(want)
    if not np.array_equal(np.isnan(got[~fin]), np.isnan(want[~fin])) or not np.array_equal(got[~fin][~np.isnan(want[~fin])],
                                                                                          want[~fin][~np.isnan(want[~fin])]):
        return math.inf
    got, want, bound = got[fin], want[fin], bound[fin]
    if not np.all(np.isfinite(got)):
        return math.inf
    err = np.abs(got - want)
    zero = ~(bound > 0)
    if np.any(err[zero] != 0):
        return math.inf
    return float((err[~zero] / bound[~zero]).max()) if np.any(~zero) else 0.0


# ---- the tensor set of the plan and kernel tests -------------------------------------------------------------------------------
BLOCK = 4096          # GEOT_OPTIM_TAIL_BLOCK_ELEMS, restated: the tests assert that the header agrees
COUNTS = (0, 1, 3, 4, 5, BLOCK, BLOCK + 1, 3 * BLOCK + 7)


def make_records(seed, counts=COUNTS, warm=True):
    """fp32 arrays for one AdamW record per count: group i % 2, clipped unless i % 3 == 2, a teacher unless i % 4 == 3;
    warm: moments as if three steps had run (step = 3), else a fresh state (zeros, step = 0).  One record's gradient is
    scaled down by 1e-3, so that eps carries weight somewhere."""
    rng = np.random.default_rng(seed)
    recs = []
    for i, n in enumerate(counts):
        g = rng.standard_normal(n).astype(np.float32) * np.float32(1e-3 if i == 5 else 1.0)
        r = {"kind": "adamw", "p": rng.standard_normal(n).astype(np.float32), "g": g, "group": i % 2,
             "clipped": i % 3 != 2, "step": 3 if warm else 0}
        if warm:
            r["m"] = (0.5 * g + 0.3 * rng.standard_normal(n) * np.abs(g)).astype(np.float32)
            r["v"] = (g.astype(np.float64) ** 2 * (0.5 + rng.random(n))).astype(np.float32)
        else:
            r["m"], r["v"] = np.zeros(n, np.float32), np.zeros(n, np.float32)
        r["t"] = (r["p"] + 0.1 * rng.standard_normal(n)).astype(np.float32) if i % 4 != 3 else None
        recs.append(r)
    return recs


def make_buffers(seed):
    """EMA-only records (float buffers) and one int64 record, as a BatchNorm holds them."""
    rng = np.random.default_rng((seed, 7))
    out = []
    for n in (1, 37, BLOCK + 3):
        out.append({"kind": "ema", "p": rng.standard_normal(n).astype(np.float32), "t": rng.standard_normal(n).astype(np.float32)})
    out.append({"kind": "int", "p": rng.integers(0, 2 ** 40, 5).astype(np.int64), "t": np.zeros(5, np.int64)})
    return out


def groups_of(hp):
    """Two groups as the optimizer factory makes them: with and without weight decay."""
    return [dict(hp), dict(hp, weight_decay=0.0)]
