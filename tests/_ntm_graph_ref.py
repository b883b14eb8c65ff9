"""fp64 restatement of the two graph losses of the FixMatch+NTM loop (threeD_space_loss, feature_space_loss) for tests that
aim the kernels at hand-made graphs: plain numpy, no project code.  The formulas are those of oracle/np_ntm.py; what this
adds is global neighbour ids (any graph, not only a kNN result), an upstream gradient, per-element conditioning figures for
a derived tolerance, chunked evaluation (131 k points x 289 floats never sit in memory as (points, k, 289)), and the graph
builders the test cases need.

    w_ij = [l_i == l_j] exp(x_ij)        (signed: +-exp(x_ij)),   x_ij = -|p_i - p_j|^2 / (2 sigma^2)
    unsigned: per_point_i = sum_j w_ij |T_i - T_j|^2 / S_i,  S_i = sum_j w_ij + 1e-3,  c_i = 2 scale upstream / S_i
    signed:   per_point_i = sum_j w_ij |T_i - T_j|^2,                                  c_i = 2 scale upstream
    grad_i   += c_i w_ij (T_i - T_j),   grad_j -= c_i w_ij (T_i - T_j)       for every edge i -> j

Tolerance rule (u2 = 2^-23), derived from the arithmetic and not from any kernel's output:
    forward : |got - want| <= (5 k + 6 + 32) u2 * mag,   mag = sum_j |w_ij| |T_i - T_j|^2 / S_i
              (at most 5 k fp32 additions per lane -- five registers of a 289-float row times k neighbours --, six shuffle
              levels, 32 units for the rounding of d^2, __expf and the division while |x| <= 16).  Unsigned weights are
              non-negative and mag IS the reference value; the signed loss subtracts, and the bound of a sum with terms of
              both signs is relative to the sum of their magnitudes, never to the (possibly cancelled) result.
    gradient: |got - want| <= (terms + 32) u2 * cond   (+ terms 2^-40 scale |upstream| on the fixed-point path),
              cond = sum of the magnitudes of the element's terms, terms = live out-edges + live in-edges of its row
              (the bound of a sum taken in any order, which covers float atomics).
A zero bound (mag == 0 or cond == 0) demands an exact zero."""
import numpy as np

U2 = 2.0 ** -23
FIX = 2.0 ** -40


# ---- the reference ------------------------------------------------------------------------------------------------------
def graph_loss(x, labels, T, nbr, sigma, signed=False, upstream=1.0, scale=1.0, chunk=2048, want_grad=True):
    """x (t, d) positions or features, labels (t,), T (t, C, C), nbr (t, k) GLOBAL neighbour ids -> dict with
    per_point (t,), mag (t,), x (t, k), and (want_grad) grad, cond (t, C*C) and terms (t,)."""
    P = np.asarray(x, dtype=np.float64)
    lab = np.asarray(labels).reshape(-1)
    t, k = nbr.shape
    Tm = np.asarray(T, dtype=np.float64).reshape(t, -1)
    cc = Tm.shape[1]
    nbr = np.asarray(nbr, dtype=np.int64)
    assert P.shape[0] == t and lab.shape[0] == t and nbr.min() >= 0 and nbr.max() < t
    xs = np.empty((t, k))
    w = np.empty((t, k))
    per_point, mag = np.empty(t), np.empty(t)
    for a in range(0, t, chunk):
        j = nbr[a:a + chunk]
        d2 = ((P[a:a + chunk, None, :] - P[j]) ** 2).sum(2)
        xs[a:a + chunk] = -d2 / (2.0 * sigma ** 2)
        same = lab[a:a + chunk, None] == lab[j]
        e = np.exp(xs[a:a + chunk])
        w[a:a + chunk] = np.where(same, e, -e if signed else 0.0)
        td = ((Tm[a:a + chunk, None, :] - Tm[j]) ** 2).sum(2)
        S = 1.0 if signed else w[a:a + chunk].sum(1) + 0.001
        per_point[a:a + chunk] = (w[a:a + chunk] * td).sum(1) / S
        mag[a:a + chunk] = (np.abs(w[a:a + chunk]) * td).sum(1) / S
    out = {"per_point": per_point, "mag": mag, "x": xs, "w": w, "k": k}
    if not want_grad:
        return out
    S = np.ones(t) if signed else w.sum(1) + 0.001
    coef = (2.0 * scale * upstream) * w / S[:, None]                    # (t, k): c_i w_ij
    grad, cond = np.zeros((t, cc)), np.zeros((t, cc))
    live = w != 0.0
    terms = live.sum(1) + np.bincount(nbr[live], minlength=t)
    # out-edges: row i collects its own k terms
    for a in range(0, t, chunk):
        diff = Tm[a:a + chunk, None, :] - Tm[nbr[a:a + chunk]]
        c = coef[a:a + chunk, :, None] * diff
        grad[a:a + chunk] = c.sum(1)
        cond[a:a + chunk] = np.abs(c).sum(1)
    # in-edges: sorted by target, summed per target with reduceat (no scatter with repeated rows)
    src = np.repeat(np.arange(t), k)
    tgt = nbr.reshape(-1)
    cf = coef.reshape(-1)
    by = np.argsort(tgt, kind="stable")
    src, tgt, cf = src[by], tgt[by], cf[by]
    step = max(chunk * max(k, 1) // 4, 1)
    for a in range(0, src.size, step):
        s_, t_, c_ = src[a:a + step], tgt[a:a + step], cf[a:a + step]
        c = c_[:, None] * (Tm[t_] - Tm[s_])                             # -(c_s w_st (T_s - T_t))
        starts = np.flatnonzero(np.r_[True, t_[1:] != t_[:-1]])
        grad[t_[starts]] += np.add.reduceat(c, starts, axis=0)
        cond[t_[starts]] += np.add.reduceat(np.abs(c), starts, axis=0)
    out.update(grad=grad, cond=cond, terms=terms)
    return out


def forward_bound(ref):
    return (5 * ref["k"] + 6 + 32) * U2 * ref["mag"]


def grad_bound(ref, fixed=None):
    """fixed: scale * |upstream| of the call when the gradient went through the 2^-40 fixed-point sums."""
    b = (ref["terms"][:, None] + 32) * U2 * ref["cond"]
    if fixed is not None:
        b = b + np.where(ref["cond"] != 0.0, ref["terms"][:, None] * FIX * fixed, 0.0)
    return b


def worst_ratio(got, want, bound, what):
    """Every element within its bound, zero-bound elements exact; returns the largest error / bound."""
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    assert np.isfinite(got).all(), "%s: %d non-finite values (a buffer the kernel did not write in full?), first at %s" % (
        what, int((~np.isfinite(got)).sum()), np.argwhere(~np.isfinite(got))[0])
    err = np.abs(got - want)
    zero = bound == 0.0
    assert not err[zero].any(), "%s: %d elements must be exactly zero, first at %s" % (
        what, int((err[zero] != 0).sum()), np.argwhere(zero & (err != 0))[0])
    ratio = np.divide(err, bound, out=np.zeros_like(err), where=~zero)
    at = np.unravel_index(int(ratio.argmax()), ratio.shape) if ratio.size else ()
    assert ratio.size == 0 or ratio[at] <= 1.0, "%s: error %.3e over the bound %.3e (x %.2f) at %s, got %r want %r; %d elements over" % (
        what, err[at], bound[at], ratio[at], at, got[at], want[at], int((ratio > 1).sum()))
    return float(ratio.max()) if ratio.size else 0.0


def check_forward(got, ref, what):
    assert np.abs(ref["x"]).max() <= 16.0
    return worst_ratio(got, ref["per_point"], forward_bound(ref), what)


def check_grad(got, ref, what, fixed=None):
    assert np.abs(ref["x"]).max() <= 16.0
    return worst_ratio(got, ref["grad"], grad_bound(ref, fixed), what)


# ---- an fp32 restatement with its own summation order (what the tolerance rule must hold for) ------------------------------
def graph_loss_fp32(x, labels, T, nbr, sigma, signed, upstream, scale, rng):
    """The same losses in fp32 numpy, every sum in a shuffled order: (per_point, grad)."""
    f = np.float32
    P, lab = np.asarray(x, dtype=f), np.asarray(labels).reshape(-1)
    t, k = nbr.shape
    Tm = np.asarray(T, dtype=f).reshape(t, -1)
    cc = Tm.shape[1]
    d2 = np.zeros((t, k), f)
    for d in rng.permutation(P.shape[1]):
        dx = P[:, None, d] - P[nbr, d]
        d2 += dx * dx
    e = np.exp(-d2 * f(1.0 / (2.0 * sigma * sigma)))
    same = lab[:, None] == lab[nbr]
    w = np.where(same, e, -e if signed else f(0)).astype(f)
    S = np.full(t, 1.0, f) if signed else np.zeros(t, f)
    acc = np.zeros(t, f)
    slots = rng.permutation(k)
    if not signed:
        for l in slots:
            S += w[:, l]
        S += f(0.001)
    cols = rng.permutation(cc)
    for l in slots:
        diff = Tm - Tm[nbr[:, l]]
        for c0 in range(0, cc, 64):
            sl = cols[c0:c0 + 64]
            acc += (w[:, l, None] * diff[:, sl] * diff[:, sl]).sum(1, dtype=f)
    per_point = acc / S
    # gradient: one list of 2 t k terms, shuffled, accumulated one after another in fp32
    two_g = f(2.0) * f(scale) * f(upstream)
    co = (two_g * (w / S[:, None])).astype(f)
    src = np.repeat(np.arange(t), k)
    tgt = nbr.reshape(-1)
    c = co.reshape(-1, 1) * (Tm[src] - Tm[tgt])
    rows = np.concatenate([src, tgt])
    vals = np.concatenate([c, -c]).astype(f)
    p = rng.permutation(rows.size)
    grad = np.zeros((t, cc), f)
    np.add.at(grad, rows[p], vals[p])
    return per_point, grad


# ---- graph builders (local ids per cloud unless said otherwise) ---------------------------------------------------------
def to_global(nbr_local):
    """(b, n, k) local ids -> (b n, k) global ids."""
    b, n, k = nbr_local.shape
    return (np.asarray(nbr_local, dtype=np.int64) + np.arange(b)[:, None, None] * n).reshape(b * n, k)


def in_degrees(nbr_global, live=None):
    t = nbr_global.shape[0]
    return np.bincount(nbr_global[live] if live is not None else nbr_global.reshape(-1), minlength=t)


def random_out_lists(rng, b, n, k, exclude=()):
    """(b, n, k) int32: k distinct ids per point, the point itself and `exclude` never among them."""
    out = np.empty((b, n, k), np.int32)
    if n > 2048:            # large clouds: distinct non-zero offsets, redrawing the (rare) rows with a repeat
        assert not exclude and 4 * k * k < n
        for bb in range(b):
            off = rng.integers(1, n, (n, k))
            while True:
                s = np.sort(off, 1)
                bad = (s[:, 1:] == s[:, :-1]).any(1)
                if not bad.any():
                    break
                off[bad] = rng.integers(1, n, (int(bad.sum()), k))
            out[bb] = (np.arange(n)[:, None] + off) % n
        return out
    ex = np.zeros(n, bool)
    ex[list(exclude)] = True
    for bb in range(b):
        for i in range(n):
            ok = ~ex
            ok[i] = False
            pool = np.flatnonzero(ok)
            assert pool.size >= k, "a cloud of %d points cannot give %d distinct neighbours" % (n, k)
            out[bb, i] = rng.choice(pool, k, replace=False)
    return out


def ensure_edge(nbr, b, i, j, slot=0):
    """Point i of cloud b lists j (in `slot` unless it already does)."""
    if j not in nbr[b, i]:
        nbr[b, i, slot] = j


def remove_edge(nbr, rng, b, i, j, avoid=()):
    """Point i of cloud b no longer lists j: the slot gets an id that is new to the list, not i and not in `avoid`."""
    n = nbr.shape[1]
    for s in np.flatnonzero(nbr[b, i] == j):
        taken = set(nbr[b, i].tolist()) | {i, j} | set(avoid)
        pool = [c for c in range(n) if c not in taken]
        nbr[b, i, s] = pool[int(rng.integers(len(pool)))]


def planted_in_degree(rng, n, k, target, d):
    """(1, n, k): exactly d points list `target`; the target's own list is random."""
    assert 0 <= d <= n - 1 and k <= n - 2
    nbr = random_out_lists(rng, 1, n, k, exclude=(target,))
    others = np.array([i for i in range(n) if i != target])
    nbr[0, target] = rng.choice(others, k, replace=False)
    for i in rng.choice(others, d, replace=False):
        nbr[0, i, int(rng.integers(k))] = target
    return nbr


def labels_equal(t):
    return np.zeros(t, np.int32)


def labels_all_different(t):
    return np.arange(t, dtype=np.int32)


def labels_mixed(rng, t, classes=3):
    return rng.integers(0, classes, t).astype(np.int32)


def row_stochastic(rng, t, c):
    """(t, c, c) float32, rows positive with unit sum: |T_i - T_j| <= 1 like sig_t_mean's output."""
    m = rng.random((t, c, c), dtype=np.float32) + np.float32(0.01)
    return (m / m.sum(2, keepdims=True)).astype(np.float32)
