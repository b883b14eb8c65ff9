"""fp64 restatement of the two per-point NTM operations (sig_t_mean, correct_logits; csrc/ntm.hip) for tests that aim the
17-class kernels at their in-kernel branches: plain numpy.  The formulas are those of oracle/np_ntm.py; what this adds is
the clamp-region masks, the entries fp32 may legitimately put on the other side of a clamp bound, d raw itself, per-row
conditioning figures for derived bounds, arbitrary-sign correct_logits operands with zero rows, the input builders the
test cases need, and an op-by-op fp32 torch composite of the same statements (the yardstick for the long sums).

    raw[i][kk][o] = sum_j p_ij W[kk][o][j] + sum_j cm[kk][j] W[kk][o][C + j]
    tc = clip(raw, 1e-5, 1 - 1e-5),  den = max(sum_o tc, 1e-12),  out = tc / den
    d raw = [1e-5 <= raw <= 1 - 1e-5] (g - sum_o g out) / den,      grad_W[kk] = d raw[:, kk]^T [p | cm[kk]]

    v = lam E + (1 - lam) T_i,  s = sum_c |v|,  tn = v / max(s, 1e-12),  out[c] = sum_r l_r tn[r][c]
    d v = (l_r g_c - sign(v) sum_c l_r g_c tn) / s   (s > 1e-12),   l_r g_c / 1e-12   (otherwise)
    grad_logits[r] = sum_c tn[r][c] g_c,  grad_ins_T = (1 - lam) d v,  grad_ema_t = lam sum_i d v

Bounds, derived from the arithmetic and never from a kernel's output:
  * RAW_EPS = 2e-7: the error of an 18-term fp32 dot product of O(1) terms.  EDGE = 10 RAW_EPS: an entry whose fp64 raw lies
    that close to a clamp bound may land on either side in fp32.  clip() is continuous, so the forward, den and the dot of
    a row do not notice; only the entry's own d raw (on or off) and its contribution to grad_W do.
  * d raw: every quantity of a row carries the relative perturbation of den, cond = n_inside RAW_EPS / den (den can be as
    small as 17e-5 when a row is nearly all clamped low).  To first order
        |delta d raw| <= 2 cond rowscale,   rowscale = (max_o |g_o| + |dot|) / den
    (cond rowscale from 1 / den, the same again from dot); the bound is (1e-4 + 3 cond) rowscale: the project's 1e-4,
    taken of the ROW's scale instead of the array's (tighter wherever a row is well conditioned), plus the conditioning.
  * grad_W: a tolerance of the array's scale plus, per weight, the summed magnitude of what the edge entries would
    contribute if they flipped.
  * correct_logits, mixed signs: absolute bounds are scaled by max|l| max|v| / min s (rows with s > 1e-12).

Any class count (the run-time-C kernels of csrc/ntm_generic.hip, tests/test_ntm_generic_kernels_gpu.py): every function takes
c, or reads it off its operands; c = 17 with default arguments is the 17-class suite's case, unchanged.  What differs at c != 17:
  * the raw-value error is per entry and derived: raw_eps = (c + 2) 2^-24 (sum_j |p_j W_j| + sum_j |cm_j W_{c+j}|), the
    first-order bound of a (2c)-term fp32 dot product in any order plus the bias' own sum and rounding; an entry is an
    edge entry within 10 raw_eps of a clamp bound, cond = sum_o raw_eps_o / den over the entries inside the clamp and the
    edge entries: an edge entry below the clamp in fp64 may be above it in fp32, by at most raw_eps, and where the rest of
    its row is clamped low (den of a few 1e-5) that is a relative change of den no fixed 1e-4 covers.
  * W is uniform in +-2 (sig_inputs(b, n, c, amp=2.0)): the 8 / sqrt(2c) scaling puts under 1 % of the raw values above the
    clamp from c = 20 up.  The all-low head is min(3, c - 1), the zero row of correct_inputs min(5, c - 1).
  * the forward's row sums: den carries at most c - 1 roundings in any summation order, an entry its reciprocal's and its
    product's, so |sum_o out - 1| <= (c + 1) U to first order; the bound is max(2c - 2, c + 1) U (32 U at c = 17, as before).
    An all-low row holds c equal entries: c 2U / c, as before.
  * the forward's entries: W in +-2 leaves rows whose den is a few 1e-4 (every entry but one or two clamped low), and there
    the raw error of an unclamped entry, raw_eps / den, exceeds the project's 1e-5 |out| + 2e-5 in any fp32 arithmetic (the
    op-by-op composite misses it 4.8-fold at c = 9, (2, 1001)).  To first order delta out_o = delta raw_o / den -
    out_o sum_o' delta raw_o' / den over the entries the clamp leaves alone, so the bound gains
    2 ([o unclamped] raw_eps_o / den + out_o cond), which is below 2e-5 wherever den >= 0.5.
  * grad_W below 32 768 points: the project's 2e-4 rule plus grad_W_cond, the conditioning term of d raw (3 cond rowscale,
    above) summed over the points with the magnitudes of [p | cm]: with W in +-2 the rows of den ~ 2e-4 carry d raw entries
    of 1e4 times the gradient with a relative error of 1e-2, and the op-by-op composite misses the plain rule 2.3-fold at
    c = 9, 8193 points.  Zero at c = 17, where the term is not derived.
  * sums over more than 32 768 points are held to 4 x the error of the fp32 composite on the same inputs, which the test
    computes itself (large_tol).  Measured on an MI355X, 2026-10-20, at (3, 10931), largest |error| / max |reference| of
    grad_W with the edge contributions taken off, composite | d raw kernel + torch.mm: c = 5 3.79e-4 | 5.14e-5, c = 6
    1.61e-4 | 3.30e-4, c = 13 1.62e-5 | 3.58e-6 (the conditioning of a few rows, not the length of the sum).
  * correct_logits' d v is a difference of products that cancel, wholly at c = 1: see grad_ins_T_cancel in correct_logits."""
import numpy as np

C = 17
LO, HI = 1e-5, 1.0 - 1e-5
RAW_EPS = 2e-7
EDGE = 2e-6
ALL_LOW_HEAD = 3
ZERO_ROW = 5
TILE = 32                      # points per tile of the ntm_correct kernels


def softmax(x, axis):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


# ---- sig_t_mean -----------------------------------------------------------------------------------------------------------
def sig_t_mean(p, cm, W, g=None, derived=None, want_grad_W=True):
    """p (B, c, N), cm (c, c), W (c, c, 2c) [kk][o][in], g (B*N, c, c) or None -> dict:
    out, raw, den, below / inside / above / edge masks, and with g: draw, draw_bound, grad_W, grad_W_edge.
    derived (default: c != 17): the raw-value error is the per-entry bound raw_eps instead of the constant RAW_EPS.
    want_grad_W=False leaves out the three weight-shaped sums (a chunk of the points has no use for them)."""
    p, cm, W = (np.asarray(a, dtype=np.float64) for a in (p, cm, W))
    B, c, N = p.shape
    derived = (c != C) if derived is None else derived
    x = p.transpose(0, 2, 1).reshape(B * N, c)
    raw = np.einsum("ij,koj->iko", x, W[:, :, :c]) + np.einsum("kj,koj->ko", cm, W[:, :, c:])[None]
    if derived:
        mag = np.einsum("ij,koj->iko", x, np.abs(W[:, :, :c])) + np.einsum("kj,koj->ko", cm, np.abs(W[:, :, c:]))[None]
        raw_eps = (c + 2) * 2.0 ** -24 * mag                     # p and cm are non-negative
    else:
        raw_eps = np.full_like(raw, RAW_EPS)
    below, above = raw < LO, raw > HI
    inside = ~(below | above)
    edge = (np.abs(raw - LO) <= 10 * raw_eps) | (np.abs(raw - HI) <= 10 * raw_eps) if derived else \
        (np.abs(raw - LO) <= EDGE) | (np.abs(raw - HI) <= EDGE)
    tc = np.clip(raw, LO, HI)
    den = np.maximum(tc.sum(2, keepdims=True), 1e-12)            # clamped values are positive
    r = dict(out=tc / den, raw=raw, den=den, below=below, inside=inside, above=above, edge=edge, raw_eps=raw_eps,
             derived=derived, cond=((inside | edge) * raw_eps).sum(2, keepdims=True) / den)
    if g is None:
        return r
    g = np.asarray(g, dtype=np.float64)
    dot = (g * r["out"]).sum(2, keepdims=True)
    dtc = (g - dot) / den
    draw = dtc * inside
    cond = r["cond"] if derived else inside.sum(2, keepdims=True) * RAW_EPS / den
    rowscale = (np.abs(g).max(2, keepdims=True) + np.abs(dot)) / den
    if not want_grad_W:
        r.update(rowscale=rowscale, draw=draw, draw_bound=np.broadcast_to((1e-4 + 3.0 * cond) * rowscale, draw.shape))
        return r
    gW = np.empty_like(W)
    gW_edge = np.empty_like(W)
    flip = np.abs(dtc) * edge
    for kk in range(c):
        gW[kk, :, :c] = draw[:, kk, :].T @ x
        gW[kk, :, c:] = draw[:, kk, :].sum(0)[:, None] * cm[kk][None]
        gW_edge[kk, :, :c] = flip[:, kk, :].T @ np.abs(x)
        gW_edge[kk, :, c:] = flip[:, kk, :].sum(0)[:, None] * np.abs(cm[kk])[None]
    # what the rows' conditioning can move in grad_W: sum_i 3 cond_i rowscale_i |[p | cm]| over the entries inside the clamp
    gW_cond = np.zeros_like(W)
    if derived:
        wob = 3.0 * cond * rowscale * inside
        for kk in range(c):
            gW_cond[kk, :, :c] = wob[:, kk, :].T @ np.abs(x)
            gW_cond[kk, :, c:] = wob[:, kk, :].sum(0)[:, None] * np.abs(cm[kk])[None]
    r.update(grad_W_cond=gW_cond, rowscale=rowscale, draw=draw, draw_bound=np.broadcast_to((1e-4 + 3.0 * cond) * rowscale, draw.shape), grad_W=gW,
             grad_W_edge=gW_edge)
    return r


def region_shares(r):
    """(below, inside, above, edge) shares of a sig_t_mean result."""
    return tuple(float(r[k].mean()) for k in ("below", "inside", "above", "edge"))


# ---- correct_logits -------------------------------------------------------------------------------------------------------
def correct_logits(logits, ins_T, E, lam, g=None, groups=None):
    """logits (B, c, N), ins_T (B*N, c, c), E (c, c) of any sign, lam as the kernel sees it (a C float) -> dict:
    out (B, c, N), s (B*N, c), scale, and with g (B, c, N): grad_logits, grad_ins_T, grad_ema_t, grad_ema_t_abs (the summed
    magnitudes of each entry's terms), grad_ema_t_tile_abs (the summed magnitudes of the 32-point tiles' sums, or of the sums
    over the points of each id of `groups` (B*N ints): what one workgroup adds with one atomic), gscale."""
    lam = float(np.float32(lam))
    l3, T, E = (np.asarray(a, dtype=np.float64) for a in (logits, ins_T, E))
    B, c, N = l3.shape
    v = lam * E[None] + (1.0 - lam) * T
    s = np.abs(v).sum(2, keepdims=True)
    den = np.maximum(s, 1e-12)
    tn = v / den
    l = l3.transpose(0, 2, 1).reshape(B * N, c)
    out = np.einsum("ir,irc->ic", l, tn)
    live = s[:, :, 0] > 1e-12
    smin = s[:, :, 0][live].min() if live.any() else 1.0
    r = dict(out=out.reshape(B, N, c).transpose(0, 2, 1), s=s[:, :, 0], live=live,
             scale=np.abs(l).max() * np.abs(v).max() / smin)
    if g is None:
        return r
    go = np.asarray(g, dtype=np.float64).transpose(0, 2, 1).reshape(B * N, c)
    gl = np.einsum("irc,ic->ir", tn, go)
    dtn = l[:, :, None] * go[:, None, :]
    dv = np.where(s > 1e-12, (dtn - np.sign(v) * (dtn * tn).sum(2, keepdims=True)) / den, dtn / den)
    # c != 17: d v is a difference of two products that cancel -- wholly at c = 1, where v / |v| is a sign and d v is zero in
    # exact arithmetic, so no multiple of the array's scale bounds what fp32 leaves.  The products carry one rounding and the
    # c-term sum in grad_logits its own: (c + 4) U (|l g_c| + |l| sum_c |tn g_c|) / s per entry, summed for grad_ema_t.
    cancel = 0.0
    if c != C:
        cancel = (c + 4) * U * (np.abs(dtn) + np.abs(l)[:, :, None] * (np.abs(tn) * np.abs(go)[:, None, :]).sum(2, keepdims=True)) / den * (s > 1e-12)
    r.update(grad_ins_T_cancel=(1.0 - lam) * cancel, grad_ema_t_cancel=lam * np.sum(cancel, axis=0))
    if groups is None:
        sums = np.add.reduceat(dv, np.arange(0, B * N, TILE), axis=0)
    else:
        order = np.argsort(np.asarray(groups), kind="stable")
        starts = np.flatnonzero(np.diff(np.asarray(groups)[order], prepend=-1))
        sums = np.add.reduceat(dv[order], starts, axis=0)
    r.update(grad_logits=gl.reshape(B, N, c).transpose(0, 2, 1), grad_ins_T=(1.0 - lam) * dv, grad_ema_t=lam * dv.sum(0),
             grad_ema_t_abs=lam * np.abs(dv).sum(0),
             grad_ema_t_tile_abs=lam * np.abs(sums).sum(0), gscale=np.abs(go).max() * np.abs(v).max() / smin)
    return r


# ---- the bounds, as checks that return the largest error / bound (a zero bound demands an exact zero) --------------------
# grad_W and grad_ema_t at 32 793 points are longer fp32 sums than the project's 2e-4 / 1e-3 were set for, so their bound there
# is 4 x the error of the op-by-op fp32 torch composite below against this fp64 reference on the same inputs (the factor
# covers another summation tree and fp32 MFMA accumulation).  Measured, largest |error| / max |reference|:
#   grad_W     composite 1.56e-7 (edge contributions taken off; 7.3e-4 with them: the composite itself flips an entry) with
#              a GEMM that blocks the 32 793-term sums; 2.2e-6 with another CPU's BLAS.  The constant is 4 x the smaller.
#   grad_ema_t composite 2.45e-7 at lam = 0.9, 1.68e-7 at lam = 1.0, exactly 0 at lam = 0
#   the kernels on an MI355X: grad_W 1.53e-7; grad_ema_t 2.76e-7 (lam = 0.9), 2.73e-7 (lam = 1.0) through the workspace,
#   9.5e-7 and 8.3e-7 in two runs of the atomic form (arrival order; it has its own any-order term below)
LARGE_PTS = 32768
GRAD_W_TOL, GRAD_W_TOL_LARGE = 2e-4, 4 * 1.56e-7
GRAD_E_TOL, GRAD_E_TOL_LARGE = 1e-3, 4 * 2.45e-7
U = 2.0 ** -24


def worst(err, bound):
    err, bound = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64))
    if err.size == 0:
        return 0.0
    assert not np.isnan(err).any(), "NaN left in a result"
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf)).max())


def sig_forward_bound(ref):
    """per entry: the project's 1e-5 |out| + 2e-5, and for c != 17 the row's conditioning (see the module's text)"""
    want = ref["out"]
    bound = 1e-5 * np.abs(want) + 2e-5
    if ref["derived"]:
        bound = bound + 2 * ((ref["inside"] | ref["edge"]) * ref["raw_eps"] / ref["den"] + want * ref["cond"])
    return bound


def sig_forward_ratio(got, ref):
    """Every entry (clip is continuous: the edge entries too), the row sums, and the all-low head's 1/c."""
    got = np.asarray(got, dtype=np.float64)
    want = ref["out"]
    c = want.shape[2]
    rows = worst(np.abs(got.sum(2) - 1.0), max(2 * c - 2, c + 1) * U)   # c - 1 additions in den, the reciprocal, c products
    low = ref["below"].all(2)                             # rows that clamp low as a whole: c equal entries
    if ref["derived"]:
        low &= ~ref["edge"].any(2)                        # (clear of the bound in fp32 too)
    flat = worst(np.abs(got[low] - 1.0 / c), c * 2 * U / c)
    return max(worst(np.abs(got - want), sig_forward_bound(ref)), rows, flat)


def draw_ratio(got, ref):
    """Every non-edge entry; an exact zero wherever the reference is outside the clamp."""
    ne = ~ref["edge"]
    return worst(np.abs(np.asarray(got, dtype=np.float64) - ref["draw"])[ne], (ref["draw_bound"] * ref["inside"])[ne])


def grad_W_ratio(got, ref, pts, base=None, large_tol=GRAD_W_TOL_LARGE):
    """base: what the buffer held before the call (the entry point adds).  The edge entries' possible contributions are taken
    off the error (|err| <= bound + edge is the same statement), so the figure says how much of the bound the sums use.
    large_tol: the bound from LARGE_PTS points up, of the array's scale (the 17-class constant, or 4 x composite_error())."""
    want = ref["grad_W"]
    top = np.abs(want).max()
    bound = large_tol * top if pts >= LARGE_PTS else GRAD_W_TOL * np.abs(want) + GRAD_W_TOL * top + ref["grad_W_cond"]
    if base is not None:
        base = np.asarray(base, dtype=np.float64)
        want, bound = want + base, bound + 2 * U * (np.abs(base) + np.abs(want))
    return worst(np.maximum(np.abs(np.asarray(got, dtype=np.float64) - want) - ref["grad_W_edge"], 0.0), bound)


def correct_forward_ratio(got, ref):
    return worst(np.abs(np.asarray(got, dtype=np.float64) - ref["out"]), 1e-5 * np.abs(ref["out"]) + 2e-5 * ref["scale"])


def correct_grads_ratio(gl, gi, gE, ref, pts, base_E=None, atomic_adds=0):
    """(grad_logits, grad_ins_T, grad_ema_t) ratios.  Rows with s <= 1e-12 hold l g / 1e-12: those entries, and the grad_ema_t
    rows they are summed into, are held entry by entry to 1e-5 of their own magnitude (of the summed magnitudes of the
    entry's terms for grad_ema_t), and stay out of every array maximum.
    atomic_adds: the form that adds its block sums to grad_ema_t with float atomics rounds the running value once per block, in
    arrival order: at most atomic_adds 2^-24 x the summed magnitudes of the block sums (a block sum is a sum of tile sums) on
    top of the bound, whatever the order."""
    gl, gi, gE = (np.asarray(a, dtype=np.float64) for a in (gl, gi, gE))
    live = ref["live"]
    r_l = worst(np.abs(gl - ref["grad_logits"]), 1e-4 * np.abs(ref["grad_logits"]) + 1e-5 * ref["gscale"])
    wi = ref["grad_ins_T"]
    top = np.abs(wi[live]).max() if live.any() else 0.0
    r_i = max(worst(np.abs(gi - wi)[live], (1e-4 * np.abs(wi) + 1e-4 * top + ref["grad_ins_T_cancel"])[live]),
              worst(np.abs(gi - wi)[~live], 1e-5 * np.abs(wi)[~live]))
    wE, rows = ref["grad_ema_t"], live.all(0)
    top = np.abs(wE[rows]).max() if rows.any() else 0.0
    bound = np.where(rows[:, None], GRAD_E_TOL_LARGE * top if pts >= LARGE_PTS else GRAD_E_TOL * np.abs(wE) + GRAD_E_TOL * top,
                     1e-5 * ref["grad_ema_t_abs"]) + atomic_adds * U * ref["grad_ema_t_tile_abs"] + ref["grad_ema_t_cancel"]
    if base_E is not None:
        base_E = np.asarray(base_E, dtype=np.float64)
        wE, bound = wE + base_E, bound + 2 * U * (np.abs(base_E) + np.abs(wE))
    return r_l, r_i, worst(np.abs(gE - wE), bound)


# ---- input builders -------------------------------------------------------------------------------------------------------
def all_low_head(c):
    return min(ALL_LOW_HEAD, c - 1)


def zero_row(c):
    return min(ZERO_ROW, c - 1)


def sig_inputs(b, n, c=C, seed=0, gain=8.0, all_low_head="default", amp=None):
    """p = softmax(2 randn), cm = softmax(randn), W uniform in +-amp, by default amp = gain / sqrt(2c) (nn.Linear's default
    init is gain = 1: no raw value reaches the upper clamp there); head `all_low_head` (by default min(3, c - 1), None: no
    such head) is -|W|, so its whole row clamps low at every point.  Also g, the upstream gradient of the output."""
    rng = np.random.default_rng(seed)
    if all_low_head == "default":
        all_low_head = min(ALL_LOW_HEAD, c - 1)
    p = softmax(rng.standard_normal((b, c, n)) * 2, 1).astype(np.float32)
    cm = softmax(rng.standard_normal((c, c)), 1).astype(np.float32)
    W = (rng.uniform(-1.0, 1.0, (c, c, 2 * c)) * (gain / np.sqrt(2 * c) if amp is None else amp)).astype(np.float32)
    if all_low_head is not None:
        W[all_low_head] = -np.abs(W[all_low_head])
    g = rng.standard_normal((b * n, c, c)).astype(np.float32)
    return p, cm, W, g


def correct_inputs(b, n, c=C, seed=1, zero_points=(), threshold_points=()):
    """logits, ins_T and E of both signs, not normalised, and the upstream gradient.  zero_points: flat point ids whose
    ins_T row zero_row(c) is exactly zero, together with E's row zero_row(c) (v = 0 there for every lam: the s <= 1e-12
    branch).  At c < 3 a row has so few entries that random ones cancel to s < 1e-3 somewhere among a few thousand points:
    there |E| >= 0.25 and 0.05 <= |ins_T| <= 2, so s >= 0.025 at lam = 0.9, 0.05 at lam = 0 and 0.25 at lam = 1.
    threshold_points (with zero_points): their row zero_row(c) is (float32(1e-12), 0, ...), so that at lam = 0 s is exactly the
    kernel's threshold 1e-12f -- not above it, in fp32 as in fp64 (the float is 9.9999999600e-13): the `s > 1e-12` side."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((b, c, n)) * 2).astype(np.float32)
    ins_T = rng.standard_normal((b * n, c, c)).astype(np.float32)
    E = rng.standard_normal((c, c)).astype(np.float32)
    g = rng.standard_normal((b, c, n)).astype(np.float32)
    if c < 3:
        E = (np.where(E < 0, -1, 1) * (0.25 + np.abs(E))).astype(np.float32)
        ins_T = (np.where(ins_T < 0, -1, 1) * np.minimum(0.05 + np.abs(ins_T), 2.0)).astype(np.float32)
    if len(zero_points):
        E[min(ZERO_ROW, c - 1)] = 0.0
        ins_T[list(zero_points), min(ZERO_ROW, c - 1)] = 0.0
        ins_T[list(threshold_points), min(ZERO_ROW, c - 1)] = 0.0
        ins_T[list(threshold_points), min(ZERO_ROW, c - 1), 0] = np.float32(1e-12)
    return logits, ins_T, E, g


# ---- the same statements op by op in fp32 torch (the yardstick of the long sums; never a kernel of the project) ------------
def composite_sig_grad_W(p, cm, W, g, device="cpu"):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(device)
    p, cm, W, g = t(p), t(cm), t(W), t(g)
    B, c, N = p.shape
    x = p.permute(0, 2, 1).reshape(B * N, c)
    raw = (x @ W[:, :, :c].reshape(c * c, c).t()).view(B * N, c, c) + torch.einsum("kj,koj->ko", cm, W[:, :, c:])[None]
    tc = raw.clamp(LO, HI)
    den = tc.sum(2, keepdim=True).clamp_min(1e-12)
    out = tc / den
    dot = (g * out).sum(2, keepdim=True)
    draw = ((g - dot) / den) * ((raw >= LO) & (raw <= HI))
    G = draw.view(B * N, c * c).t() @ torch.cat([x, torch.ones_like(x[:, :1])], 1)
    gW = torch.cat([G[:, :c].reshape(c, c, c), G[:, c].reshape(c, c, 1) * cm.unsqueeze(1)], 2)
    return out.cpu().numpy(), draw.cpu().numpy(), gW.cpu().numpy()


def composite_correct(logits, ins_T, E, lam, g, device="cpu"):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(device)
    l3, T, E, g = t(logits), t(ins_T), t(E), t(g)
    lam = float(np.float32(lam))
    B, c, N = l3.shape
    v = lam * E[None] + (1.0 - lam) * T
    s = v.abs().sum(2, keepdim=True)
    den = s.clamp_min(1e-12)
    tn = v / den
    l = l3.permute(0, 2, 1).reshape(B * N, c)
    go = g.permute(0, 2, 1).reshape(B * N, c)
    out = torch.einsum("ir,irc->ic", l, tn)
    gl = torch.einsum("irc,ic->ir", tn, go)
    dtn = l[:, :, None] * go[:, None, :]
    dv = torch.where(s > 1e-12, (dtn - torch.sign(v) * (dtn * tn).sum(2, keepdim=True)) / den, dtn / den)
    back = lambda a: a.reshape(B, N, c).permute(0, 2, 1).cpu().numpy()
    return back(out), back(gl), ((1.0 - lam) * dv).cpu().numpy(), (lam * dv.sum(0)).cpu().numpy()
