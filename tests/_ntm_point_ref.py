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
  * correct_logits, mixed signs: absolute bounds are scaled by max|l| max|v| / min s (rows with s > 1e-12)."""
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
def sig_t_mean(p, cm, W, g=None):
    """p (B, C, N), cm (C, C), W (C, C, 2C) [kk][o][in], g (B*N, C, C) or None -> dict:
    out, raw, den, below / inside / above / edge masks, and with g: draw, draw_bound, grad_W, grad_W_edge."""
    p, cm, W = (np.asarray(a, dtype=np.float64) for a in (p, cm, W))
    B, c, N = p.shape
    x = p.transpose(0, 2, 1).reshape(B * N, c)
    raw = np.einsum("ij,koj->iko", x, W[:, :, :c]) + np.einsum("kj,koj->ko", cm, W[:, :, c:])[None]
    below, above = raw < LO, raw > HI
    inside = ~(below | above)
    edge = (np.abs(raw - LO) <= EDGE) | (np.abs(raw - HI) <= EDGE)
    tc = np.clip(raw, LO, HI)
    den = np.maximum(tc.sum(2, keepdims=True), 1e-12)            # clamped values are positive
    r = dict(out=tc / den, raw=raw, den=den, below=below, inside=inside, above=above, edge=edge)
    if g is None:
        return r
    g = np.asarray(g, dtype=np.float64)
    dot = (g * r["out"]).sum(2, keepdims=True)
    dtc = (g - dot) / den
    draw = dtc * inside
    cond = inside.sum(2, keepdims=True) * RAW_EPS / den
    rowscale = (np.abs(g).max(2, keepdims=True) + np.abs(dot)) / den
    gW = np.empty_like(W)
    gW_edge = np.empty_like(W)
    flip = np.abs(dtc) * edge
    for kk in range(c):
        gW[kk, :, :c] = draw[:, kk, :].T @ x
        gW[kk, :, c:] = draw[:, kk, :].sum(0)[:, None] * cm[kk][None]
        gW_edge[kk, :, :c] = flip[:, kk, :].T @ np.abs(x)
        gW_edge[kk, :, c:] = flip[:, kk, :].sum(0)[:, None] * np.abs(cm[kk])[None]
    r.update(draw=draw, draw_bound=np.broadcast_to((1e-4 + 3.0 * cond) * rowscale, draw.shape), grad_W=gW,
             grad_W_edge=gW_edge)
    return r


def region_shares(r):
    """(below, inside, above, edge) shares of a sig_t_mean result."""
    return tuple(float(r[k].mean()) for k in ("below", "inside", "above", "edge"))


# ---- correct_logits -------------------------------------------------------------------------------------------------------
def correct_logits(logits, ins_T, E, lam, g=None):
    """logits (B, C, N), ins_T (B*N, C, C), E (C, C) of any sign, lam as the kernel sees it (a C float) -> dict:
    out (B, C, N), s (B*N, C), scale, and with g (B, C, N): grad_logits, grad_ins_T, grad_ema_t, grad_ema_t_abs (the summed
    magnitudes of each entry's terms), grad_ema_t_tile_abs (the summed magnitudes of the 32-point tiles' sums), gscale."""
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
    r.update(grad_logits=gl.reshape(B, N, c).transpose(0, 2, 1), grad_ins_T=(1.0 - lam) * dv, grad_ema_t=lam * dv.sum(0),
             grad_ema_t_abs=lam * np.abs(dv).sum(0),
             grad_ema_t_tile_abs=lam * np.abs(np.add.reduceat(dv, np.arange(0, B * N, TILE), axis=0)).sum(0), gscale=np.abs(go).max() * np.abs(v).max() / smin)
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


def sig_forward_ratio(got, ref):
    """Every entry (clip is continuous: the edge entries too), the row sums, and the all-low head's 1/17."""
    got = np.asarray(got, dtype=np.float64)
    want = ref["out"]
    rows = worst(np.abs(got.sum(2) - 1.0), 32 * U)       # 16 additions in den, the reciprocal, 17 products
    low = ref["below"].all(2)                             # rows that clamp low as a whole: 17 equal entries
    flat = worst(np.abs(got[low] - 1.0 / C), 17 * 2 * U / C)
    return max(worst(np.abs(got - want), 1e-5 * np.abs(want) + 2e-5), rows, flat)


def draw_ratio(got, ref):
    """Every non-edge entry; an exact zero wherever the reference is outside the clamp."""
    ne = ~ref["edge"]
    return worst(np.abs(np.asarray(got, dtype=np.float64) - ref["draw"])[ne], (ref["draw_bound"] * ref["inside"])[ne])


def grad_W_ratio(got, ref, pts, base=None):
    """base: what the buffer held before the call (the entry point adds).  The edge entries' possible contributions are taken
    off the error (|err| <= bound + edge is the same statement), so the figure says how much of the bound the sums use."""
    want = ref["grad_W"]
    top = np.abs(want).max()
    bound = GRAD_W_TOL_LARGE * top if pts >= LARGE_PTS else GRAD_W_TOL * np.abs(want) + GRAD_W_TOL * top
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
    r_i = max(worst(np.abs(gi - wi)[live], (1e-4 * np.abs(wi) + 1e-4 * top)[live]),
              worst(np.abs(gi - wi)[~live], 1e-5 * np.abs(wi)[~live]))
    wE, rows = ref["grad_ema_t"], live.all(0)
    top = np.abs(wE[rows]).max() if rows.any() else 0.0
    bound = np.where(rows[:, None], GRAD_E_TOL_LARGE * top if pts >= LARGE_PTS else GRAD_E_TOL * np.abs(wE) + GRAD_E_TOL * top,
                     1e-5 * ref["grad_ema_t_abs"]) + atomic_adds * U * ref["grad_ema_t_tile_abs"]
    if base_E is not None:
        base_E = np.asarray(base_E, dtype=np.float64)
        wE, bound = wE + base_E, bound + 2 * U * (np.abs(base_E) + np.abs(wE))
    return r_l, r_i, worst(np.abs(gE - wE), bound)


# ---- input builders -------------------------------------------------------------------------------------------------------
def sig_inputs(b, n, seed=0, gain=8.0, all_low_head=ALL_LOW_HEAD):
    """p = softmax(2 randn), cm = softmax(randn), W uniform in +-gain / sqrt(2C) (nn.Linear's default init is gain = 1: no raw
    value reaches the upper clamp there); head `all_low_head` is -|W|, so its whole row clamps low at every point.
    Also g, the upstream gradient of the output."""
    rng = np.random.default_rng(seed)
    p = softmax(rng.standard_normal((b, C, n)) * 2, 1).astype(np.float32)
    cm = softmax(rng.standard_normal((C, C)), 1).astype(np.float32)
    W = (rng.uniform(-1.0, 1.0, (C, C, 2 * C)) * gain / np.sqrt(2 * C)).astype(np.float32)
    if all_low_head is not None:
        W[all_low_head] = -np.abs(W[all_low_head])
    g = rng.standard_normal((b * n, C, C)).astype(np.float32)
    return p, cm, W, g


def correct_inputs(b, n, seed=1, zero_points=()):
    """logits, ins_T and E of both signs, not normalised, and the upstream gradient.  zero_points: flat point ids whose
    ins_T row ZERO_ROW is exactly zero, together with E's row ZERO_ROW (v = 0 there for every lam: the s <= 1e-12 branch)."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((b, C, n)) * 2).astype(np.float32)
    ins_T = rng.standard_normal((b * n, C, C)).astype(np.float32)
    E = rng.standard_normal((C, C)).astype(np.float32)
    g = rng.standard_normal((b, C, n)).astype(np.float32)
    if len(zero_points):
        E[ZERO_ROW] = 0.0
        ins_T[list(zero_points), ZERO_ROW] = 0.0
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
