"""fp64 numpy restatement of the teacher-student contrastive loss (include/geot_hip.h "ABI 24", geot_amd/utils/
cluster_contrastloss.py steps 1-6), written from the contract: nothing of geot_amd is imported.  The device draw is
tests/_sample_draw_ref.py's keyed bijection.  The reference class forces fp32 (.float() at :1224 and :1259), so an fp64
referee has to be this restatement, not a run of the class in double.

    select(score, th, s, perms=None, seed=None, counter=None)   anchors, per-cloud counts, A, bank rows, the permutations
    loss_grad(feat_s, feat_t, anchors, bank, g=1.0)             loss, l_a, dense gradient, x^, t^, |x|
    enqueue(that, rows, bank, ptr, s)                           the bank and the pointer after the call
    Reference(s, d, bank)                                       the state over consecutive calls
    bounds(...)                                                 absolute error bounds of an fp32 implementation

Error bounds.  u = 2^-24 (fp32 unit roundoff), first order in u, every term a count of operations, none fitted:
    e_n   one component of x^ or t^, relative: D fused terms of the sum of squares halve under the root ((D + 1) / 2 u),
          the root and the quotient one u each, rounded up:                                   e_n = (D / 2 + 3) u
    e_u   one scaled product u_aj, absolute: both factors perturbed (2 e_n) and D accumulated terms (D u) on a sum of
          |x^_c t^_c| <= 1, the division by tau (u |u_aj| <= u / tau) and tau = 0.1 held in fp32 or folded into a
          multiplication (2 u / tau):                                                          e_u = (2 e_n + (D + 3) u) / tau
    e_s   a shifted value u_aj - max: two such values and the rounding of a difference <= 2 / tau:  e_s = 2 e_u + 2 u / tau
    e_e   one exponential, relative: expm1(e_s) from its argument and 2 ulp = 4 u from expf (the device library and the
          vectorised host one both document <= 1 ulp; 2 leaves room for either)
    e_z   Z_a, relative: e_e, N = A + 4S summed terms in any order (N u), and R rescalings of the running sum where the
          running maximum moves: each is one expf (4 u), two rounded differences in its argument (2 u / tau each side of
          the identity exp(a - b) exp(b - c) = exp(a - c)), a multiplication and an addition (2 u), rounded up to
          (8 + 2 / tau) u; R = ceil(N / 16) + 16: tiles of at least 16 keys, at most 16 chunk merges
    e_l   l_a, absolute: (tau / tau_b) (e_s + e_z + 8 u (2 / tau + log N)): log(1 + e) <= e, logf at 2 ulp of log Z <=
          log N, the two differences and the product on values <= 2 / tau + log N
    loss  e_l + (A + 2) u l_max, l_max = (tau / tau_b) (2 / tau + log N): A terms in any order and the quotient
    e_g   one component of t^_a - W_a / Z_a, absolute: W / Z is a convex combination of unit-row components, its weights
          carry e_z each way, its rows e_n; t^ carries e_n:                                    e_g = 2 e_n + 2 e_z + 4 u
    grad  per row with Y = 2 g / (A tau_b) >= |dy| and e_dy = (Y / 2) (e_g + 8 u):
          |x| >= 1e-12: ((1 + sqrt D) e_dy + Y (2 e_n + (D + 6) u) + 2 Y (D / 2 + 3) u) / |x|
          -- dy_c, the dot product's share sqrt(D) e_dy, x^ perturbed twice, D accumulated terms, three roundings on each of
          two terms, and the quotient by a norm of relative error (D / 2 + 3) u on |dx| <= 2 Y / |x|;
          otherwise (e_dy + 2 u Y) / 1e-12.  Rows that are no anchor: 0 (an exact zero is demanded).
    bank  a written row: t^ (e_n) normalised once more (2 e_n for its norm and quotient, 4 u): 3 e_n + 4 u; every other
          row and the pointer: 0.
"""
import math

import numpy as np

from _sample_draw_ref import _without_replacement

U = 2.0 ** -24
EPS = 1e-12
TAU = float(np.float32(0.1))
TAU_B = 1.0


# tests/golden/contrast_loss_ref.npz: shapes, the candidate counts per call and cloud, and the pointer the sequence starts at.
# With S = 16 (bank 64) the six calls meet K < S, K = S, K > S and K = 0 in a cloud; call 0 enqueues 7 < S rows (50 -> 57),
# call 1 passes the end (57 + 16 > 64: rows [48, 64), pointer 0), calls 2-5 enqueue 16 each and the last one ends at 64 exactly.
FIXTURE = dict(seed=20240611, B=2, P=96, D=128, S=16, th=0.9, ptr0=50,
               K=((3, 4), (16, 40), (96, 2), (16, 16), (20, 0), (9, 10)))


def fixture_inputs(call):
    """(feat_s, score, feat_t) fp32 of fixture call `call`, from numpy's default_rng((seed, call)).  K[call][b] points of
    cloud b score in [0.9, 1) -- the first of them exactly fp32(0.9) -- all others in [0, 0.9)."""
    f = FIXTURE
    rng = np.random.default_rng((f["seed"], call))
    b, p, d = f["B"], f["P"], f["D"]
    feat_s = rng.standard_normal((b, p, d)).astype(np.float32)
    feat_t = (0.5 * feat_s + rng.standard_normal((b, p, d))).astype(np.float32)
    score = (rng.random((b, p)) * 0.89).astype(np.float32)
    for c in range(b):
        k = f["K"][call][c]
        where = rng.permutation(p)[:k]
        score[c, where] = (0.9 + 0.0999 * rng.random(k)).astype(np.float32)
        if k:
            score[c, where[0]] = np.float32(0.9)
    assert tuple((score >= np.float32(f["th"])).sum(1)) == tuple(f["K"][call])
    return feat_s, score, feat_t


def fixture_bank():
    """The seeded initial bank, fp32 rows of unit norm up to rounding."""
    f = FIXTURE
    raw = np.random.default_rng((f["seed"], 99)).standard_normal((4 * f["S"], f["D"]))
    return (raw / np.sqrt((raw * raw).sum(1, keepdims=True))).astype(np.float32)


def draw(n, m, seed, d):
    """The first m entries of the keyed permutation of [0, n) with draw id d (geot_sample_draw, n >= m)."""
    if m == 0:
        return np.zeros(0, np.int64)
    return _without_replacement(int(n), int(m), seed, np.asarray([d & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))[0]


def select(score, th, s, perms=None, seed=None, counter=None):
    """score (B, P).  perms: (list of B permutations (at least the first m entries), permutation of [0, A)) or None: the
    device draw with (seed, counter).  -> dict anchors (A,) global ids, m (B,), A, rows (min(A, s),), perm, perm_q."""
    score = np.asarray(score, dtype=np.float32)
    b, p = score.shape
    keep = score >= np.float32(th)           # a NaN compares false
    anchors, ms, used = [], [], []
    for c in range(b):
        cand = np.nonzero(keep[c])[0]
        k = len(cand)
        m = min(k, s)
        perm = np.asarray(perms[0][c], dtype=np.int64)[:m] if perms is not None else draw(k, m, seed, counter + c)
        used.append(perm)
        anchors.append(c * p + cand[perm])
        ms.append(m)
    anchors = np.concatenate(anchors).astype(np.int64) if anchors else np.zeros(0, np.int64)
    a = len(anchors)
    cnt = min(a, s)
    perm_q = np.asarray(perms[1], dtype=np.int64)[:cnt] if perms is not None else draw(a, cnt, seed, counter + b)
    return {"anchors": anchors, "m": np.asarray(ms), "A": a, "rows": perm_q, "perm": used, "perm_q": perm_q}


def normalize(x):
    n = np.sqrt((x * x).sum(-1, keepdims=True))
    return x / np.maximum(n, EPS), n[..., 0]


def loss_grad(feat_s, feat_t, anchors, bank, g=1.0, tau=TAU, tau_b=TAU_B):
    """feat_s, feat_t (B, P, D) point-major.  -> dict loss, ell (A,), grad (B, P, D), xhat, that (A, D), norm (A,), gdir."""
    fs = np.asarray(feat_s, dtype=np.float64)
    ft = np.asarray(feat_t, dtype=np.float64)
    bank = np.asarray(bank, dtype=np.float64)
    d = fs.shape[-1]
    x, t = fs.reshape(-1, d)[anchors], ft.reshape(-1, d)[anchors]
    a = len(anchors)
    grad = np.zeros(fs.shape, dtype=np.float64)
    if a == 0:
        return {"loss": 0.0, "ell": np.zeros(0), "grad": grad, "xhat": x, "that": t, "norm": np.zeros(0), "gdir": x}
    xh, nx = normalize(x)
    th, _ = normalize(t)
    u, v = xh @ th.T / tau, xh @ bank.T / tau
    mu, nu = u.max(1), v.max(1)
    eu, ev = np.exp(u - mu[:, None]), np.exp(v - nu[:, None])
    z = eu.sum(1) + ev.sum(1)
    ell = -(tau / tau_b) * ((np.diag(u) - mu) - np.log(z))
    w = eu @ th + ev @ bank
    gdir = th - w / z[:, None]
    dy = -(g / (a * tau_b)) * gdir
    big = nx >= EPS
    dot = (dy * xh).sum(1, keepdims=True)
    dx = np.where(big[:, None], (dy - xh * dot) / np.maximum(nx, EPS)[:, None], dy / EPS)
    grad.reshape(-1, d)[anchors] = dx
    return {"loss": float(ell.mean()), "ell": ell, "grad": grad, "xhat": xh, "that": th, "norm": nx, "gdir": gdir}


def enqueue(that, rows, bank, ptr, s):
    """-> (bank after, pointer after, the written row range)."""
    bank = np.array(bank, dtype=np.float64)
    cnt = len(rows)
    if cnt == 0:
        return bank, ptr, (0, 0)
    new, _ = normalize(np.asarray(that, dtype=np.float64)[rows])
    size = 4 * s
    if ptr + cnt > size:
        lo, ptr = size - cnt, 0
    else:
        lo, ptr = ptr, (ptr + cnt) % size
    bank[lo:lo + cnt] = new
    return bank, ptr, (lo, lo + cnt)


class Reference:
    """Bank and pointer over consecutive calls."""

    def __init__(self, s, bank, th=0.9):
        self.s, self.th, self.ptr = s, th, 0
        self.bank = np.array(bank, dtype=np.float64)

    def __call__(self, feat_s, score, feat_t, perms=None, seed=None, counter=None, g=1.0):
        sel = select(score, self.th, self.s, perms, seed, counter)
        out = loss_grad(feat_s, feat_t, sel["anchors"], self.bank, g)
        out.update(sel)
        out["bank_before"] = self.bank
        if sel["A"] > 0:
            self.bank, self.ptr, out["written"] = enqueue(out["that"], sel["rows"], self.bank, self.ptr, self.s)
        else:
            out["written"] = (0, 0)
        out["bank"], out["ptr"] = self.bank, self.ptr
        return out


def bounds(d, a, s, norm, g=1.0, tau=TAU, tau_b=TAU_B):
    """Absolute bounds for A = a anchors of dimension d against a bank of 4 s rows; norm (A,): |x| per anchor.
    -> dict loss, ell, grad (A,) per anchor row, bank."""
    n = a + 4 * s
    e_n = (d / 2 + 3) * U
    e_u = (2 * e_n + (d + 3) * U) / tau
    e_s = 2 * e_u + 2 * U / tau
    e_e = math.expm1(e_s) + 4 * U
    r = -(-n // 16) + 16
    e_z = e_e + n * U + r * (8 + 2 / tau) * U
    span = 2 / tau + math.log(n)
    e_l = (tau / tau_b) * (e_s + e_z + 8 * U * span)
    l_max = (tau / tau_b) * span
    e_g = 2 * e_n + 2 * e_z + 4 * U
    out = {"ell": e_l, "loss": e_l + (a + 2) * U * l_max if a else 0.0, "bank": 3 * e_n + 4 * U}
    if a:
        y = 2 * abs(g) / (a * tau_b)
        e_dy = (y / 2) * (e_g + 8 * U)
        norm = np.asarray(norm, dtype=np.float64)
        big = ((1 + math.sqrt(d)) * e_dy + y * (2 * e_n + (d + 6) * U) + 2 * y * (d / 2 + 3) * U) / np.maximum(norm, EPS)
        out["grad"] = np.where(norm >= EPS, big, (e_dy + 2 * U * y) / EPS)
    else:
        out["grad"] = np.zeros(0)
    return out


def grad_bound_dense(shape, anchors, row_bounds):
    """Per-element bound of the dense gradient: the anchor rows' bounds, 0 everywhere else."""
    d = shape[-1]
    out = np.zeros(shape, dtype=np.float64)
    out.reshape(-1, d)[anchors] = np.asarray(row_bounds)[:, None]
    return out


def ratio(err, bound):
    """Largest |err| / bound; where the bound is 0 an exact zero is demanded (inf otherwise)."""
    err, bound = np.abs(np.asarray(err, dtype=np.float64)).ravel(), np.broadcast_to(bound, np.shape(err)).ravel()
    if err.size == 0:
        return 0.0
    if not np.all(np.isfinite(err)):
        return math.inf
    zero = bound == 0
    if np.any(err[zero] != 0):
        return math.inf
    return float((err[~zero] / bound[~zero]).max()) if np.any(~zero) else 0.0
