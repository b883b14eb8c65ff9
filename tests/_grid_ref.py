"""A NumPy restatement of the uniform grid of geot_amd/csrc/knn_grid.{h,hip}, used as a CLASSIFIER only.

Each query of knn_grid_kernel and ball_grid_kernel picks its branch from its data: how many records sit in the 3 x 3 x 3
block of cells around it, how many fall inside the certified radius, whether twelve halvings find a threshold, how many
rings the general loop needs.  This module restates that arithmetic in fp32, operation for operation (the library is
built with -ffp-contract=off, so NumPy's float32 gives the same bits), and names the branch of every query.  It never
produces an expected RESULT -- those come from the CPU oracle -- so a mistake here can only fail the census of
test_grid_search_cpu.py; it cannot make a wrong kernel pass.

It also holds the inputs the CPU census and the GPU tests share: the clouds, the queries and the cases with the classes
each is meant to reach.  Every kernel constant comes from geot_knn_grid_plan / geot_ball_grid_plan.
"""
import ctypes

import numpy as np

F = np.float32
INF = F(np.inf)

KNN_PLAN_FIELDS = ("G", "gmax", "slots", "kmin", "kmax", "waves", "sort_max")
BALL_PLAN_FIELDS = ("gmax", "slots", "waves")


def knn_plan(lib, b, nq, nr, k):
    """geot_knn_grid_plan as a dict, or None where the sizes do not take the grid"""
    out = (ctypes.c_longlong * len(KNN_PLAN_FIELDS))()
    if lib.geot_knn_grid_plan(int(b), int(nq), int(nr), int(k), out, len(KNN_PLAN_FIELDS)) != 1:
        return None
    return dict(zip(KNN_PLAN_FIELDS, (int(v) for v in out)))


def ball_plan(lib, b, n, m, radius, nsample):
    """geot_ball_grid_plan as a dict, or None"""
    out = (ctypes.c_longlong * len(BALL_PLAN_FIELDS))()
    if lib.geot_ball_grid_plan(int(b), int(n), int(m), float(radius), int(nsample), out, len(BALL_PLAN_FIELDS)) != 1:
        return None
    return dict(zip(BALL_PLAN_FIELDS, (int(v) for v in out)))


# ---- the grid -------------------------------------------------------------------------------------------------------
class Grid:
    """kg_grid + the counting sort of one cloud: lo, h, inv_h, dim, ok; per reference point its cell coordinates; start
    (exclusive scan of the x-fastest cell counters) and rec (reference indices in cell order, ascending inside a cell:
    the kernel's arrival order differs, the SET of a range does not)."""


def box(ref):
    """kg_bbox_kernel: per component the smallest and the largest value that is not NaN (NaN where there is none)"""
    lo, hi = np.full(3, np.nan, F), np.full(3, np.nan, F)
    for a in range(3):
        v = ref[:, a]
        v = v[v == v]
        if v.size:
            lo[a], hi[a] = v.min(), v.max()
    return lo, hi


def kg_grid(lo, hi, gtarget, min_h=F(0), gmax=32):
    g = Grid()
    with np.errstate(all="ignore"):
        ext = (hi - lo).astype(F)
        ext[~(ext >= 0)] = F(0)                                       # empty cloud / NaN
        mx = F(max(F(0), ext[0], ext[1], ext[2]))
        ok = bool(mx > 0 and mx < INF)
        if min_h > 0:
            f = F(mx / F(min_h)) if ok else F(1)
            gtarget = int(gmax) if f >= F(gmax) else (int(f) if f >= 1 else 1)
        g.lo, g.ok, g.gtarget = lo.astype(F), ok, int(gtarget)
        g.h = F(mx / F(gtarget)) if ok else INF
        g.inv_h = F(F(gtarget) / mx) if ok else F(0)
        g.dim = [min(max(int(F(ext[a] * g.inv_h)) + 1, 1), int(gtarget)) if ok else 1 for a in range(3)]
    return g


def kg_cell1(p, lo, inv_h, dim):
    """cell of coordinates p (array) on one axis; NaN -> 0"""
    with np.errstate(all="ignore"):
        f = ((p.astype(F) - F(lo)).astype(F) * F(inv_h)).astype(F)
        c = np.minimum(f, F(dim - 1))
        return np.where(f >= 0, np.nan_to_num(c, nan=0.0), 0).astype(np.int64)   # f >= 0 is false for NaN


def cells_of(g, pts):
    return np.stack([kg_cell1(pts[:, a], g.lo[a], g.inv_h, g.dim[a]) for a in range(3)], 1)


def build_grid(ref, gtarget, min_h=F(0), gmax=32):
    lo, hi = box(ref)
    g = kg_grid(lo, hi, gtarget, F(min_h), gmax)
    g.cells = cells_of(g, ref)
    dx, dy, dz = g.dim
    lin = (g.cells[:, 2] * dy + g.cells[:, 1]) * dx + g.cells[:, 0]
    g.start = np.concatenate([[0], np.cumsum(np.bincount(lin, minlength=dx * dy * dz))]).astype(np.int64)
    g.rec = np.argsort(lin, kind="stable")
    return g


def row_ranges(g, c):
    """the nine record ranges [s, e) of the 3 x 3 x 3 block around cell c, rows in the kernel's order (lane = row)"""
    dx, dy, dz = g.dim
    cx, cy, cz = (int(v) for v in c)
    out = []
    for lane in range(9):
        y, z = cy + lane % 3 - 1, cz + lane // 3 - 1
        if 0 <= y < dy and 0 <= z < dz:
            base = (z * dy + y) * dx
            out.append((int(g.start[base + max(cx - 1, 0)]), int(g.start[base + min(cx + 1, dx - 1) + 1])))
        else:
            out.append((0, 0))
    return out


def slot_count(ranges):
    return sum((e - s + 63) >> 6 for s, e in ranges)


def rmax_of(g, c):
    return max(max(int(c[a]), g.dim[a] - 1 - int(c[a])) for a in range(3))


def face_bound(g, q, c, r):
    """distance from q to the nearest face of the (2r+1)^3 block that still has cells behind it, minus the h/1000 slack
    (inf when the block covers the grid, and for a NaN query)"""
    with np.errstate(all="ignore"):
        b = INF
        for a in range(3):
            ca, d = int(c[a]), g.dim[a]
            if ca - r > 0:
                b = np.fmin(b, F(q[a] - F(g.lo[a] + F(F(ca - r) * g.h))))
            if ca + r < d - 1:
                b = np.fmin(b, F(F(g.lo[a] + F(F(ca + r + 1) * g.h)) - q[a]))
        return F(np.fmax(F(b - F(g.h * F(1e-3))), F(0)))      # fminf / fmaxf drop a NaN operand: a NaN query leaves inf


def sqdist(q, ref):
    """sqdist3 in the exact mode: ((dx * dx) + (dy * dy)) + (dz * dz), fp32"""
    with np.errstate(all="ignore"):
        d = (q[None, :].astype(F) - ref.astype(F)).astype(F)
        return ((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F) + (d[:, 2] * d[:, 2]).astype(F)


# ---- kNN classes ----------------------------------------------------------------------------------------------------
FAST_CLASSES = ("rings_only", "slots_overflow", "nan_query", "zero_radius", "direct", "bisect_found", "bisect_gave_up",
                "kth_outside_block", "rmax1")
RING_CLASSES = ("r1_bound", "r2_3_bound", "r4plus_bound", "r1_covered", "r2_3_covered", "r4plus_covered")


def _fast_class(d_block, slots, b2, k, plan, rmax, nan_q):
    """the select fast path of knn_grid_kernel for one query: its label, and True when the query is answered there"""
    if slots > plan["slots"]:
        return "slots_overflow", False
    if not b2 > 0:
        return "zero_radius", False
    if nan_q:                                           # every distance is NaN: no probe counts anything
        return "nan_query", False
    with np.errstate(all="ignore"):
        def count_le(tau):
            return int(np.count_nonzero(d_block <= tau))
        tau = b2
        c = count_le(tau)
        found = k <= c <= 64
        gave_up = False
        if c > 64:
            lo_t, hi_t = F(0), b2
            for _ in range(12):
                tau = F(F(0.5) * F(lo_t + hi_t))
                c = count_le(tau)
                if c < k:
                    lo_t = tau
                elif c > 64:
                    hi_t = tau
                else:
                    found = True
                    break
            gave_up = not found
    if rmax <= 1:
        return "rmax1", found
    if found:
        return ("direct" if tau == b2 else "bisect_found"), True
    return ("bisect_gave_up" if gave_up else "kth_outside_block"), False


def _ring_class(g, q, c, d_all, cheb, k, rmax, scale):
    """kg_rings for one query: after ring r, tau = the k-th smallest d2 inside the (2r+1)^3 block; the loop stops on
    r >= rmax (covered) or tau < bound^2 * 0.99999 (bound).  scale multiplies the threshold (marginality)."""
    finite = d_all < INF                                # NaN and +inf distances are never inserted
    r = 1
    while True:
        inside = d_all[(cheb <= r) & finite]
        tau = np.partition(inside, k - 1)[k - 1] if inside.size >= k else INF
        if r >= rmax:
            why = "covered"
            break
        bound = face_bound(g, q, c, r)
        with np.errstate(all="ignore"):
            if tau < F(F(F(bound * bound) * F(0.99999)) * F(scale)):
                why = "bound"
                break
        r += 1
    return ("r1_" if r == 1 else "r2_3_" if r <= 3 else "r4plus_") + why


def classify_knn(ref, qry, k, plan):
    """(fast, ring, marginal, grid) of every query of one cloud.  fast: a FAST_CLASSES label; ring: a RING_CLASSES label,
    or '' where the fast path answers; marginal: a label changes when the certified radius (b2, and the ring stop's
    threshold) is scaled by 1 +- 1e-5."""
    g = build_grid(ref, plan["G"], gmax=plan["gmax"])
    qc = cells_of(g, qry)
    fast, ring, marg = [], [], []
    for j in range(qry.shape[0]):
        q, c = qry[j].astype(F), qc[j]
        rmax = rmax_of(g, c)
        d_all = sqdist(q, ref)
        cheb = np.abs(g.cells - c[None, :]).max(1)
        labels = []
        for scale in (1.0, 1.0 + 1e-5, 1.0 - 1e-5):
            if not plan["kmin"] <= k <= plan["kmax"]:
                f, done = "rings_only", False
            else:
                ranges = row_ranges(g, c)
                members = np.concatenate([g.rec[s:e] for s, e in ranges]) if slot_count(ranges) else np.zeros(0, np.int64)
                b2 = F(3.0e38)
                if rmax > 1:
                    bound = face_bound(g, q, c, 1)
                    with np.errstate(all="ignore"):
                        b2 = F(np.fmin(F(F(F(bound * bound) * F(0.9999)) * F(scale)), F(3.0e38)))
                f, done = _fast_class(d_all[members], slot_count(ranges), b2, k, plan, rmax, bool(np.isnan(q).any()))
            labels.append((f, "" if done else _ring_class(g, q, c, d_all, cheb, k, rmax, scale)))
        fast.append(labels[0][0])
        ring.append(labels[0][1])
        marg.append(labels[1] != labels[0] or labels[2] != labels[0])
    return np.array(fast), np.array(ring), np.array(marg), g


# ---- ball classes ---------------------------------------------------------------------------------------------------
BALL_CLASSES = ("zero_hits", "short_fill", "direct", "bisect", "dense_insertion_le", "dense_insertion_gt")


def classify_ball(ref, qry, radius, nsample, plan):
    """ball_grid_kernel's branch per query of one cloud: cells of edge >= 1.0001 radius (the documented contract),
    the slot count of the 3 x 3 x 3 block and the hit count H inside it"""
    radius = F(radius)
    g = build_grid(ref, 1, min_h=F(radius * F(1.0001)), gmax=plan["gmax"])
    r2 = F(radius * radius)
    qc = cells_of(g, qry)
    out = []
    for j in range(qry.shape[0]):
        ranges = row_ranges(g, qc[j])
        slots = slot_count(ranges)
        members = np.concatenate([g.rec[s:e] for s, e in ranges]) if slots else np.zeros(0, np.int64)
        with np.errstate(all="ignore"):
            H = int(np.count_nonzero(sqdist(qry[j].astype(F), ref[members]) < r2))
        if slots > plan["slots"]:
            out.append("dense_insertion_le" if H <= nsample else "dense_insertion_gt")
        elif H == 0:
            out.append("zero_hits")
        elif H < nsample:
            out.append("short_fill")
        else:
            out.append("direct" if H <= 64 else "bisect")
    return np.array(out), g


# ---- geot_spatial_order ---------------------------------------------------------------------------------------------
def morton_keys(ref, gmax):
    """Morton cell of every point on the gmax^3 grid over the cloud's box (kg_morton15: x in bits 0, 3, ..)"""
    g = build_grid(ref, gmax, gmax=gmax)
    key = np.zeros(ref.shape[0], np.int64)
    for bit in range(5):
        for a in range(3):
            key |= ((g.cells[:, a] >> bit) & 1) << (3 * bit + a)
    return key


# ---- shared inputs --------------------------------------------------------------------------------------------------
CLOUDS = ("volume", "sphere", "clusters", "line", "lattice", "dups", "outlier", "slab", "identical", "naninf")
NQ = 241            # per cloud; not a multiple of the queries per workgroup (asserted against the plan)
SAME_POINT = (0.25, -0.5, 0.0)


def make_clouds(nr, seed=1):
    """(10, nr, 3) fp32: every cloud has its own box"""
    rng = np.random.default_rng(seed)
    u = rng.random((nr, 3)).astype(F)
    sph = rng.standard_normal((nr, 3))
    sph = (sph / np.linalg.norm(sph, axis=1, keepdims=True)).astype(F)
    clus = (rng.integers(0, 5, (nr, 1)) * 0.2 + rng.standard_normal((nr, 3)) * 0.003).astype(F)
    line = np.zeros((nr, 3), F)
    line[:, 0] = np.linspace(-1, 1, nr, dtype=F)
    side = int(np.ceil(np.sqrt(nr)))
    gx, gy = np.meshgrid(np.arange(side, dtype=F), np.arange(side, dtype=F))
    lattice = np.stack([gx.ravel()[:nr] / 64, gy.ravel()[:nr] / 64, np.zeros(nr, F)], 1).astype(F)      # exact ties
    dup = u.copy()
    dup[nr // 2:] = dup[rng.integers(0, nr // 2, nr - nr // 2)]
    outl = (u * F(0.01)).astype(F)
    outl[7] = (50.0, -30.0, 10.0)
    slab = u.copy()
    slab[:, 2] *= F(0.01)
    same = np.tile(np.array(SAME_POINT, F), (nr, 1))
    bad = rng.random((nr, 3)).astype(F)
    bad[5] = np.nan                                                    # a NaN point: in no box, in cell 0
    bad[9, 0] = np.inf                                                 # an infinite extent: ok == false, one cell
    clouds = dict(volume=u, sphere=sph, clusters=clus, line=line, lattice=lattice, dups=dup, outlier=outl, slab=slab,
                  identical=same, naninf=bad)
    return np.ascontiguousarray(np.stack([clouds[c] for c in CLOUDS]).astype(F))


def make_knn_queries(ref, seed=2):
    """(10, 241, 3): the first 150 references, 30 from N(0, 3^2) (mostly outside the box), the last 60 references + 1e-3,
    one NaN query"""
    rng = np.random.default_rng(seed)
    b = ref.shape[0]
    far = (rng.standard_normal((b, 30, 3)) * 3).astype(F)
    nanq = np.full((b, 1, 3), np.nan, F)
    q = np.concatenate([ref[:, :150], far, ref[:, -60:] + F(1e-3), nanq], 1).astype(F)
    assert q.shape[1] == NQ
    return np.ascontiguousarray(q)


def make_ball_queries(ref, radius, seed=3):
    """(10, 241, 3): the first 120 references; references 150..169 moved by fl(radius) along z (EXACTLY radius away from
    their reference wherever its z is 0: line, lattice, identical -- d2 < r2 is strict); 24 points up to 0.9 radius
    outside the box, four on each side; 30 from N(0, 3^2); the last 46 references + 1e-3; one NaN query"""
    rng = np.random.default_rng(seed)
    b = ref.shape[0]
    radius = F(radius)
    exact = ref[:, 150:170].copy()
    exact[:, :, 2] = (exact[:, :, 2] + radius).astype(F)
    outside = np.zeros((b, 24, 3), F)
    for c in range(b):
        lo, hi = box(ref[c])
        lo, hi = np.nan_to_num(lo, nan=0.0, posinf=1.0, neginf=-1.0), np.nan_to_num(hi, nan=0.0, posinf=1.0, neginf=-1.0)
        for s in range(24):
            a, up = (s // 4) % 3, s // 12
            p = (lo + (hi - lo) * rng.random(3)).astype(F)
            off = F(0.9) * radius * F(rng.random())
            p[a] = hi[a] + off if up else lo[a] - off
            outside[c, s] = p
    far = (rng.standard_normal((b, 30, 3)) * 3).astype(F)
    nanq = np.full((b, 1, 3), np.nan, F)
    q = np.concatenate([ref[:, :120], exact, outside, far, ref[:, -46:] + F(1e-3), nanq], 1).astype(F)
    assert q.shape[1] == NQ
    return np.ascontiguousarray(q)


NR = 2048           # the eligibility floor of both grid searches (asserted in the CPU test)
KNN_KS = (1, 3, 7, 8, 16, 33, 48, 49, 64)
BALL_CASES = ((0.02, 8), (0.1, 32), (0.3, 64), (2.5, 32), (0.1, 1), (0.1, 64))
MIN_PER_CLASS = 5
MARGINAL_CAP = 0.01

# The classes each case is meant to reach: (cloud, class) -> at least MIN_PER_CLASS queries that are not marginal; the
# cloud "any" counts over the whole batch (there is one NaN query per cloud).  Fast-path labels and ring labels share one
# table; test_grid_search_cpu.py prints the whole census and asserts these cells.
_RINGS_ONLY = [(c, "rings_only") for c in CLOUDS]
_KNN_INTENDED_2048 = {
    1: _RINGS_ONLY + [("volume", "r1_bound"), ("volume", "r4plus_bound"), ("volume", "r4plus_covered"),
                      ("outlier", "r2_3_bound"), ("identical", "r1_covered"), ("naninf", "r1_covered")],
    3: _RINGS_ONLY + [("volume", "r1_bound"), ("volume", "r2_3_bound"), ("volume", "r4plus_bound"),
                      ("volume", "r4plus_covered"), ("dups", "r2_3_bound")],
    7: _RINGS_ONLY + [("volume", "r1_bound"), ("volume", "r2_3_bound")],
    8: [("volume", "direct"), ("volume", "kth_outside_block"), ("volume", "r2_3_bound"), ("clusters", "bisect_found"),
        ("dups", "direct"), ("outlier", "slots_overflow"), ("outlier", "r1_bound"), ("identical", "slots_overflow"),
        ("identical", "r1_covered"), ("naninf", "slots_overflow"), ("any", "nan_query")],
    16: [("clusters", "bisect_found"), ("clusters", "bisect_gave_up"), ("clusters", "slots_overflow"),
         ("clusters", "kth_outside_block"), ("volume", "direct"), ("dups", "direct"), ("lattice", "bisect_found"),
         ("any", "nan_query")],
    33: [("volume", "direct"), ("volume", "bisect_found"), ("volume", "kth_outside_block"), ("volume", "r2_3_bound"),
         ("volume", "r4plus_covered"), ("clusters", "slots_overflow"), ("dups", "direct"), ("any", "nan_query")],
    48: [("volume", "direct"), ("volume", "bisect_found"), ("volume", "kth_outside_block"), ("line", "slots_overflow"),
         ("slab", "slots_overflow"), ("any", "nan_query")],
    49: _RINGS_ONLY + [("volume", "r1_bound"), ("volume", "r2_3_bound"), ("volume", "r4plus_covered")],
    64: _RINGS_ONLY + [("volume", "r1_bound"), ("volume", "r2_3_covered"), ("sphere", "r2_3_bound")],
}
KNN_INTENDED = {(NR, k): v for k, v in _KNN_INTENDED_2048.items()}
# one more reference point: record ranges that are multiples of nothing
KNN_INTENDED[(NR + 1, 3)] = _RINGS_ONLY + [("volume", "r1_bound"), ("volume", "r2_3_bound"), ("volume", "r4plus_covered")]
KNN_INTENDED[(NR + 1, 16)] = [("volume", "direct"), ("volume", "kth_outside_block"), ("clusters", "bisect_found"),
                              ("clusters", "slots_overflow"), ("any", "nan_query")]
KNN_CASES = tuple(KNN_INTENDED)
BALL_INTENDED = {
    (0.02, 8): [("clusters", "bisect"), ("clusters", "zero_hits"), ("line", "direct"), ("volume", "zero_hits"),
                ("volume", "short_fill"), ("outlier", "dense_insertion_gt"), ("outlier", "dense_insertion_le")],
    (0.1, 32): [("slab", "direct"), ("slab", "bisect"), ("slab", "short_fill"), ("slab", "zero_hits"),
                ("lattice", "direct"), ("clusters", "dense_insertion_gt"), ("identical", "dense_insertion_gt"),
                ("identical", "dense_insertion_le")],
    (0.3, 64): [("volume", "dense_insertion_gt"), ("volume", "dense_insertion_le"), ("volume", "bisect"),
                ("volume", "short_fill"), ("volume", "zero_hits"), ("line", "bisect")],
    (2.5, 32): [(c, "dense_insertion_gt") for c in CLOUDS] + [("volume", "dense_insertion_le")],
    (0.1, 1): [("volume", "direct"), ("slab", "bisect"), ("volume", "zero_hits"), ("line", "direct")],
    (0.1, 64): [("slab", "direct"), ("slab", "bisect"), ("slab", "short_fill"), ("volume", "short_fill"),
                ("line", "bisect")],
}


# ---- the cases, classified once per process -------------------------------------------------------------------------
_CACHE = {}


def inputs(nr):
    if ("in", nr) not in _CACHE:
        ref = make_clouds(nr)
        _CACHE["in", nr] = (ref, make_knn_queries(ref))
    return _CACHE["in", nr]


def knn_case(lib, nr, k):
    """dict(ref, qry, plan, fast, ring, marginal, grids) of one kNN case, the last four per cloud.  GEOT_NN_IMPL=grid
    must be set: the plan exists only where the grid is taken."""
    key = ("knn", nr, k)
    if key not in _CACHE:
        ref, qry = inputs(nr)
        plan = knn_plan(lib, ref.shape[0], NQ, nr, k)
        assert plan is not None, "not grid-eligible: nr = %d, k = %d" % (nr, k)
        per = [classify_knn(ref[c], qry[c], k, plan) for c in range(ref.shape[0])]
        _CACHE[key] = dict(ref=ref, qry=qry, plan=plan, fast=[p[0] for p in per], ring=[p[1] for p in per],
                           marginal=[p[2] for p in per], grids=[p[3] for p in per])
    return _CACHE[key]


def ball_case(lib, nr, radius, nsample):
    key = ("ball", nr, radius, nsample)
    if key not in _CACHE:
        ref, _ = inputs(nr)
        plan = ball_plan(lib, ref.shape[0], nr, NQ, radius, nsample)
        assert plan is not None, "not grid-eligible: radius = %g, nsample = %d" % (radius, nsample)
        qry = make_ball_queries(ref, radius)
        per = [classify_ball(ref[c], qry[c], radius, nsample, plan) for c in range(ref.shape[0])]
        _CACHE[key] = dict(ref=ref, qry=qry, plan=plan, cls=[p[0] for p in per], grids=[p[1] for p in per])
    return _CACHE[key]


def census(labels_per_cloud, keep_per_cloud=None):
    """{(cloud, label): count} over the queries kept (all when keep is None), with the batch-wide ("any", label) too"""
    out = {}
    for c, name in enumerate(CLOUDS):
        lab = labels_per_cloud[c] if keep_per_cloud is None else labels_per_cloud[c][keep_per_cloud[c]]
        for v, n in zip(*np.unique(lab, return_counts=True)):
            if v:
                out[name, str(v)] = out.get((name, str(v)), 0) + int(n)
                out["any", str(v)] = out.get(("any", str(v)), 0) + int(n)
    return out


# ---- a cloud on which the ring loop's h / 1000 slack decides the answer ----------------------------------------------
# A point is given its cell by fl(fl(p - lo) * inv_h), a block face sits at fl(lo + fl(c * h)): with the box a few
# extents away from the origin the two disagree by a rounding of the COORDINATE, and a point p just below face c is
# counted to cell c.  The query q is the last value of cell c - 2, so the 3-cell block ends at face c, bound = face - q is
# one cell edge, and p, outside the block, is nearer than bound by more than the 0.99999 of the stop test allows for.
# With a visited point v whose squared distance lies between d2(p) and bound^2 * 0.99999, the search may only stop at
# ring 1 if the slack is there.  Everything is found by scanning fp32 neighbours, nothing is tuned to a kernel's output.
FACE_BOX = (0.80929834, 2.2929325)      # one of many boxes (a random search finds one in ~400) where such p, q exist
FACE_K = 1                              # G = 32 at 2048 points: the smallest cells, the bound nearest to the rounding


def _down(x):
    return np.nextafter(F(x), F(-np.inf))


def _up(x):
    return np.nextafter(F(x), F(np.inf))


def make_face_rounding_case(nr=NR, G=32):
    """dict(ref (1, nr, 3), qry (1, 8, 3), c, p_index, v_index, d2p, d2v, thr_mut, thr): query 0 is the designed one"""
    lo, hi = F(FACE_BOX[0]), F(FACE_BOX[1])
    mx = F(hi - lo)
    h, inv_h = F(mx / F(G)), F(F(G) / mx)

    def cell(x):
        return int(kg_cell1(np.array([x], F), lo, inv_h, G)[0])

    def face(c):
        return F(lo + F(F(c) * h))
    found = None
    for c in range(5, G - 1):
        p = face(c)
        while cell(_down(p)) >= c:
            p = _down(p)
        q = face(c - 1)
        while cell(q) > c - 2:
            q = _down(q)
        while cell(_up(q)) <= c - 2:
            q = _up(q)
        if cell(p) < c or cell(q) != c - 2:
            continue
        bound = F(face(c) - q)                                        # without the slack
        thr_mut = F(F(bound * bound) * F(0.99999))
        with_slack = F(np.fmax(F(bound - F(h * F(1e-3))), F(0)))
        thr = F(F(with_slack * with_slack) * F(0.99999))
        d2p = F(F(p - q) * F(p - q))
        if d2p < thr_mut:
            # v = (q - a, b, 0): a^2 a little under d2p, b^2 lifts the sum into (d2p, thr_mut]
            a = F(p - q)
            for _ in range(64):
                a = _down(a)
                xv = F(q - a)
                dx2 = F(F(q - xv) * F(q - xv))
                if not dx2 < d2p:
                    continue
                for b in np.geomspace(1e-7, 1e-3, 4000).astype(F):
                    d2v = F(dx2 + F(b * b))
                    if d2p < d2v <= thr_mut and not d2v < thr and c - 3 <= cell(xv) <= c - 1:
                        found = dict(c=c, p=p, q=q, v=np.array([xv, b, 0], F), d2p=d2p, d2v=d2v, thr_mut=thr_mut, thr=thr)
                        break
                if found:
                    break
        if found:
            break
    assert found is not None, "no face-rounding triple in this box"
    c, p, q = found["c"], found["p"], found["q"]
    n_low = (nr - 2) * 2 // 3
    low = np.linspace(lo, face(c - 5), n_low, dtype=F)                # cells <= c - 5: behind v, outside the block
    high = np.linspace(F(p + h / 4), hi, nr - 2 - n_low, dtype=F)     # beyond p
    low[0], high[-1] = lo, hi
    ref = np.zeros((nr, 3), F)
    ref[:n_low, 0] = low
    ref[n_low] = found["v"]
    ref[n_low + 1, 0] = p
    ref[n_low + 2:, 0] = high
    qs = [q]
    for _ in range(7):
        qs.append(_down(qs[-1]))
    qry = np.zeros((8, 3), F)
    qry[:, 0] = qs
    found.update(ref=ref[None], qry=qry[None], v_index=n_low, p_index=n_low + 1)
    return found
