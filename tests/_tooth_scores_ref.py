"""References for the Teeth3DS challenge scores (geot_tooth_moments, geot_amd/validation.py ToothScores):
(1) the numpy int64 restatement of the moments -- the kernel's integers, bit for bit, skip rules included;
(2) a second, independent fp64 computation of the four scores straight from vertices, labels and predictions, without the
    quantisation and without the moments' layout;
(3) the bound between the two, derived from the resolution and the data."""
import numpy as np

F32 = np.float32
ENTRIES = 21
BIAS = 1 << 30
LIMIT = F32(16384.0)
SCALE = F32(65536.0)


def quantise(points, center):
    """(usable (M,) bool, q (M, 3) int64): d = points - center in fp32, usable iff all |d| < 16384 (a NaN or an infinity is
    not), q = rint(d * 65536), ties to even."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = points.astype(F32) - center.astype(F32)[None]
        usable = (np.abs(d) < LIMIT).all(1)
        q = np.zeros(d.shape, np.int64)
        q[usable] = np.rint(d[usable] * SCALE).astype(np.int64)
    return usable, q


def moments_ref(b, c, points, labels, offsets, scan_ids, center, work, out_offsets, pred, rows=None):
    """geot_tooth_moments on the host: every argument a numpy array as the kernel sees it; rows (b, 21 c + 2) int64 are added
    to / max-combined (default: zeros) and returned."""
    words = ENTRIES * c + 2
    rows = np.zeros((b, words), np.int64) if rows is None else rows
    n_scans, total = len(offsets) - 1, len(points)
    for s, first, count, _ in np.asarray(work).reshape(-1, 4).tolist():
        if not 0 <= s < b:
            continue
        sid = int(scan_ids[s])
        if not 0 <= sid < n_scans:
            continue
        lo, hi = int(offsets[sid]), int(offsets[sid + 1])
        if lo < 0 or hi <= lo or hi > total or hi - lo > 2 ** 31 - 1:
            continue
        if first < 0 or first >= hi - lo or count < 1:
            continue
        end = min(first + count, hi - lo)
        v = np.arange(first, end)
        usable, q = quantise(points[lo + v], center[s])
        lab = labels[lo + v].astype(np.int64)
        prd = pred[int(out_offsets[s]) + v].astype(np.int64)
        row = rows[s]
        row[words - 1] += int((~usable).sum())
        l_in, p_in = usable & (lab >= 0) & (lab < c), usable & (prd >= 0) & (prd < c)
        for side, key, on in ((0, lab, l_in), (10, prd, p_in)):
            at = key[on] * ENTRIES + side
            np.add.at(row, at, 1)
            for a in range(3):
                np.add.at(row, at + 1 + a, q[on, a])
                np.maximum.at(row, at + 4 + a, q[on, a] + BIAS)
                np.maximum.at(row, at + 7 + a, BIAS - q[on, a])
        hit = l_in & (lab == prd)
        np.add.at(row, lab[hit] * ENTRIES + 20, 1)
        row[words - 2] += int((l_in & p_in & (lab >= 1) & (prd >= 1)).sum())
    return rows


def scores_fp64(points, labels, preds, c):
    """The four scores of ONE scan straight from its vertices, in float64 and without quantisation: points (M, 3), labels and
    preds (M,) -> dict(tsa, tsa_instance, tla, tir, teeth, hits, degenerate [classes], dist {class: d_t}, size {class: 3-vector})."""
    x = np.asarray(points, np.float64)
    lab, prd = np.asarray(labels, np.int64), np.asarray(preds, np.int64)
    ok = (lab >= 0) & (lab < c)
    G = [k for k in range(1, c) if (lab == k).any()]
    P = [k for k in range(1, c) if (prd == k).any()]
    out = dict(teeth=0, hits=0, degenerate=[], dist={}, size={})
    if not G:
        out.update(tsa=np.nan, tsa_instance=np.nan, tla=np.nan, tir=np.nan)
        return out
    p_ok = (prd >= 0) & (prd < c)
    agree = ok & p_ok & ((lab != 0) == (prd != 0))
    out["tsa"] = agree.sum() / ok.sum()
    out["tsa_instance"] = float(np.mean([2.0 * ((lab == k) & (prd == k)).sum() / ((lab == k).sum() + (prd == k).sum()) for k in G]))
    cents = {k: x[prd == k].mean(0) for k in P}
    for t in G:
        mine = x[lab == t]
        size = mine.max(0) - mine.min(0)
        if (size == 0).any():
            out["degenerate"].append(t)
            continue
        out["teeth"] += 1
        out["size"][t] = size
        if not P:
            out["dist"][t] = 5.0
            continue
        g = mine.mean(0)
        best = min(P, key=lambda u: (np.linalg.norm(cents[u] - g), u))
        d = float(np.linalg.norm((g - cents[best]) / size))
        out["dist"][t] = d
        out["hits"] += int(d < 0.5 and best == t)
    n = out["teeth"]
    out["tla"] = float(np.mean(list(out["dist"].values()))) if n else np.nan
    out["tir"] = out["hits"] / n if n else np.nan
    return out


def tla_bound(points, center, labels, c):
    """How far a scan's quantised TLA may lie from the fp64 one, from the resolution and the data alone.
    A vertex's quantised offset q / 65536 differs from x - center by at most e = 2^-17 (the rounding of rint) plus the fp32
    rounding of the subtraction, half a unit in the last place of the largest |x - center| of the scan.  A centroid is a mean
    of such positions, so it moves by at most e per axis; an extent is a difference of two, so it moves by at most 2 e.  With
    delta = g - p (per axis at most D, the scan's diameter, moved by at most 2 e) and s the smallest extent of a true tooth
    that is not degenerate, |delta' / s' - delta / s| <= (2 e s + 2 e D) / (s (s - 2 e)) per axis, and the 2-norm over three
    axes at most sqrt(3) times that.  Valid while the nearest predicted tooth is the same one in both computations (the tests
    check the gap) and s > 2 e."""
    x = np.asarray(points, np.float64) - np.asarray(center, np.float64)[None]
    e = 2.0 ** -17 + np.spacing(F32(np.abs(x).max())) / 2
    e += 16 * np.spacing(np.abs(np.asarray(points, np.float64)).max())       # the float64 roundings of both computations' means
    diam = float((x.max(0) - x.min(0)).max())
    sizes = [np.ptp(x[labels == k], axis=0) for k in range(1, c) if (labels == k).any()]
    s = min(float(v.min()) for v in sizes if (v > 0).all())
    assert s > 2 * e
    return np.sqrt(3.0) * (2 * e * s + 2 * e * diam) / (s * (s - 2 * e))
