"""part_seg_refinement (train.py:57-73) restated in numpy, rule by rule (include/geot_hip.h geot_scan_refine):

1. snap: the scan's labels before anything changes (what `pred.cpu().data.numpy()` is for the CUDA tensor the reference is
   written for).  alias=True is the other reading -- a CPU tensor, whose numpy view follows every write -- kept only to show
   that the two differ.
2. Counter(snap): the member count of every class present, in the order of first occurrence; one class: nothing happens.
3. every present class i, in that order, with count[i] < n or i not allowed: the queries are the vertices with snap == i;
   each counts the CURRENT labels of its n + 1 nearest vertices (earlier steps seen, this step's writes not), zeroes class i
   and takes the first maximum (all zero: 0).
4. neighbours by (d2, vertex index), d2 = ((dx dx) + (dy dy)) + (dz dz) in fp32; distances that are not finite never enter.
A label outside [0, c) is never a query, never votes and is never written.
"""
import numpy as np


def sqdist(q, pts):
    """fp32 ((dx dx) + (dy dy)) + (dz dz) of the queries q (Q, 3) against pts (M, 3) -> (Q, M)."""
    q, pts = np.asarray(q, np.float32), np.asarray(pts, np.float32)
    d = q[:, None, :] - pts[None, :, :]
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float32)


def nearest(pts, queries, k):
    """The k nearest vertices of every query vertex by (d2, index): (Q, k) int64, -1 where fewer than k distances are finite."""
    out = np.full((len(queries), k), -1, np.int64)
    for at in range(0, len(queries), 512):                          # (blocks of queries: the distance matrix stays small)
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = sqdist(pts[queries[at:at + 512]], pts)
        kth = np.partition(d2, k - 1, axis=1)[:, k - 1] if d2.shape[1] >= k else np.full(d2.shape[0], np.inf, np.float32)
        rows, cols = np.nonzero((d2 <= np.where(kth < np.inf, kth, np.inf)[:, None]) & (d2 < np.inf))     # what can be among the k
        by = np.lexsort((cols, d2[rows, cols], rows))                # per query by (d2, index)
        rows, cols = rows[by], cols[by]
        rank = np.arange(rows.size) - np.searchsorted(rows, np.arange(d2.shape[0]))[rows]
        out[at + rows[rank < k], rank[rank < k]] = cols[rank < k]
    return out


def refine_scan(pred, pts, c, n=10, allowed=None, alias=False):
    """One scan: pred (M,) integer labels, pts (M, 3) fp32, allowed: iterable of allowed labels or None (all)
    -> (refined (M,) int64, [steps, queries, changed, labels outside [0, c)])."""
    pred = np.array(pred, dtype=np.int64).reshape(-1)
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    snap = pred if alias else pred.copy()
    inside = (snap >= 0) & (snap < c)
    stats = [0, 0, 0, int((~inside).sum())]
    first = {}
    for v in np.flatnonzero(inside):
        first.setdefault(int(snap[v]), int(v))
    count = {i: int((snap == i).sum()) for i in first}
    if len(first) <= 1:
        return pred, stats
    ok = set(range(c)) if allowed is None else {int(a) for a in allowed}
    for i in sorted(first, key=first.get):                          # Counter iterates in the order of first occurrence
        if not (count[i] < n or i not in ok):
            continue
        queries = np.flatnonzero(snap == i)
        if queries.size == 0:                                        # (alias form only: an earlier step took them all)
            continue
        nbr = nearest(pts, queries, n + 1)
        labels = np.where(nbr >= 0, pred[np.maximum(nbr, 0)], -1)
        votes = np.zeros((queries.size, c), np.int64)
        for cls in range(c):
            votes[:, cls] = (labels == cls).sum(1)
        votes[:, i] = 0
        new = votes.argmax(1)                                        # the first maximum; all zero: 0
        stats[0] += 1
        stats[1] += int(queries.size)
        stats[2] += int((new != pred[queries]).sum())
        pred[queries] = new
    return pred, stats


def refine_scans(preds, clouds, c, n=10, allowed=None):
    """Several scans: lists of (M_i,) labels and (M_i, 3) vertices, allowed: None or one entry per scan
    -> (list of refined labels, (B, 4) int32 stats)."""
    out, stats = [], []
    for s, (p, x) in enumerate(zip(preds, clouds)):
        r, st = refine_scan(p, x, c, n, None if allowed is None else allowed[s])
        out.append(r)
        stats.append(st)
    return out, np.asarray(stats, np.int32).reshape(-1, 4)


def allowed_bits(labels):
    """geot_scan_refine's mask of one slot."""
    return int(sum(1 << int(a) for a in set(labels)))


def knn_gap(pts, queries, n):
    """Smallest fp64 gap between the (n + 1)-th and (n + 2)-th squared distance over the queries, in units of one fp32 ulp of
    the largest squared vertex norm (where torch.cdist + topk and the (d2, index) order cannot disagree about the set)."""
    x = np.asarray(pts, np.float64)
    d2 = ((x[queries][:, None, :] - x[None, :, :]) ** 2).sum(-1)
    d2.sort(axis=1)
    if d2.shape[1] < n + 2 or len(queries) == 0:
        return np.inf
    ulp = np.spacing(np.float32((x ** 2).sum(1).max())).astype(np.float64)
    return float((d2[:, n + 1] - d2[:, n]).min() / ulp)
