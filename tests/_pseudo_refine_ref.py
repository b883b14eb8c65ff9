"""numpy float32 restatement of geot_pseudo_refine's contract (include/geot_hip.h): utils/pseudo_mask.py's three refinements
behind their neighbour search, every statement one fp32 operation in the header's order.  The maker of
tests/golden/pseudo_label_refine_ref.npz asserts it equals the reference's output exactly; the GPU tests compare the kernel
against it, bit for bit."""
import numpy as np

MODES = ("max", "margin", "margin_v1")


def neighbours_fp64(pos, n):
    """The n nearest OTHER points of every point by (fp64 squared distance, index) -> (B, N, n) int32, and per point the fp64
    gap between the (n + 1)-th and (n + 2)-th squared distance (the point itself is the first) in fp32 ulp of the largest
    squared norm: where it is wide, any fp32 search picks the same set."""
    ids, gaps = [], []
    for x in np.asarray(pos, np.float64):
        d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
        order = np.argsort(d2, axis=1, kind="stable")
        assert np.array_equal(order[:, 0], np.arange(len(x))), "a point is not its own nearest: duplicates"
        ids.append(order[:, 1:n + 1])
        srt = np.take_along_axis(d2, order, 1)
        ulp = np.float64(np.spacing(np.float32((x ** 2).sum(1).max())))
        gaps.append((srt[:, n + 1] - srt[:, n]) / ulp)
    return np.stack(ids).astype(np.int32), np.stack(gaps)


def refine(prob, nbr, k, mode, th, beta, e_joint=None):
    """prob (B, C, N) fp32, nbr (B, N, n) local ids, beta an fp32 scalar, e_joint >= C entries (margin_v1)
    -> (keep (B, N) uint8, value (B, N) fp32).  A point with an id outside [0, N): keep 0, value NaN."""
    assert mode in MODES
    prob = np.ascontiguousarray(prob, np.float32)
    nbr = np.asarray(nbr)
    bsz, c, npts = prob.shape
    n = nbr.shape[2]
    assert nbr.shape == (bsz, npts, n) and 1 <= k <= n
    beta = np.float32(beta)
    bad = ((nbr < 0) | (nbr >= npts)).any(-1)
    ids = np.where((nbr < 0) | (nbr >= npts), np.arange(npts)[None, :, None], nbr)
    vals = prob[np.arange(bsz)[:, None, None, None], np.arange(c)[None, :, None, None], ids[:, None, :, :]]      # (B, C, N, n)
    vals = np.sort(vals, axis=-1)[..., ::-1]                 # descending; np.sort puts NaN last, so it comes first here
    p = prob.copy()
    with np.errstate(all="ignore"):
        for s in range(k):
            v = vals[..., s]
            if mode == "margin_v1":
                e = np.asarray(e_joint, np.float64)[:c].astype(np.float32)[None, :, None]
                ub = (e * p) / v
                p = (p + v) - (p * ub)
            else:
                p = (p + beta * v) - ((p * v) * beta)
        assert p.dtype == np.float32
        top = np.sort(p, axis=1)[:, ::-1]
        value = top[:, 0] if mode == "max" else top[:, 0] - top[:, 1]
        value = np.where(bad, np.float32(np.nan), value).astype(np.float32)
        keep = (value >= np.float32(th)).astype(np.uint8)
    return keep, value
