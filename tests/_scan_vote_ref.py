"""geot_scan_vote restated in numpy fp64 (include/geot_hip.h): per vote the three nearest sampled points of every vertex,
get_pred_whole's inverse-distance weights -- computed in fp64 from the fp32 squared distances, which are what the kernel and
geot_three_nn_ws agree on bit for bit -- and the interpolation of the class probabilities; then the sum over the votes and
torch.argmax's rule (the first NaN if there is one, else the first maximum).

The tolerance of an accumulator element after V votes, absolute: (16 V + V^2) 2^-24.  The values lie in [0, V]; every
interpolated value carries about 16 fp32 roundings of quantities <= 1 (three reciprocals with their square roots and sums,
the norm's two sums, three divisions, three products, two sums), and the V - 1 additions round sums <= V."""
import numpy as np

EPS = 2.0 ** -24


def tolerance(votes):
    return (16 * votes + votes * votes) * EPS


def three_nn(unknown, known):
    """geot_three_nn's contract on the host: d2 = ((dx dx) + (dy dy)) + (dz dz) in fp32, the three smallest by (d2, index);
    with fewer than three sampled points the missing entries are (+inf, index 0), and a NaN vertex gets three of those
    -> (d2 (M, 3) float32, idx (M, 3) int64)."""
    unknown, known = np.asarray(unknown, np.float32), np.asarray(known, np.float32)
    d = unknown[:, None, :] - known[None, :, :]
    sq = d * d
    d2 = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
    m, n = d2.shape
    out_d, out_i = np.full((m, 3), np.inf, np.float32), np.zeros((m, 3), np.int64)
    for v in range(m):
        row = d2[v]
        keep = np.flatnonzero(~np.isnan(row))
        order = keep[np.lexsort((keep, row[keep]))][:3]
        out_d[v, :order.size], out_i[v, :order.size] = row[order], order
    return out_d, out_i


def interpolate(prob, d2, idx):
    """One vote: prob (C, n) fp32, d2 / idx (M, 3) -> (M, C) fp64."""
    prob = np.asarray(prob, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        r = 1.0 / (np.sqrt(np.asarray(d2, np.float32).astype(np.float64)) + 1e-8)
        w = r / ((r[:, 0] + r[:, 2]) + r[:, 1])[:, None]
        idx = np.asarray(idx).astype(np.int64)
        return prob[:, idx[:, 0]].T * w[:, 0:1] + prob[:, idx[:, 1]].T * w[:, 1:2] + prob[:, idx[:, 2]].T * w[:, 2:3]


def vote_sum(votes):
    """votes: per vote (prob (C, n), d2 (M, 3), idx (M, 3)) -> the (M, C) fp64 sum, added in call order."""
    total = None
    for prob, d2, idx in votes:
        one = interpolate(prob, d2, idx)
        total = one if total is None else total + one
    return total


def argmax(values):
    """torch.argmax(dim=1) of (M, C): the first NaN if the row has one, else the first maximum."""
    values = np.asarray(values)
    nan = np.isnan(values)
    return np.where(nan.any(1), nan.argmax(1), np.where(nan, -np.inf, values).argmax(1)).astype(np.int64)


def margin(values):
    """The gap between a row's two largest values (inf for one class, NaN for a row with a NaN)."""
    values = np.asarray(values, np.float64)
    if values.shape[1] == 1:
        return np.full(values.shape[0], np.inf)
    top = np.sort(values, axis=1)
    return top[:, -1] - top[:, -2]


def decided(values, votes):
    """The rows whose fp64 arg-max an fp32 accumulator within tolerance(votes) must reproduce: top-two margin >= twice the
    tolerance.  Rows with a NaN are decided by the first-NaN rule and count as decided."""
    with np.errstate(invalid="ignore"):
        return np.isnan(values).any(1) | (margin(values) >= 2 * tolerance(votes))
