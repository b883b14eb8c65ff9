"""numpy float32 restatement of the cfg.filter_outlier anchors (geot_ntm_filtered_anchors, include/geot_hip.h "ABI 26") and the
inputs its CPU and GPU tests share.

threshold(): torch.quantile's linear interpolation as torch computes it for a float32 input -- the rank, the weight and the
lerp in float32, every operation rounded (the library is built with -ffp-contract=off) -- on np.sort's order.
anchors(): examples/segmentation/train.py:505-526 with cfg.filter_outlier written literally: class after class, the values at
or above the class's threshold set to 0 IN PLACE, then the first arg-max and that point's row of the edited array."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ntm_ref_transition.npz")
F32 = np.float32


def ranks(m, q):
    """(lo, hi, w) of torch.quantile over m values: rank = fl32(q) * fl32(m - 1), one float32 product."""
    rank = F32(q) * F32(m - 1)
    lo, hi = int(np.floor(rank)), int(np.ceil(rank))
    return lo, hi, F32(rank - F32(lo))


def threshold(flat, q):
    """-> (threshold float32, lo, hi, s[lo], s[hi])."""
    s = np.sort(np.asarray(flat, dtype=F32).reshape(-1))
    lo, hi, w = ranks(s.size, q)
    d = F32(s[hi] - s[lo])
    t = F32(s[lo] + F32(w * d)) if w < F32(0.5) else F32(s[hi] - F32(d * F32(F32(1) - w)))
    return t, lo, hi, s[lo], s[hi]


def anchors(eta, q=0.97):
    """eta (B, C, N) float32 -> (class_T (C,C), v_star (C,), thresh (C,), lo, hi), all float32."""
    work = np.array(eta, dtype=F32)       # a copy: the filter writes into it, as the reference's clone() (train.py:507)
    B, C, N = work.shape
    class_T, v_star, thresh = np.empty((C, C), F32), np.empty(C, F32), np.empty(C, F32)
    lo = hi = 0
    for cc in range(C):
        view = work[:, cc, :]
        thresh[cc], lo, hi = threshold(view, q)[:3]
        view[view >= thresh[cc]] = 0.0
        best = int(np.argmax(view.reshape(B * N)))         # first maximum
        class_T[cc] = work[best // N, :, best % N]
        v_star[cc] = view[best // N, best % N]
    return class_T, v_star, thresh, lo, hi


# ---- the inputs ------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 17), (1, 2, 17), (1, 3, 2), (1, 35, 17), (1, 101, 3), (2, 96, 17), (1, 1023, 5), (1, 1024, 17), (1, 1025, 17),
          (1, 2049, 1), (2, 4099, 32), (3, 5000, 17),
          # the select kernel keeps up to 48 x 1024 keys in registers and streams above that: the last size of the one form (every
          # register slot full) and the first of the other (four sweeps of 16 x 1024, the last one a single value)
          (3, 16384, 2), (1, 49153, 3)]
BOUNDARY_SHAPES = SHAPES[-2:]
Q_SHAPE = (1, 1025, 17)
PLANTED_CLASS, CONSTANT_VALUE = 2, 0.25


def _softmax(logits):
    e = np.exp(logits - logits.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(F32)


def constant_class(shape):
    return min(1, shape[2] - 1)


@functools.lru_cache(maxsize=None)
def make_eta(kind, shape, seed):
    """One input of the given kind, (B, C, N) float32 with shape = (B, N, C) as the ABI orders its sizes."""
    B, N, C = shape
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((B, C, N))
    if kind == "fixture":
        assert shape == (2, 96, 17)
        eta = np.load(GOLDEN)["c17_filt_eta"].astype(F32)
    elif kind == "random":
        eta = _softmax(8 * logits)
    elif kind == "saturated":         # many exact 1.0f, exact zeros and denormals
        eta = _softmax(60 * logits)
    elif kind == "ties":              # values rounded to eighths
        eta = (np.round(_softmax(8 * logits) * 8) / 8).astype(F32)
    elif kind == "constant":          # one class constant at every point: all of it is filtered
        eta = _softmax(8 * logits)
        eta[:, constant_class(shape), :] = CONSTANT_VALUE
    elif kind == "normal":            # keys of both signs
        eta = logits.astype(F32)
    elif kind == "negative":          # negative keys only: the substituted 0 is the maximum, the first filtered position wins
        eta = (-np.abs(logits) - 0.125).astype(F32)
    elif kind == "planted":
        # class PLANTED_CLASS: a tenth of the points hold exactly 0.9 (the 0.97-quantile falls among them: they are filtered),
        # (0, 0) holds 0.95 (filtered, must not win), (0, N-1) and (1, 3) hold 0.7, everything else is below 0.5
        assert B >= 2 and N >= 40
        eta = _softmax(8 * logits)
        vals = (0.5 * rng.random((B, N))).astype(F32)
        high = rng.permutation(np.arange(1, B * N))
        high = high[(high != N - 1) & (high != N + 3)][:(B * N) // 10]
        vals.reshape(-1)[high] = 0.9
        vals[0, 0], vals[0, N - 1], vals[1, 3] = 0.95, 0.7, 0.7
        eta[:, PLANTED_CLASS, :] = vals
    else:
        raise ValueError(kind)
    eta = np.ascontiguousarray(eta, dtype=F32)
    eta.setflags(write=False)
    return eta


def _cases():
    out = []
    for s, shape in enumerate(SHAPES):
        B, N, C = shape
        for k, kind in enumerate(("random", "saturated", "ties", "constant", "normal", "planted", "negative")):
            if kind == "saturated" and C < 2:       # a one-class soft-max is constant
                continue
            if kind == "constant" and shape not in ((1, 1, 17), (1, 35, 17), (2, 96, 17), (1, 1025, 17), (1, 2049, 1),
                                                    (2, 4099, 32)):
                continue
            if kind == "planted" and (B < 2 or C <= PLANTED_CLASS):
                continue
            if shape in BOUNDARY_SHAPES and kind not in ("random", "saturated", "ties", "negative"):
                continue
            out.append((kind, shape, 0.97, 100 * s + k))
    out.append(("fixture", (2, 96, 17), 0.97, 0))
    for i, q in enumerate((0.0, 0.5, 1.0)):         # (0.97 at this shape is in the crossing above)
        out.append(("random", Q_SHAPE, q, 2000 + i))
        out.append(("saturated", Q_SHAPE, q, 2100 + i))
    return out


CASES = _cases()       # (kind, (B, N, C), q, seed): the SAME list for the CPU and the GPU tests


def case_id(case):
    kind, (B, N, C), q, _ = case
    return "%s-%dx%dx%d-q%g" % (kind, B, N, C, q)


@functools.lru_cache(maxsize=None)
def expected(case):
    """The restatement's (class_T, v_star, thresh, lo, hi) of a case, computed once."""
    kind, shape, q, seed = case
    out = anchors(make_eta(kind, shape, seed), q)
    for a in out[:3]:
        a.setflags(write=False)
    return out
