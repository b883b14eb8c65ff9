"""CPU checks of tests/_ntm_graph_ref.py, the fp64 helper tests/test_ntm_graph_gpu.py aims at the graph-loss kernels: it agrees
with oracle/np_ntm.py, its gradient is the derivative of its own loss, its builders keep their promises, and its tolerance
rule holds for an fp32 restatement of the same arithmetic that sums in a shuffled order (so the rule is about fp32, not about
one kernel).  The last test prints the largest error / bound per case family (pytest -s)."""
import numpy as np
import pytest

import _ntm_graph_ref as R
from oracle import np_ntm

C = 17


def _case(rng, b, n, k, c=C, d=3, labels="mixed", spread=1.0):
    t = b * n
    x = (rng.random((t, d), dtype=np.float32) * np.float32(spread / np.sqrt(d / 3.0))).astype(np.float32)
    lab = {"mixed": lambda: R.labels_mixed(rng, t), "equal": lambda: R.labels_equal(t),
           "different": lambda: R.labels_all_different(t)}[labels]()
    return x, lab, R.row_stochastic(rng, t, c), R.random_out_lists(rng, b, n, k)


def test_helper_agrees_with_the_oracle_restatement():
    rng = np.random.default_rng(0)
    b, n, k = 2, 40, 5
    x, lab, T, nbr = _case(rng, b, n, k)
    want_l, want_g, want_pp = np_ntm.threed_space_loss(x.reshape(b, n, 3), lab.reshape(b, n), T, nbr, 0.7)
    ref = R.graph_loss(x, lab, T, R.to_global(nbr), 0.7, signed=False, upstream=1.0, scale=1.0 / (b * n), chunk=16)
    assert np.abs(ref["per_point"] - want_pp).max() <= 1e-12 and abs(ref["per_point"].mean() - want_l) <= 1e-12
    assert np.abs(ref["grad"].reshape(want_g.shape) - want_g).max() <= 1e-12
    assert np.array_equal(ref["mag"], ref["per_point"])              # unsigned: no cancellation, mag is the value
    feats = rng.random((b, n, C), dtype=np.float32) / 4
    want_l, want_g, want_pp = np_ntm.feature_space_loss(feats.transpose(0, 2, 1), lab.reshape(b, n), T, nbr, 0.7)
    ref = R.graph_loss(feats.reshape(b * n, C), lab, T, R.to_global(nbr), 0.7, signed=True, upstream=1.0,
                       scale=1.0 / (b * n * k), chunk=16)
    assert np.abs(ref["per_point"] - want_pp).max() <= 1e-12 and abs(ref["per_point"].sum() / (b * n * k) - want_l) <= 1e-12
    assert np.abs(ref["grad"].reshape(want_g.shape) - want_g).max() <= 1e-12
    assert (ref["mag"] >= np.abs(ref["per_point"])).all() and (ref["terms"] >= k).all()


@pytest.mark.parametrize("signed", [False, True])
def test_helper_gradient_is_the_derivative_of_its_loss(signed):
    rng = np.random.default_rng(1)
    b, n, k, c = 2, 9, 3, 4
    x, lab, T, nbr = _case(rng, b, n, k, c=c)
    g = R.to_global(nbr)
    up, scale = -2.5, 1.0 / (b * n)
    ref = R.graph_loss(x, lab, T, g, 0.8, signed, up, scale)
    T64 = T.astype(np.float64)

    def loss(Tm):
        return up * scale * R.graph_loss(x, lab, Tm, g, 0.8, signed, want_grad=False)["per_point"].sum()
    h = 1e-6
    for _ in range(40):
        i, r, cc = int(rng.integers(b * n)), int(rng.integers(c)), int(rng.integers(c))
        p, m = T64.copy(), T64.copy()
        p[i, r, cc] += h
        m[i, r, cc] -= h
        fd = (loss(p) - loss(m)) / (2 * h)
        assert abs(fd - ref["grad"][i, r * c + cc]) <= 1e-8 * max(1.0, abs(fd))
    # terms and cond: a row's live out-edges plus live in-edges, and an upper bound of |grad|
    live = ref["w"] != 0
    assert np.array_equal(ref["terms"], live.sum(1) + R.in_degrees(g, live))
    assert (ref["cond"] >= np.abs(ref["grad"]) - 1e-15).all()


def test_builders_keep_their_promises():
    rng = np.random.default_rng(2)
    for b, n, k in ((3, 11, 3), (2, 130, 64), (1, 4097, 2), (1, 2, 1)):
        nbr = R.random_out_lists(rng, b, n, k)
        assert nbr.dtype == np.int32 and nbr.min() >= 0 and nbr.max() < n
        assert (nbr != np.arange(n)[None, :, None]).all()                              # self excluded
        assert (np.diff(np.sort(nbr, 2), axis=2) > 0).all()                            # distinct within a list
    n, k, tgt = 300, 8, 123
    for d in (0, 1, 63, 64, 65, 128, 129, n - 1):
        nbr = R.planted_in_degree(rng, n, k, tgt, d)
        assert R.in_degrees(R.to_global(nbr))[tgt] == d
        assert (nbr != np.arange(n)[None, :, None]).all() and (np.diff(np.sort(nbr, 2), axis=2) > 0).all()
    nbr = R.random_out_lists(rng, 1, 50, 4)
    R.ensure_edge(nbr, 0, 7, 9)
    R.ensure_edge(nbr, 0, 9, 7)                                                        # mutual
    R.ensure_edge(nbr, 0, 20, 21)
    R.remove_edge(nbr, rng, 0, 21, 20)                                                 # one-way
    for i in range(50):
        R.remove_edge(nbr, rng, 0, i, 30, avoid=(7, 9, 20, 21))                        # nobody lists 30
    assert 9 in nbr[0, 7] and 7 in nbr[0, 9] and 21 in nbr[0, 20] and 20 not in nbr[0, 21]
    assert R.in_degrees(R.to_global(nbr))[30] == 0 and (np.diff(np.sort(nbr, 2), axis=2) > 0).all()
    assert (nbr != np.arange(50)[None, :, None]).all()
    assert len(set(R.labels_all_different(40))) == 40 and len(set(R.labels_equal(40))) == 1
    assert set(R.labels_mixed(rng, 400)) == {0, 1, 2}


FAMILIES = (
    # name, b, n, k, c, labels, sigma, upstream
    [("k=%d" % k, 2, 130, k, C, "equal" if k == 64 else "mixed", 1.0, 1.0) for k in (1, 2, 3, 31, 32, 33, 63, 64)] +
    [("sigma=%g" % s, 2, 130, 7, C, "mixed", s, 1.0) for s in (0.35, 1.0, 2.0)] +
    [("upstream=%g" % u, 1, 300, 8, C, "equal", 1.0, u) for u in (-2.5, 0.0)] +
    [("labels %s" % l, 2, 130, 7, C, l, 1.0, 1.0) for l in ("equal", "different", "mixed")] +
    [("C=%d" % c, 1, 130, 5, c, "mixed", 1.0, 1.0) for c in (11, 12, 17, 18, 22, 23)] +
    [("walk t=%d" % t, 1, t, min(3, t - 1), C, "mixed", 1.0, 1.0) for t in (2, 17, 33, 129)] +
    [("scan t=4097", 1, 4097, 2, 2, "mixed", 1.0, 1.0)])


def test_tolerance_rule_holds_for_an_fp32_restatement(capsys):
    """Every family of the GPU table (and planted in-degrees up to t - 1), 3-D unsigned and feature-space signed: the fp32
    restatement with shuffled sums stays under the bound everywhere; nothing is masked."""
    rng = np.random.default_rng(3)
    worst = {}

    def run(name, x, lab, T, g, sigma, up, b_n_k):
        for signed in (False, True):
            xs = x if not signed else (rng.random((x.shape[0], T.shape[1]), dtype=np.float32) / np.float32(np.sqrt(T.shape[1])))
            scale = 1.0 / (b_n_k if signed else x.shape[0])
            ref = R.graph_loss(xs, lab, T, g, sigma, signed, up, scale)
            pp, grad = R.graph_loss_fp32(xs, lab, T, g, sigma, signed, up, scale, rng)
            fam = name.split("=")[0].split(" ")[0] + (" signed" if signed else "")
            rf = R.check_forward(pp, ref, name + " forward")
            rg = R.check_grad(grad, ref, name + " gradient")
            worst[fam] = max(worst.get(fam, 0.0), rf, rg)

    for name, b, n, k, c, labels, sigma, up in FAMILIES:
        x, lab, T, nbr = _case(rng, b, n, k, c=c, labels=labels)
        run(name, x, lab, T, R.to_global(nbr), sigma, up, b * n * k)
    for d in (0, 1, 63, 64, 65, 128, 129, 299):
        x, lab, T, _ = _case(rng, 1, 300, 8, labels="equal")
        run("in-degree=%d" % d, x, lab, T, R.to_global(R.planted_in_degree(rng, 300, 8, 17, d)), 1.0, 1.0, 300 * 8)
    with capsys.disabled():
        print("\nfp32 restatement, largest error / bound: " + ", ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert worst and max(worst.values()) < 1.0
