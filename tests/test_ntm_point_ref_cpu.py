"""CPU checks of tests/_ntm_point_ref.py, the fp64 helper tests/test_ntm_point_kernels_gpu.py aims at the 17-class per-point
NTM kernels: it agrees with oracle/np_ntm.py on the inputs of the original tests, its gradients are the derivatives of its own
outputs, its input builders reach what they promise (so no GPU test can pass by exercising nothing), and every bound the GPU
tests apply is met, with room, by an op-by-op fp32 restatement of the same statements (so the bounds are about fp32, not
about one kernel).  The last tests print their figures (pytest -s)."""
import numpy as np
import pytest

import _ntm_point_ref as R
from oracle import np_ntm

C = R.C
SHAPES = [(1, 1), (5, 7), (1, 32), (1, 33), (2, 1001), (3, 10931)]
LAMS = [0.9, 0.0, 1.0]
ZERO_SHAPE, ZERO_POINTS = (2, 1001), (0, 1001, 2001)       # a first point, a batch's first point, the last point (partial tile)

_sig = {}


def sig_case(b, n):
    if (b, n) not in _sig:
        p, cm, W, g = R.sig_inputs(b, n)
        _sig[(b, n)] = (p, cm, W, g, R.sig_t_mean(p, cm, W, g))
    return _sig[(b, n)]


def test_helper_agrees_with_the_oracle_on_the_original_inputs():
    import torch
    torch.manual_seed(0)
    W = torch.stack([torch.nn.Linear(2 * C, C, bias=False).weight for _ in range(C)]).detach().numpy()   # Ins_T_mean's init
    rng = np.random.default_rng(0)
    B, N = 2, 500
    p = R.softmax(rng.standard_normal((B, C, N)) * 2, 1).astype(np.float32)
    cm = R.softmax(rng.standard_normal((C, C)), 1).astype(np.float32)
    g = rng.standard_normal((B * N, C, C)).astype(np.float32)
    r = R.sig_t_mean(p, cm, W, g)
    assert np.abs(r["out"] - np_ntm.sig_t_mean(p, cm, W)).max() <= 1e-12
    want = np_ntm.sig_t_mean_grad_W(p, cm, W, g)
    assert np.abs(r["grad_W"] - want).max() <= 1e-12 * np.abs(want).max()
    assert not r["above"].any()                        # the gap: nn.Linear's init never reaches the upper clamp
    rng = np.random.default_rng(2)
    B, N = 1, 70
    logits = (rng.standard_normal((B, C, N)) * 2).astype(np.float32)
    insT = np_ntm.l1_normalize(rng.random((B * N, C, C)) + 0.01, 2).astype(np.float32)
    E = np_ntm.l1_normalize(rng.random((C, C)) + 0.01, 1).astype(np.float32)
    g = rng.standard_normal((B, C, N)).astype(np.float32)
    lam = float(np.float32(0.9))                       # the helper rounds lam as the C entry point does
    r = R.correct_logits(logits, insT, E, 0.9, g)
    assert np.abs(r["out"] - np_ntm.correct_logits(logits, insT, E, lam)[1]).max() <= 1e-12
    for got, want in zip((r["grad_logits"], r["grad_ins_T"], r["grad_ema_t"]), np_ntm.correct_logits_grads(logits, insT, E, lam, g)):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # and on operands of both signs with zero rows (np_ntm states the s <= 1e-12 form too)
    logits, insT, E, g = R.correct_inputs(1, 40, zero_points=(0, 39))
    r = R.correct_logits(logits, insT, E, 0.9, g)
    assert not r["live"][0, R.ZERO_ROW] and not r["live"][39, R.ZERO_ROW] and r["live"].sum() == 40 * C - 2
    for got, want in zip((r["grad_logits"], r["grad_ins_T"], r["grad_ema_t"]), np_ntm.correct_logits_grads(logits, insT, E, lam, g)):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_sig_gradients_are_the_derivatives_of_the_output():
    """Central differences in fp64, b*n = 4 points, every raw value at least 1e-4 from both clamp bounds."""
    rng = np.random.default_rng(3)
    p, cm, W, g = R.sig_inputs(2, 2, seed=5)
    r = R.sig_t_mean(p, cm, W, g)
    assert np.minimum(np.abs(r["raw"] - R.LO), np.abs(r["raw"] - R.HI)).min() > 1e-4
    assert r["inside"].any() and r["below"].any() and r["above"].any()
    W64, g64 = W.astype(np.float64), g.astype(np.float64)
    x = np.concatenate([p.transpose(0, 2, 1).reshape(4, C).astype(np.float64), np.ones((4, 1))], 1)

    def loss(Wm):
        return (R.sig_t_mean(p, cm, Wm)["out"] * g64).sum()
    h = 1e-6
    picks = [(R.ALL_LOW_HEAD, 0, 0)] + [tuple(int(v) for v in rng.integers(0, (C, C, 2 * C))) for _ in range(60)]
    for kk, o, j in picks:
        a, b_ = W64.copy(), W64.copy()
        a[kk, o, j] += h
        b_[kk, o, j] -= h
        fd = (loss(a) - loss(b_)) / (2 * h)
        assert abs(fd - r["grad_W"][kk, o, j]) <= 1e-7 * max(1.0, abs(fd))
    # d raw is the gradient with respect to raw: grad_W = d raw^T [p | 1], the constant column spread over cm
    G = np.einsum("iko,ij->koj", r["draw"], x)
    want = np.concatenate([G[:, :, :C], G[:, :, C:] * cm.astype(np.float64)[:, None, :]], 2)
    assert np.abs(want - r["grad_W"]).max() <= 1e-12
    assert (r["draw"][:, R.ALL_LOW_HEAD] == 0).all() and (r["grad_W"][R.ALL_LOW_HEAD] == 0).all()


@pytest.mark.parametrize("lam", LAMS)
def test_correct_gradients_are_the_derivatives_of_the_output(lam):
    rng = np.random.default_rng(4)
    logits, insT, E, g = R.correct_inputs(1, 3, seed=7)
    lam64 = float(np.float32(lam))
    assert np.abs(lam64 * E[None].astype(np.float64) + (1 - lam64) * insT).min() > 1e-4          # h = 1e-6 stays clear of the kinks of |v|
    r = R.correct_logits(logits, insT, E, lam, g)
    args = [a.astype(np.float64) for a in (logits, insT, E)]
    g64 = g.astype(np.float64)
    h = 1e-6
    for which, grad in ((0, r["grad_logits"]), (1, r["grad_ins_T"]), (2, r["grad_ema_t"])):
        for _ in range(25):
            idx = tuple(int(rng.integers(s)) for s in args[which].shape)
            a, b_ = [x.copy() for x in args], [x.copy() for x in args]
            a[which][idx] += h
            b_[which][idx] -= h
            fd = ((R.correct_logits(*a, lam)["out"] - R.correct_logits(*b_, lam)["out"]) * g64).sum() / (2 * h)
            assert abs(fd - grad[idx]) <= 1e-7 * max(1.0, abs(fd))


@pytest.mark.parametrize("b,n", SHAPES)
def test_sig_inputs_reach_every_clamp_region(b, n):
    p, cm, W, g, r = sig_case(b, n)
    below, inside, above, edge = R.region_shares(r)
    print("ntm-point-inputs | sig (%d, %d) | below %.4f inside %.4f above %.4f edge %.2e" % (b, n, below, inside, above, edge))
    assert min(below, inside, above) >= 0.01 and edge <= 1e-4
    assert abs(np.abs(W).max() * np.sqrt(2 * C) / 8 - 1) < 0.01 and np.allclose(p.sum(1), 1, atol=1e-6)
    # the all-low head: the whole row below the clamp at every point, 1/17 out, no gradient
    assert r["below"][:, R.ALL_LOW_HEAD].all() and not r["edge"][:, R.ALL_LOW_HEAD].any()
    assert np.abs(r["out"][:, R.ALL_LOW_HEAD] - 1.0 / C).max() <= 1e-15 and (r["draw"][:, R.ALL_LOW_HEAD] == 0).all()
    # every other head has live gradients, and rows are normalised
    live = r["inside"].any((0, 2))
    assert live[np.arange(C) != R.ALL_LOW_HEAD].all() or b * n < 8
    assert np.abs(r["out"].sum(2) - 1).max() <= 1e-12


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("b,n", SHAPES)
def test_correct_inputs_have_both_signs_and_conditioned_rows(b, n, lam):
    logits, insT, E, g = R.correct_inputs(b, n)
    r = R.correct_logits(logits, insT, E, lam)
    assert r["live"].all() and r["s"].min() > 1e-3
    assert 0.4 < (E < 0).mean() < 0.6
    if b * n >= 32:
        assert 0.45 < (insT < 0).mean() < 0.55
    else:
        assert (insT < 0).any() and (insT > 0).any()
    assert np.abs(insT).sum(2).std() > 0.1                  # not normalised


@pytest.mark.parametrize("lam", LAMS)
def test_degenerate_inputs_take_the_tiny_norm_branch(lam):
    b, n = ZERO_SHAPE
    t = b * n
    assert t % 32 != 0 and ZERO_POINTS[-1] >= t // 32 * 32 and ZERO_POINTS[0] < 32      # one in the partial last tile
    logits, insT, E, g = R.correct_inputs(b, n, zero_points=ZERO_POINTS)
    r = R.correct_logits(logits, insT, E, lam, g)
    dead = ~r["live"]
    assert (dead[:, np.arange(C) != R.ZERO_ROW] == 0).all()
    assert dead[list(ZERO_POINTS), R.ZERO_ROW].all() and (r["s"][dead] == 0).all()
    assert dead.sum() == (t if lam == 1.0 else 3)
    assert r["s"][r["live"]].min() > 1e-3
    # the forward gets exactly nothing from such a row; the backward is l g / 1e-12
    l = logits.transpose(0, 2, 1).reshape(t, C).astype(np.float64)
    go = g.transpose(0, 2, 1).reshape(t, C).astype(np.float64)
    lam64 = float(np.float32(lam))
    for i in ZERO_POINTS:
        want = (1 - lam64) * l[i, R.ZERO_ROW] * go[i] / 1e-12
        assert np.abs(r["grad_ins_T"][i, R.ZERO_ROW] - want).max() <= 1e-14 * np.abs(want).max()
        assert lam == 1.0 or np.abs(want).min() > 1e6
    zeroed = logits.copy()
    zeroed.transpose(0, 2, 1).reshape(t, C)[list(ZERO_POINTS), R.ZERO_ROW] = 0
    assert np.array_equal(R.correct_logits(zeroed, insT, E, lam)["out"], r["out"])


@pytest.mark.parametrize("b,n", SHAPES)
def test_an_fp32_restatement_meets_every_sig_bound(b, n):
    p, cm, W, g, r = sig_case(b, n)
    out, draw, gW = R.composite_sig_grad_W(p, cm, W, g)
    ratios = R.sig_forward_ratio(out, r), R.draw_ratio(draw, r), R.grad_W_ratio(gW, r, b * n)
    print("ntm-point-fp32 | sig (%d, %d) | forward %.4f d raw %.4f grad_W %.4f" % ((b, n) + ratios))
    assert max(ratios[:2]) <= 0.5                           # with room (the row sums come closest: 17 fp32 roundings)
    # The long sum: GRAD_W_TOL_LARGE is 4 x this composite's error where it was measured (0.25 printed above).  How a CPU GEMM
    # sums 32 793 terms is the BLAS build's business -- another machine's printed 3.5 here, 2.2e-6 of the scale, ten times the
    # MI355X kernel's own error -- so what is asserted of the composite is the project's bound, which any order meets.
    assert R.grad_W_ratio(gW, r, 0) <= 0.5
    base = np.random.default_rng(8).standard_normal(gW.shape).astype(np.float32)
    assert R.grad_W_ratio((base + gW).astype(np.float32), r, 0, base=base) <= 1.0


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("b,n,zero", [s + ((),) for s in SHAPES] + [ZERO_SHAPE + (ZERO_POINTS,)])
def test_an_fp32_restatement_meets_every_correct_bound(b, n, zero, lam):
    logits, insT, E, g = R.correct_inputs(b, n, zero_points=zero)
    r = R.correct_logits(logits, insT, E, lam, g)
    out, gl, gi, gE = R.composite_correct(logits, insT, E, lam, g)
    ratios = (R.correct_forward_ratio(out, r),) + R.correct_grads_ratio(gl, gi, gE, r, b * n)
    print("ntm-point-fp32 | correct (%d, %d) zero %s lam %.1f | out %.4f grad_logits %.4f grad_ins_T %.4f grad_ema_t %.4f"
          % ((b, n, bool(zero), lam) + ratios))
    assert max(ratios[:3]) <= 0.5
    assert R.correct_grads_ratio(gl, gi, gE, r, 0)[2] <= 0.5       # as for grad_W: the composite's own long sum, the project's bound
    assert (r["grad_ema_t_tile_abs"] <= r["grad_ema_t_abs"] * (1 + 1e-12)).all()       # |sum of a tile| <= sum of magnitudes
    if lam == 0.0:
        assert not gE.any()
    if lam == 1.0:
        assert not gi.any()
