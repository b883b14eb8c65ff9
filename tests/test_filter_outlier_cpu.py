"""cfg.filter_outlier's anchors (geot_ntm_filtered_anchors, include/geot_hip.h "ABI 26") without a GPU: the numpy float32
restatement the GPU tests referee with (tests/_outlier_ref.py) against the reference's loop run literally on CPU torch, against
the vectorised composite ntm._filtered_anchor_rows, against the float64 oracle and against the reference-executed fixture --
on every input the GPU tests use, drawn by the one shared helper; that each threshold lies between its two order statistics;
the branches the shapes were chosen for; the ABI."""
import os
import re

import numpy as np
import pytest
import torch

import _outlier_ref as ref
from geot_amd import _lib, ntm
from oracle import np_ntm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# If an input ever makes CPU torch's mask (or the float64 oracle's) differ from the restatement's, its SEED changes in
# tests/_outlier_ref.py, not the rule: that can only happen when an interpolated threshold rounds onto s[lo] in one
# arithmetic and not in the other (torch's own lerp is contracted on some CPUs: one ulp in the last step).


def _reference_loop(eta, q):
    """train.py:505-526 with cfg.filter_outlier, literally (the in-place edit of eta_corr included), on CPU torch."""
    eta_corr = torch.from_numpy(np.array(eta))
    B, C, N = eta_corr.shape
    class_T = torch.empty(C, C)
    for cc in range(C):
        thresh = eta_corr[:, cc, :].quantile(q=q)
        robust = eta_corr[:, cc, :]
        robust[robust >= thresh] = 0.0
        best = torch.argmax(robust.contiguous().view(-1))
        class_T[cc] = eta_corr[best // N, :, best % N]
    return class_T.numpy()


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_restatement_equals_the_reference_loop_the_composite_and_the_oracle(case):
    kind, shape, q, seed = case
    eta = ref.make_eta(kind, shape, seed)
    class_T, v_star, thresh, lo, hi = ref.expected(case)
    assert np.array_equal(class_T, _reference_loop(eta, q)), "the literal loop on CPU torch"
    got_T, got_v = ntm._filtered_anchor_rows(torch.from_numpy(np.array(eta)), q)
    assert np.array_equal(class_T, got_T.numpy()) and np.array_equal(v_star, got_v.numpy()), "ntm._filtered_anchor_rows"
    B, N, C = shape
    if C <= len(np_ntm.LABEL_PROJ):
        with np.errstate(invalid="ignore", divide="ignore"):      # (the rows after class_T: an all-zero row sum at tiny shapes)
            want = np_ntm.class_transition(eta, np.full(C, 0.4), np.eye(C), filter_outlier=True, outlier_q=q)["class_T"]
        assert np.array_equal(class_T.astype(np.float64), want), "oracle.np_ntm.class_transition"


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_threshold_lies_between_its_order_statistics(case):
    kind, shape, q, seed = case
    eta = ref.make_eta(kind, shape, seed)
    for cc in range(shape[2]):
        t, lo, hi, s_lo, s_hi = ref.threshold(eta[:, cc, :], q)
        assert 0 <= lo <= hi <= min(lo + 1, eta.shape[0] * eta.shape[2] - 1)
        assert s_lo <= t <= s_hi, (cc, float(s_lo), float(t), float(s_hi))


def test_fixture_class_T_exactly():
    z = np.load(ref.GOLDEN)
    class_T = ref.expected(("fixture", (2, 96, 17), 0.97, 0))[0]
    assert np.array_equal(class_T, z["c17_filt_class_T_f32"])


def test_shapes_reach_the_branches_they_were_chosen_for():
    assert ref.ranks(1, 0.97) == (0, 0, 0.0)                         # (1, 1, 17): lo == hi == 0
    lo, hi, w = ref.ranks(35, 0.97)                                  # the second interpolation form
    assert (lo, hi) == (32, 33) and abs(float(w) - 0.98) < 1e-5 and w >= 0.5
    assert ref.ranks(101, 0.97) == (97, 97, 0.0)                     # w = 0 exactly: fl32(0.97) * 100 rounds to 97
    lo, hi, w = ref.ranks(2049, 0.97)
    assert hi == lo + 1 and abs(float(w) - 0.56) < 1e-3
    assert ref.ranks(1025, 0.0) == (0, 0, 0.0) and ref.ranks(1025, 1.0) == (1024, 1024, 0.0) and ref.ranks(1025, 0.5)[2] == 0.0
    assert ref.ranks(1 << 24, 1.0) == ((1 << 24) - 1, (1 << 24) - 1, 0.0)
    # everything filtered: index 0 wins and v_star = 0
    class_T, v_star, thresh, _, _ = ref.expected(("random", (1, 1, 17), 0.97, 0))
    row = ref.make_eta("random", (1, 1, 17), 0)[0, :, 0]       # row cc: columns 0..cc filtered, the later ones not yet
    assert not v_star.any() and np.array_equal(class_T, np.triu(np.tile(row, (17, 1)), 1))
    for case in ref.CASES:
        kind, shape, q, seed = case
        eta = ref.make_eta(kind, shape, seed)
        class_T, v_star, thresh, _, _ = ref.expected(case)
        if kind == "constant":
            k = ref.constant_class(shape)
            assert thresh[k] == np.float32(ref.CONSTANT_VALUE) and v_star[k] == 0
        if kind == "planted":       # the first of the two equal surviving maxima: (0, N - 1), not (1, 3), not the larger (0, 0)
            k, n = ref.PLANTED_CLASS, shape[1]
            assert thresh[k] == np.float32(0.9) and v_star[k] == np.float32(0.7)
            assert class_T[k, k + 1] == eta[0, k + 1, n - 1] != eta[1, k + 1, 3]
        if kind == "normal" and shape[0] * shape[1] > 1:
            assert (eta < 0).any() and (eta > 0).any()
        if kind == "negative":      # the substituted 0 is the maximum: the first filtered position wins
            assert (eta < 0).all() and (thresh < 0).all() and not v_star.any()
            first = np.argmax(eta[:, 0, :].reshape(-1) >= thresh[0])
            assert np.array_equal(class_T[0, 1:], eta[first // shape[1], 1:, first % shape[1]])
        if kind == "saturated" and shape[0] * shape[1] >= 1023:
            assert (eta == 1).sum() > 100 and (eta == 0).any()
        if kind == "ties":
            assert np.array_equal(eta * 8, np.round(eta * 8))


def test_header_declares_the_entry_point_and_abi_agrees():
    hdr = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    assert int(re.search(r"GEOT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 26
    lib = _lib.load()
    assert lib.geot_abi_version() == _lib.ABI_VERSION
    assert "geot_ntm_filtered_anchors" in _lib.PROTOTYPES and hasattr(lib, "geot_ntm_filtered_anchors")
    kinds = [a.__name__ for a in _lib.PROTOTYPES["geot_ntm_filtered_anchors"]]
    assert kinds == ["c_int"] * 3 + ["c_double"] + ["c_void_p"] * 5
    assert ntm.FILTER_MAX_POINTS == 1 << 24
