"""The Teeth3DS challenge scores without a GPU: the header's version and prototype, every refusal of geot_tooth_moments
through the host-only path (a refusal comes before any launch), tooth_scores_from_moments on hand-built rows -- a perfect
prediction, two neighbouring teeth swapped, no predicted tooth, a one-vertex tooth, a tie between two predicted centroids --
the quantised scores against an independent unquantised fp64 computation within a bound derived from the resolution and the
data, and fit()'s val_teeth3ds switch."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tooth_scores_ref as tref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from geot_amd import _lib, build
    build.build()
    return _lib.load()


def test_abi_version_and_signature(lib):
    from geot_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    assert int(re.search(r"GEOT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 32
    assert lib.geot_abi_version() == _lib.ABI_VERSION
    proto = re.search(r"int geot_tooth_moments\((.*?)\);", hdr, flags=re.S).group(1)
    assert len(proto.split(",")) == len(_lib.PROTOTYPES["geot_tooth_moments"]) == 15
    assert lib.geot_tooth_moments.restype is ctypes.c_int
    assert "tooth_scores.hip" in open(os.path.join(ROOT, "geot_amd", "build.py")).read()


def _args(**over):
    one = 4096                          # any non-NULL, 16-byte aligned address: a refusal never reads it
    args = dict(b=1, c=17, n_scans=1, total=8, points=one, labels=one, offsets=one, scan_ids=one, center=one, n_work=1, work=one,
                out_offsets=one, pred=one, moments=one, stream=None)
    args.update(over)
    return list(args.values())


REFUSALS = [dict(b=-1), dict(b=65536), dict(c=0), dict(c=33), dict(n_scans=0), dict(total=0), dict(n_work=-1), dict(work=None),
            dict(work=4100)] + [{k: None} for k in ("points", "labels", "offsets", "scan_ids", "center", "out_offsets", "pred", "moments")]


@pytest.mark.parametrize("over", REFUSALS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_refusals_come_before_any_launch(lib, over):
    assert lib.geot_tooth_moments(*_args(**over)) == 1            # hipErrorInvalidValue


def test_nothing_to_do_is_success(lib):
    for over in (dict(b=0), dict(n_work=0, work=None)):
        assert lib.geot_tooth_moments(*_args(**over)) == 0, over


# ---------------------------------------------------------------------------------------------------- hand-built rows
C = 5
rng = np.random.default_rng(11)


def _teeth(n=12):
    """Four teeth in a row along x, 3 apart and about 2 wide, plus gingiva: (points (M, 3) fp32, labels (M,) int64)."""
    pts, lab = [rng.uniform(-1, 1, size=(40, 3)) * [8, 1, 1] + [4, -4, 0]], [np.zeros(40, np.int64)]
    for k in range(1, C):
        pts.append(rng.uniform(-1, 1, size=(n, 3)) + [3.0 * k, 0, 0])
        lab.append(np.full(n, k, np.int64))
    return np.concatenate(pts).astype(np.float32), np.concatenate(lab)


def _rows(points, labels, preds, center):
    m = len(points)
    return tref.moments_ref(1, C, points, labels.astype(np.int32), np.array([0, m]), np.array([0]), center[None],
                            np.array([[0, 0, m, 0]]), np.array([0]), preds)


def _scores(points, labels, preds, center=None):
    from geot_amd.validation import tooth_scores_from_moments
    center = points.mean(0).astype(np.float32) if center is None else center
    return tooth_scores_from_moments(_rows(points, labels, preds, center), center[None], C, [True])


def test_a_perfect_prediction():
    points, labels = _teeth()
    out = _scores(points, labels, labels.copy())
    assert out["tla"] == 0 and out["tir"] == 1 and out["tsa"] == 1 and out["tsa_instance"] == 1
    assert out["exp_neg_tla"] == 1 and out["score"] == 1 and out["degenerate"] == [] and out["unusable"] == 0
    assert out["teeth_list"] == [4] and out["hits_list"] == [4] and out["mandible_tir"] == 1 and np.isnan(out["maxillary_tir"])


def test_two_neighbouring_teeth_swapped_cost_exactly_two_teeth_of_tir():
    points, labels = _teeth()
    preds = labels.copy()
    preds[labels == 2], preds[labels == 3] = 3, 2
    out = _scores(points, labels, preds)
    assert out["tir"] == 1 - 2 / 4 and out["tsa"] == 1              # every tooth vertex is still a tooth vertex
    assert out["tsa_instance"] == 0.5 and out["tla"] == 0           # each true tooth has a predicted centroid on top of it
    assert out["hits_list"] == [2]


def test_no_predicted_tooth_is_the_penalty():
    points, labels = _teeth()
    out = _scores(points, labels, np.zeros_like(labels))
    assert out["tla"] == 5 and out["tir"] == 0 and out["exp_neg_tla"] == np.exp(-5.0)
    assert out["tsa"] == (labels == 0).mean() and out["tsa_instance"] == 0


def test_a_one_vertex_tooth_is_degenerate_and_leaves_the_denominators():
    points, labels = _teeth()
    keep = np.ones(len(labels), bool)
    keep[np.flatnonzero(labels == 4)[1:]] = False                   # tooth 4 keeps one vertex: no extent
    points, labels = points[keep], labels[keep]
    preds = labels.copy()
    preds[labels == 1] = 0                                          # tooth 1 is missed: its nearest centroid is tooth 2's
    out = _scores(points, labels, preds)
    assert out["degenerate"] == [(0, 4)] and out["teeth_list"] == [3] and out["hits_list"] == [2]
    assert out["tir"] == 2 / 3 and len(out["tla_list"]) == 1 and out["tla"] > 0
    want = tref.scores_fp64(points, labels, preds, C)
    assert want["degenerate"] == [4] and want["teeth"] == 3 and want["hits"] == 2


def test_a_tie_between_two_predicted_centroids_goes_to_the_lower_class():
    # true tooth 2 at the origin; predicted teeth 3 and 1 with centroids at exactly -+ 0.25 on x (integers after scaling)
    points = np.array([[-1, -1, -1], [1, 1, 1], [0.25, 0, 0], [-0.25, 0, 0], [5, 5, 5]], np.float32)
    labels = np.array([2, 2, 0, 0, 0], np.int64)
    center = np.zeros(3, np.float32)
    for first, second, want_hit in ((3, 1, 0), (1, 3, 0)):
        preds = np.array([0, 0, first, second, 0], np.int64)
        out = _scores(points, labels, preds, center)
        assert out["tla_list"] == [np.sqrt((0.25 / 2) ** 2)] and out["hits_list"] == [want_hit]
    # the same tie with the true class among the two: class 2 (lower than 3) wins and is a hit; against class 1 it loses
    assert _scores(points, labels, np.array([0, 0, 3, 2, 0], np.int64), center)["hits_list"] == [1]
    assert _scores(points, labels, np.array([0, 0, 1, 2, 0], np.int64), center)["hits_list"] == [0]


def test_quantised_scores_agree_with_unquantised_fp64_within_the_derived_bound():
    """Scan coordinates in millimetres away from the origin, a noisy prediction; the bound comes from the resolution, the fp32
    rounding of x - center and the smallest extent of this data (tests/_tooth_scores_ref.py tla_bound)."""
    from geot_amd.validation import tooth_scores_from_moments
    r = np.random.default_rng(12)
    rows, centers, wants, bounds = [], [], [], []
    for shift in ([14.0, -37.0, 61.0], [-80.0, 20.0, 5.0]):
        points, labels = _teeth(40)
        points = (points + np.array(shift, np.float32)).astype(np.float32)
        preds = labels.copy()
        flip = r.random(len(labels)) < 0.2
        preds[flip] = r.integers(0, C, size=int(flip.sum()))
        center = points.mean(0).astype(np.float32)
        rows.append(_rows(points, labels, preds, center)[0])
        centers.append(center)
        wants.append(tref.scores_fp64(points, labels, preds, C))
        bounds.append(tref.tla_bound(points, center, labels, C))
    got = tooth_scores_from_moments(np.stack(rows), np.stack(centers), C, [True, False])
    for i, (want, bound) in enumerate(zip(wants, bounds)):
        print("scan %d: tla %.9f (fp64 %.9f), bound %.3e" % (i, got["tla_list"][i], want["tla"], bound))
        assert 0 < bound < 1e-3                                             # far below the 0.5 the identification turns on
        assert abs(got["tla_list"][i] - want["tla"]) <= bound
        assert min(abs(d - 0.5) for d in want["dist"].values()) > bound    # no tooth sits on the threshold: TIR is exact
        assert got["tir_list"][i] == want["tir"] and got["hits_list"][i] == want["hits"]
        assert got["tsa_list"][i] == want["tsa"] and got["tsa_instance_list"][i] == want["tsa_instance"]      # counts: exact
    assert got["tir"] == sum(w["hits"] for w in wants) / sum(w["teeth"] for w in wants)
    assert abs(got["tla"] - np.mean([w["tla"] for w in wants])) <= max(bounds)
    assert got["score"] == (got["tsa"] + np.exp(-got["tla"]) + got["tir"]) / 3
    assert got["mandible_tla"] == got["tla_list"][0] and got["maxillary_tla"] == got["tla_list"][1]


def test_unusable_positions_are_counted_and_warned_about(caplog):
    from geot_amd.validation import tooth_scores_from_moments
    points, labels = _teeth()
    points[3, 1] = np.nan
    center = np.zeros(3, np.float32)
    with caplog.at_level("WARNING"):
        out = tooth_scores_from_moments(_rows(points, labels, labels.copy(), center), center[None], C, [False])
    assert out["unusable"] == 1 and "1 vertex positions" in caplog.text and out["tir"] == 1


def test_fit_refuses_a_val_teeth3ds_that_is_no_bool_before_anything_runs():
    from geot_amd.fit import _val_teeth3ds, fit
    assert _val_teeth3ds({}) is False and _val_teeth3ds({"val_teeth3ds": True}) is True
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="val_teeth3ds"):
            fit(None, None, {"val_teeth3ds": bad, "epochs": 1})


def test_the_names_are_exported():
    import geot_amd
    from geot_amd import validation
    for name in ("ToothScores", "tooth_scores_from_moments", "tooth_instances"):
        assert getattr(geot_amd, name) is getattr(validation, name)
