"""CPU suite: the host half of the FixMatch batcher (geot_amd/openpoints/dataset/fixmatch_batch.py) against the
reference-executed fixture tests/golden/fixmatch_views_ref.npz (tests/golden/make_views_golden.py) -- the random draws, the
generators' state after them, the tests' own restatement (tests/_views_ref.py) and the argument checks.  No GPU."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _views_ref as vr  # noqa: E402

CASES = ("cfg", "rot")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("fixmatch_views_ref.npz")


def _sizes(fx, split):
    return [fx["scan_%s%d" % (split, i)].shape[0] for i in range(3)]


def _replay(fx, case):
    """The per-item sequence of the reference under the fixture's seed -> (labelled params, (weak, strong) pairs)."""
    from geot_amd.openpoints.dataset import draw_view_params
    kwargs = json.loads(str(fx[case + "_kwargs"]))
    m = int(fx["num_points"])
    seed = int(fx[case + "_seed"])
    np.random.seed(seed)
    torch.manual_seed(seed)
    lab, unl = [], []
    for i, n in enumerate(_sizes(fx, "l")):
        sel = np.random.choice(n, m, replace=n < m)
        assert np.array_equal(sel, fx[case + "_l_sel"][i])
        lab.append(draw_view_params("train", kwargs))
    for i, n in enumerate(_sizes(fx, "u")):
        sel = np.random.choice(n, m, replace=n < m)
        assert np.array_equal(sel, fx[case + "_u_sel"][i])
        unl.append((draw_view_params("train_w", kwargs), draw_view_params("train_s", kwargs)))
    return lab, unl


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("case", CASES)
def test_draws_match_the_reference_bit_for_bit(fx, case):
    lab, unl = _replay(fx, case)
    for i, p in enumerate(lab):
        assert p["kind"] == "train" and not p["rotate"] and not p["translate"]
        assert _same_bits(p["s"], fx[case + "_l_s"][i])
        assert _same_bits(p["R"], np.eye(3)) and _same_bits(p["t"], np.zeros(3))
    for i, (w, s) in enumerate(unl):
        assert _same_bits(w["s"], np.ones(3)) and _same_bits(w["R"], np.eye(3)) and _same_bits(w["t"], np.zeros(3))
        assert not w["rotate"] and not w["translate"]
        assert s["rotate"] and s["translate"]
        assert _same_bits(s["s"], fx[case + "_u_s_s"][i])
        assert _same_bits(s["R"], fx[case + "_u_R_s"][i])
        assert _same_bits(s["t"], fx[case + "_u_t_s"][i])
    # quirk 1: the configured rotation is exactly the identity (the yaml's `angle` is read by nothing); angle_s rotates
    identity = all(_same_bits(fx[case + "_u_R_s"][i], np.eye(3)) for i in range(3))
    assert identity == (case == "cfg")
    assert (np.abs(fx[case + "_u_theta"]).max() == 0) == (case == "cfg")


@pytest.mark.parametrize("case", CASES)
def test_generators_end_where_the_reference_left_them(fx, case):
    _replay(fx, case)
    assert np.array_equal(np.random.random_sample(4), fx[case + "_next_np"])
    assert np.array_equal(torch.rand(4).numpy(), fx[case + "_next_torch"])


@pytest.mark.parametrize("case", CASES)
def test_batcher_draw_order_is_the_per_item_order(fx, case):
    """FixMatchBatcher.draw (host only) consumes both streams as the two datasets do."""
    from geot_amd.openpoints.dataset import FixMatchBatcher
    b = FixMatchBatcher.__new__(FixMatchBatcher)          # the draw needs the sizes alone: no device
    b.n_l, b.n_u, b.m, b.kwargs = 3, 3, int(fx["num_points"]), json.loads(str(fx[case + "_kwargs"]))
    b.scans = type("Sizes", (), {"sizes": _sizes(fx, "l") + _sizes(fx, "u")})()
    seed = int(fx[case + "_seed"])
    np.random.seed(seed)
    torch.manual_seed(seed)
    sel, params = b.draw([0, 1, 2], [0, 1, 2])
    assert np.array_equal(sel[:3], fx[case + "_l_sel"]) and np.array_equal(sel[3:], fx[case + "_u_sel"])
    for i in range(3):
        assert _same_bits(params[i]["s"], fx[case + "_l_s"][i])
        assert _same_bits(params[3 + i][1]["R"], fx[case + "_u_R_s"][i]) and _same_bits(params[3 + i][1]["t"], fx[case + "_u_t_s"][i])
    assert np.array_equal(np.random.random_sample(4), fx[case + "_next_np"])
    assert np.array_equal(torch.rand(4).numpy(), fx[case + "_next_torch"])


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_fixture_within_e_ref(fx, case):
    g = json.loads(str(fx[case + "_kwargs"]))["gravity_dim"]
    eye, zero, one = np.eye(3, dtype=np.float32), np.zeros(3, np.float32), np.ones(3, np.float32)
    jobs = [("l_", "", fx[case + "_l_raw_pos"][i], i, fx[case + "_l_s"][i], eye, zero, False) for i in range(3)]
    jobs += [("u_", "_w", fx[case + "_u_raw_pos"][i], i, one, eye, zero, False) for i in range(3)]
    jobs += [("u_", "_s", fx[case + "_u_raw_pos"][i], i, fx[case + "_u_s_s"][i], fx[case + "_u_R_s"][i], fx[case + "_u_t_s"][i], True)
             for i in range(3)]
    for side, suffix, raw, i, s, R, t, strong in jobs:
        ref = vr.view_f64(raw, s, R, t, g, rotate=strong, translate=strong)
        key = case + "_" + side
        assert np.array_equal(fx[key + "x" + suffix][i], ref["x"].T)                      # one rounding of identical inputs
        assert np.array_equal(fx[key + "heights" + suffix][i], ref["heights"])
        e_ref = float(fx[case + "_eref_" + side + "pos" + suffix])
        assert 0 < e_ref < 1e-6
        err = np.abs(fx[key + "pos" + suffix][i].astype(np.float64) - ref["pos"]).max()
        print("%s %spos%s[%d]: |fixture - fp64| = %.3e (e_ref %.3e)" % (case, side, suffix, i, err, e_ref))
        assert err <= e_ref
        assert float(fx[case + "_eref_" + side + "x" + suffix]) == 0 and float(fx[case + "_eref_" + side + "heights" + suffix]) == 0
        # the fp32 statements, given the fp64 statistics rounded once, stay inside the same bound plus their own rounding
        p32 = vr.pos_f32_given_stats(raw, s, R, t, ref["center"], ref["scale"], rotate=strong, translate=strong)
        assert np.abs(p32.astype(np.float64) - ref["pos"]).max() <= 8 * vr.EPS32
    # quirk 3: the un-suffixed keys of the unlabelled batch are the untransformed sample
    for k in ("pos", "x"):
        assert np.array_equal(fx[case + "_u_" + k], fx[case + "_u_raw_pos"])
    for k in ("y", "cls", "class_weights"):
        assert np.array_equal(fx[case + "_u_" + k], fx[case + "_u_" + k + "_w"])
        assert np.array_equal(fx[case + "_u_" + k], fx[case + "_u_" + k + "_s"])


@pytest.mark.parametrize("m", (1, 5, 513, 768, 24577, 30000))
def test_the_restated_reduction_tree_is_the_fp64_mean_up_to_its_last_bits(m):
    """Two orders of summing m fp64 numbers differ by at most 2 (m - 1) 2^-53 sum|q|: for the mean, 2 m 2^-53 mean|q|."""
    rng = np.random.default_rng(m)
    q = (rng.standard_normal((m, 3)) * np.array([.3, .2, .08]) + np.array([.1, -.2, .05])).astype(np.float32)
    tree, mean = vr.mean_tree_f64(q), q.astype(np.float64).mean(axis=0)
    bound = 2 * m * 2.0 ** -53 * np.abs(q.astype(np.float64)).mean(axis=0)
    print("m=%d: |tree - np.mean| = %s (bound %s)" % (m, np.abs(tree - mean), bound))
    assert tree.dtype == np.float64 and (np.abs(tree - mean) <= bound).all()
    if m == 1:
        assert np.array_equal(tree, q[0].astype(np.float64))
    q[m // 2, 1] = np.nan                                     # a NaN vertex reaches its column alone
    assert np.array_equal(np.isnan(vr.mean_tree_f64(q)), [False, True, False])


def test_fixture_is_data_with_provenance(fx):
    meta = json.loads(str(fx["meta"]))
    assert meta["generator"] == "tests/golden/make_views_golden.py" and meta["provenance"]
    assert meta["lists"]["train_s"][1:] == ["PointCloudScaling_s", "PointCloudCenterAndNormalize", "PointCloudRotation_s",
                                            "PointCloudTranslation_s"]
    assert min(_sizes(fx, "u")) < int(fx["num_points"])           # one scan is sampled with replacement
    assert all(a.dtype.kind in "fiuU" for a in (fx[k] for k in fx.files))
    from geot_amd.openpoints.dataset import TOOTH_VIEW_KWARGS
    cfg = json.loads(str(fx["cfg_kwargs"]))
    assert all(cfg[k] == v for k, v in TOOTH_VIEW_KWARGS.items()) and "angle_s" not in cfg


def test_argument_errors_raise_before_any_device_call():
    from geot_amd.openpoints.dataset import DeviceScanSet, FixMatchBatcher, cloud_sample_batch, draw_view_params, fixmatch_views
    from geot_amd.openpoints.dataset.fixmatch_batch import pack_view_jobs
    with pytest.raises(RuntimeError, match="kind must be one of"):
        draw_view_params("val")
    p = draw_view_params("train_w")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        fixmatch_views(torch.zeros(1, 8, 3), [(0, 0, p)])
    with pytest.raises(RuntimeError, match="CPU not supported"):
        DeviceScanSet([np.zeros((4, 3), np.float32)], [np.zeros(4, np.int32)], device="cpu")
    with pytest.raises(RuntimeError, match="reads row 2 of 2"):
        pack_view_jobs([(2, 0, p)], 2, 1)
    with pytest.raises(RuntimeError, match="each row once"):
        pack_view_jobs([(0, 0, p), (1, 0, p)], 2, 2)
    with pytest.raises(RuntimeError, match="each row once"):
        pack_view_jobs([(0, 1, p)], 2, 1)
    with pytest.raises(RuntimeError, match="s, R, t"):
        pack_view_jobs([(0, 0, {"s": np.ones(3)})], 1, 1)
    with pytest.raises(RuntimeError, match=r"s \(3,\), R \(3,3\), t \(3,\)"):
        pack_view_jobs([(0, 0, dict(p, R=np.eye(4)))], 1, 1)
    with pytest.raises(RuntimeError, match="at least one job"):
        pack_view_jobs([], 1, 1)
    with pytest.raises(RuntimeError, match="must be a DeviceScanSet"):
        cloud_sample_batch(object(), [0], np.zeros((1, 4), np.int64))
    with pytest.raises(RuntimeError, match="must be DeviceScanSets"):
        FixMatchBatcher(None, None, 16)
    with pytest.raises(RuntimeError, match="one label array per scan"):
        DeviceScanSet([], [])
    # the record layout the kernel reads (include/geot_hip.h): ints 0-2, s 4-6, R 7-15 row-major, t 16-18
    strong = {"s": [1, 2, 3], "R": np.arange(9).reshape(3, 3), "t": [7, 8, 9]}
    rec = pack_view_jobs([(1, 0, strong), (0, 1, p)], 2, 2)
    assert rec.shape == (2, 20) and rec.dtype == np.int32
    assert rec[0, :4].tolist() == [1, 0, 3, 0] and rec[1, :4].tolist() == [0, 1, 0, 0]
    assert rec.view(np.float32)[0, 4:19].tolist() == [1, 2, 3, 0, 1, 2, 3, 4, 5, 6, 7, 8, 7, 8, 9]


def test_entry_points_refuse_bad_arguments_without_a_device():
    """hipErrorInvalidValue (1) before any launch: null pointers, non-positive sizes."""
    from geot_amd import _lib
    lib = _lib.load()
    one = 4096          # any non-null address: the checks come before it is used
    ok_views = [1, 8, 1, 1, 1] + [one] * 7 + [None]
    for at, bad in ((0, 0), (1, 0), (1, 400000000), (2, 0), (3, 0), (4, 3), (4, -1), (5, None), (6, None), (9, None), (11, None)):
        args = list(ok_views)
        args[at] = bad
        assert lib.geot_fixmatch_views(*args) == 1, (at, bad)
    ok_batch = [2, 8, 17, 2, 100] + [one] * 12 + [1 << 30, None]
    for at, bad in ((0, 0), (0, 70000), (1, 0), (2, 0), (2, 5000), (3, 0), (4, 0), (5, None), (6, None), (7, None), (9, None),
                    (10, None), (15, None), (16, None), (17, 8)):
        args = list(ok_batch)
        args[at] = bad
        assert lib.geot_cloud_sample_batch(*args) == 1, (at, bad)
    args = list(ok_batch)
    args[3], args[8] = 1, None            # identity scan ids need n_scans >= s
    assert lib.geot_cloud_sample_batch(*args) == 1
    assert lib.geot_cloud_sample_batch_ws_bytes(0, 17) == 0 and lib.geot_cloud_sample_batch_ws_bytes(2, 17) >= 2 * 256 * 3 * 8
    assert _lib.VIEW_JOB_WORDS == 20 and _lib.VIEW_REG_POINTS == 24576
