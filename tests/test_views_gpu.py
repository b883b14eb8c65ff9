"""GPU suite of the FixMatch batcher (geot_amd/openpoints/dataset/fixmatch_batch.py; geot_cloud_sample_batch,
geot_fixmatch_views) against the reference-executed fixture tests/golden/fixmatch_views_ref.npz, the fp64 restatement of
tests/_views_ref.py and prepare_sample.

Bounds.  B_POS = 1e-5 (atol) is the project's figure for this pipeline (tests/test_data_gpu.py holds prepare_sample to it) and
the kernel-versus-fp64 bound of the full-size test; against the fixture a position may additionally be off by the
reference's own distance e_ref from the fp64 restatement (stored per key by the fixture's maker): triangle inequality, no
free margin.  x and heights are one rounding of identical inputs and are compared exactly.  The strong view's rotation and
shift are held to 1e-6 against fp64 applied to the kernel's own pre-rotation positions: twice the fp32 bound of a 3-term dot
product with |p|, |R| <= 1 plus one add."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _views_ref as vr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fixmatch_views_ref.npz")
B_POS = 1e-5
CASES = ("cfg", "rot")
EYE, ZERO, ONE = np.eye(3, dtype=np.float32), np.zeros(3, np.float32), np.ones(3, np.float32)


def _fx():
    return np.load(GOLDEN, allow_pickle=False)


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def _params(s=ONE, R=EYE, t=ZERO, strong=False):
    return {"s": s, "R": R, "t": t, "rotate": strong, "translate": strong}


def _fixture_params(fx, case):
    lab = [_params(fx[case + "_l_s"][i]) for i in range(3)]
    unl = [(_params(), _params(fx[case + "_u_s_s"][i], fx[case + "_u_R_s"][i], fx[case + "_u_t_s"][i], True)) for i in range(3)]
    return lab + unl


def _jobs(params, bl, bu):
    """The batcher's job order: labelled rows, weak rows, strong rows."""
    return ([(i, i, params[i]) for i in range(bl)] + [(bl + i, bl + i, params[bl + i][0]) for i in range(bu)]
            + [(bl + i, bl + bu + i, params[bl + i][1]) for i in range(bu)])


def _check_views(fx, case, views, raw, g, against_fixture):
    """views: pos / x / heights with rows [labelled 0-2, weak 3-5, strong 6-8]; raw (6, m, 3) what they were made of."""
    params = _fixture_params(fx, case)
    rows = [("l_", "", i, i, params[i]) for i in range(3)]
    rows += [("u_", "_w", i, 3 + i, params[3 + i][0]) for i in range(3)] + [("u_", "_s", i, 6 + i, params[3 + i][1]) for i in range(3)]
    for side, suffix, i, row, p in rows:
        e_ref = float(fx["%s_eref_%spos%s" % (case, side, suffix)])
        ref = vr.view_f64(raw[3 + i if side == "u_" else i], p["s"], p["R"], p["t"], g, p["rotate"], p["translate"])
        x, h, pos = (views[k][row].cpu().numpy() for k in ("x", "heights", "pos"))
        if against_fixture:
            want_x, want_h = fx[case + "_" + side + "x" + suffix][i], fx[case + "_" + side + "heights" + suffix][i]
            want_pos = fx[case + "_" + side + "pos" + suffix][i].astype(np.float64)
        else:
            want_x, want_h, want_pos = ref["x"].T, ref["heights"], ref["pos"]
        assert _same_bits(x, want_x), (case, side, suffix, i, "x")
        assert _same_bits(h, want_h), (case, side, suffix, i, "heights")
        err = float(np.abs(pos.astype(np.float64) - want_pos).max())
        print("%s %spos%s[%d]: %.3e (e_ref %.3e + b %.0e)" % (case, side, suffix, i, err, e_ref, B_POS))
        assert err <= e_ref + B_POS, (case, side, suffix, i, err)


# ------------------------------------------------------------------------------------------------ 1. the fixture
@pytest.mark.parametrize("case", CASES)
def test_fixture_stage_i_views_of_the_fixtures_own_samples(case):
    from geot_amd.openpoints.dataset import fixmatch_views
    fx = _fx()
    g = json.loads(str(fx[case + "_kwargs"]))["gravity_dim"]
    raw = np.concatenate([fx[case + "_l_raw_pos"], fx[case + "_u_raw_pos"]])
    v = fixmatch_views(torch.from_numpy(raw).to(DEV), _jobs(_fixture_params(fx, case), 3, 3), g, 9)
    _check_views(fx, case, v, raw, g, against_fixture=True)


def _fixture_sets(fx):
    from geot_amd.openpoints.dataset import DeviceScanSet
    sets = []
    for split in ("l", "u"):
        sets.append(DeviceScanSet([fx["scan_%s%d" % (split, i)] for i in range(3)], [fx["lab_%s%d" % (split, i)] for i in range(3)],
                                  cls=fx["cls_" + split], device=DEV))
    return sets


@pytest.mark.parametrize("case", CASES)
def test_fixture_stage_ii_the_batcher_on_the_fixtures_scans(case):
    from geot_amd.openpoints.dataset import FixMatchBatcher, cloud_sample_batch
    fx = _fx()
    kwargs = json.loads(str(fx[case + "_kwargs"]))
    lab, unl = _fixture_sets(fx)
    batcher = FixMatchBatcher(lab, unl, int(fx["num_points"]), int(fx["num_classes"]), kwargs=kwargs)
    data, data_u = batcher.batch([0, 1, 2], [0, 1, 2], sel_l=fx[case + "_l_sel"], sel_u=fx[case + "_u_sel"],
                                 params=_fixture_params(fx, case), check=True)
    for side, got in (("l_", data), ("u_", data_u)):
        prefix = case + "_" + side
        want_keys = {k[len(prefix):] for k in fx.files if k.startswith(prefix)} - {"sel", "s", "s_s", "R_s", "t_s", "theta", "perm"}
        if side == "l_":
            want_keys -= {"raw_pos"}          # (the fixture's extra: the labelled items' untransformed sample)
        assert set(got) == want_keys, (side, sorted(set(got) ^ want_keys))
        for k in sorted(want_keys):
            want = fx[prefix + k]
            assert tuple(got[k].shape) == want.shape and got[k].is_cuda and got[k].is_contiguous(), (side, k, got[k].shape, want.shape)
            assert str(got[k].dtype).replace("torch.", "") == str(want.dtype), (side, k, got[k].dtype, want.dtype)
            if k.startswith(("y", "cls", "class_weights")):
                assert np.array_equal(got[k].cpu().numpy(), want), (side, k)
    # the untransformed sample: the reference's numpy pc_norm sums in fp32, ours in fp64 -- prepare_sample's bound
    for k in ("raw_pos", "pos", "x"):
        np.testing.assert_allclose(data_u[k].cpu().numpy(), fx[case + "_u_" + k], rtol=0, atol=1e-5)
    # the views, against the restatement applied to OUR samples
    ours = cloud_sample_batch(batcher.scans, [0, 1, 2, 3, 4, 5], np.concatenate([fx[case + "_l_sel"], fx[case + "_u_sel"]]),
                              int(fx["num_classes"]))
    assert torch.equal(ours["raw"][3:], data_u["raw_pos"])
    np.testing.assert_allclose(ours["raw"][:3].cpu().numpy(), fx[case + "_l_raw_pos"], rtol=0, atol=1e-5)
    views = {k: torch.cat([data[k], data_u[k + "_w"], data_u[k + "_s"]]) for k in ("pos", "x", "heights")}
    _check_views(fx, case, views, ours["raw"].cpu().numpy(), kwargs["gravity_dim"], against_fixture=False)


# ------------------------------------------------------------------------------------------------ 2. / 3. full size
SIZES = (16000, 24000, 24577, 40000, 1, 5)
SCAN_VERTICES = (90000, 130000, 104729, 117000)


@functools.lru_cache(maxsize=None)
def _full_size_scans():
    from geot_amd.openpoints.dataset import DeviceScanSet
    rng = np.random.default_rng(2024)
    scans, labels = [], []
    for n in SCAN_VERTICES:           # millimetres, far from the origin, anisotropic
        scans.append((rng.standard_normal((n, 3)) * np.array([30, 20, 8]) + np.array([250, -400, 120])).astype(np.float32))
        labels.append(rng.integers(0, 17, n).astype(np.int32))
    return DeviceScanSet(scans, labels, device=DEV)


def _rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _full(m):
    """S = 4 scans, per scan a labelled-like, a weak, a strong (R != I) and a strong-with-R = I view -> numpy results."""
    from geot_amd.openpoints.dataset import cloud_sample_batch, fixmatch_views
    scans = _full_size_scans()
    rng = np.random.default_rng(m)
    sel = np.stack([rng.choice(n, m, replace=n < m) for n in SCAN_VERTICES])
    s = cloud_sample_batch(scans, [0, 1, 2, 3], sel, 17)
    params = []
    for i in range(4):
        params.append([_params(rng.uniform(0.9, 1.1, 3).astype(np.float32)), _params(),
                       _params(rng.uniform(0.8, 1.2, 3).astype(np.float32), _rotation(rng), rng.uniform(0, 0.2, 3).astype(np.float32), True),
                       _params(rng.uniform(0.8, 1.2, 3).astype(np.float32), EYE, rng.uniform(0, 0.2, 3).astype(np.float32), True)])
    jobs = [(i, 4 * i + k, params[i][k]) for i in range(4) for k in range(4)]
    v = fixmatch_views(s["raw"], jobs, 1, 16)
    again = fixmatch_views(s["raw"], jobs, 1, 16)
    assert all(_same_bits(v[k], again[k]) for k in v), "not reproducible call to call"
    return s["raw"].cpu().numpy(), params, {k: t.cpu().numpy() for k, t in v.items()}


@pytest.mark.parametrize("m", SIZES)
def test_full_size_against_fp64(m):
    raw, params, v = _full(m)
    for i in range(4):
        for k in range(4):
            p, row = params[i][k], 4 * i + k
            ref = vr.view_f64(raw[i], p["s"], p["R"], p["t"], 1, p["rotate"], p["translate"])
            assert _same_bits(v["x"][row], ref["x"].T) and _same_bits(v["heights"][row], ref["heights"])
            assert np.isfinite(v["x"][row]).all() and np.isfinite(v["heights"][row]).all()
            # the mean: fp64 sums rounded once -> within one fp32 rounding of the fp64 mean
            assert (np.abs(v["view_center"][row].astype(np.float64) - ref["center"]) <= vr.EPS32 * np.abs(ref["center"]) + 1e-15).all()
            if m == 1:           # 0 / 0, as the reference: NaN positions, finite x and heights
                assert v["view_scale"][row] == 0 and ref["scale"] == 0
                assert np.isnan(v["pos"][row]).all() and np.isnan(ref["pos"]).all()
                continue
            assert abs(float(v["view_scale"][row]) - ref["scale"]) <= 1e-5 * ref["scale"]
            err = float(np.abs(v["pos"][row].astype(np.float64) - ref["pos"]).max())
            print("m=%d scan %d view %d: |pos - fp64| = %.3e" % (m, i, k, err))
            assert np.allclose(v["pos"][row].astype(np.float64), ref["pos"], rtol=0, atol=B_POS, equal_nan=True), err
            if p["rotate"]:
                pre = vr.pos_f32_given_stats(raw[i], p["s"], p["R"], p["t"], v["view_center"][row], v["view_scale"][row], False, False)
                err_r = float(np.abs(v["pos"][row].astype(np.float64) - vr.rotate_f64(pre, p["R"], p["t"])).max())
                print("m=%d scan %d view %d: |pos_s - fp64 rotation of the kernel's pre-rotation pos| = %.3e" % (m, i, k, err_r))
                assert err_r <= 1e-6


@pytest.mark.parametrize("m", SIZES)
def test_bits_given_the_kernels_statistics(m):
    """The kernel's mean and maximum norm fed to the fp32 statements on the CPU: pos, pos_w and (R = I) pos_s carry identical
    bits -- the idiom of test_prepare_sample_matches_numpy_pipeline; so does the maximum norm given the mean."""
    raw, params, v = _full(m)
    for i in range(4):
        for k in (0, 1, 3):
            p, row = params[i][k], 4 * i + k
            want = vr.pos_f32_given_stats(raw[i], p["s"], p["R"], p["t"], v["view_center"][row], v["view_scale"][row],
                                          p["rotate"], p["translate"])
            assert np.array_equal(_bits(v["pos"][row]), _bits(want)), (m, i, k)
            assert _same_bits(np.float32(vr.norm_f32(vr.scaled(raw[i], p["s"]), v["view_center"][row])), v["view_scale"][row])


def test_rotate_and_translate_are_independent_flags():
    """One cloud, the four (rotate, translate) combinations in one launch, each held bit for bit to the fp32 statements
    with the same flags given the kernel's statistics (the other tests set both flags or neither).  m = 768: two rounds
    of the 512 threads, the second half empty."""
    from geot_amd.openpoints.dataset import fixmatch_views
    rng = np.random.default_rng(768)
    raw = (rng.standard_normal((1, 768, 3)) * np.array([.3, .2, .08]) + np.array([.1, -.2, .05])).astype(np.float32)
    s, R, t = rng.uniform(0.8, 1.2, 3).astype(np.float32), _rotation(rng), rng.uniform(0, 0.2, 3).astype(np.float32)
    flags = [(False, False), (True, False), (False, True), (True, True)]
    jobs = [(0, k, {"s": s, "R": R, "t": t, "rotate": rot, "translate": tr}) for k, (rot, tr) in enumerate(flags)]
    v = {k: a.cpu().numpy() for k, a in fixmatch_views(torch.from_numpy(raw).to(DEV), jobs, 1, 4).items()}
    for k, (rot, tr) in enumerate(flags):
        want = vr.pos_f32_given_stats(raw[0], s, R, t, v["view_center"][k], v["view_scale"][k], rot, tr)
        err = float(np.abs(v["pos"][k].astype(np.float64) - want.astype(np.float64)).max())
        print("rotate %s translate %s: bits equal %s, |pos - fp32 statements| = %.3e" % (rot, tr, _same_bits(v["pos"][k], want), err))
        assert _same_bits(v["pos"][k], want), (rot, tr, err)
        assert _same_bits(v["x"][k], vr.scaled(raw[0], s).T) and _same_bits(v["view_center"][k], v["view_center"][0])
    assert not _same_bits(v["pos"][1], v["pos"][0]) and not _same_bits(v["pos"][2], v["pos"][0]) and not _same_bits(v["pos"][3], v["pos"][1])


# ------------------------------------------------------------------------------------------------ 4. the batched sampler
RAGGED = (1, 700, 5000, 100000, 1234)


def _ragged_set():
    from geot_amd.openpoints.dataset import DeviceScanSet
    rng = np.random.default_rng(11)
    scans = [(rng.standard_normal((n, 3)) * np.array([30, 20, 8]) + np.array([5, -40, 12])).astype(np.float32) for n in RAGGED]
    labels = [rng.integers(0, 17, n).astype(np.int32) for n in RAGGED]
    return scans, labels, DeviceScanSet(scans, labels, device=DEV)


def test_cloud_sample_batch_equals_prepare_sample_scan_by_scan():
    from geot_amd.openpoints.dataset import cloud_sample_batch, prepare_sample
    scans, labels, dset = _ragged_set()
    m, ids = 2048, [3, 0, 4, 1, 1, 2]              # n < m for three of the five scans, a 1-vertex scan, a scan twice
    rng = np.random.default_rng(12)
    sel = np.stack([rng.choice(RAGGED[i], m, replace=RAGGED[i] < m) for i in ids])
    got = cloud_sample_batch(dset, ids, sel, 17)
    assert got["bad"].tolist() == [0] * len(ids)
    for slot, i in enumerate(ids):
        one = prepare_sample(torch.from_numpy(scans[i]).to(DEV), torch.from_numpy(labels[i]).to(DEV), torch.from_numpy(sel[slot]).to(DEV))
        for ours, theirs in (("raw", "pos"), ("y", "y"), ("class_weights", "class_weights"), ("center", "center"), ("scale", "scale")):
            assert _same_bits(got[ours][slot], one[theirs]), (slot, i, ours)     # (bits: the 1-vertex scan's 0 / 0 is NaN)
    assert got["y"].dtype == torch.int64 and torch.isnan(got["raw"][1]).all() and float(got["scale"][1]) == 0


def test_bad_index_flags_its_scan_only():
    from geot_amd.openpoints.dataset import DeviceScanSet, FixMatchBatcher, cloud_sample_batch
    scans, labels, dset = _ragged_set()
    m, ids = 512, [1, 2, 4, 3]
    rng = np.random.default_rng(13)
    sel = np.stack([rng.choice(RAGGED[i], m, replace=RAGGED[i] < m) for i in ids])
    clean = cloud_sample_batch(dset, ids, sel, 17)
    sel_bad = sel.copy()
    sel_bad[2, 77] = RAGGED[4]                     # one past the end of slot 2's scan
    sel_bad[2, 78] = -1
    got = cloud_sample_batch(dset, ids, sel_bad, 17, check=False)
    assert got["bad"].tolist() == [0, 0, 1, 0]
    for k in ("raw", "y", "class_weights", "center", "scale"):
        assert all(_same_bits(got[k][s], clean[k][s]) for s in (0, 1, 3)), k
    with pytest.raises(IndexError, match="slot 2"):
        cloud_sample_batch(dset, ids, sel_bad, 17, check=True)
    lab = DeviceScanSet(scans[1:3], labels[1:3], device=DEV)
    unl = DeviceScanSet(scans[3:], labels[3:], device=DEV)
    batcher = FixMatchBatcher(lab, unl, m)
    ok = batcher.batch([0, 1], [1, 0], sel_l=sel[:2], sel_u=sel[2:], check=True)
    assert ok[0]["pos"].shape == (2, m, 3)
    with pytest.raises(IndexError, match="slot 2"):
        batcher.batch([0, 1], [1, 0], sel_l=sel_bad[:2], sel_u=sel_bad[2:], check=True)
    batcher.batch([0, 1], [1, 0], sel_l=sel_bad[:2], sel_u=sel_bad[2:])            # the default does not read the flags


# ------------------------------------------------------------------------------------------------ 5. reproducibility and hygiene
SMALL = dict(trans_dim=384, depth=3, num_heads=4, group_size=32, num_group=128, encoder_dims=256, nclasses=17,
             drop_path_rate=0.1, downsample_targets=[2048, 1024, 512], extract_layers=[1, 2, 3])
M_STEP = 4096


def _synthetic_sets(vertices=12000):
    from geot_amd.openpoints.dataset import DeviceScanSet
    from geot_amd.synth import make_batch, region_labels
    sets = []
    for start in (3, 60):
        xyz = make_batch(3, vertices, start_index=start)[0]
        pts = [(xyz[i] * np.float32(25) + np.array([10, -30, 55], np.float32)).astype(np.float32) for i in range(3)]
        labs = [region_labels(xyz[i:i + 1])[0].astype(np.int32) for i in range(3)]
        sets.append(DeviceScanSet(pts, labs, cls=[0, 1, 0], device=DEV))
    return sets


def _equal_batches(a, b):
    for da, db in zip(a, b):
        assert set(da) == set(db)
        for k in da:
            assert _same_bits(da[k], db[k]), k


def test_two_calls_and_two_batchers_agree():
    from geot_amd.openpoints.dataset import FixMatchBatcher
    lab, unl = _synthetic_sets()
    first, second = FixMatchBatcher(lab, unl, M_STEP), FixMatchBatcher(lab, unl, M_STEP)
    np.random.seed(5)
    torch.manual_seed(5)
    sel, params = first.draw([0, 2], [1, 0])
    runs = [b.batch([0, 2], [1, 0], sel_l=sel[:2], sel_u=sel[2:], params=params) for b in (first, first, second)]
    _equal_batches(runs[0], runs[1])
    _equal_batches(runs[0], runs[2])
    assert runs[0][0]["pos"].data_ptr() != runs[1][0]["pos"].data_ptr()            # freshly allocated
    # seeded alike, the default draws give the same batch as the explicit ones
    np.random.seed(5)
    torch.manual_seed(5)
    _equal_batches(runs[0], first.batch([0, 2], [1, 0]))
    assert set(runs[0][1]) == {k + sfx for k in ("pos", "x", "y", "cls", "class_weights") for sfx in ("", "_w", "_s")} \
        | {"heights_w", "heights_s", "raw_pos"}
    assert set(runs[0][0]) == {"pos", "x", "y", "cls", "class_weights", "heights"}


def test_a_batch_does_not_synchronise():
    """torch's sync debug mode raises on a synchronising HIP call (checked first: .item() under it raises here)."""
    from geot_amd.openpoints.dataset import FixMatchBatcher
    lab, unl = _synthetic_sets()
    batcher = FixMatchBatcher(lab, unl, M_STEP)
    warm = batcher.batch([0, 1], [0, 1])                # warm: kernels, the pinned pool, the allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError, match="synchroniz"):
            warm[0]["pos"].sum().item()
        for i in range(3):
            data, data_u = batcher.batch([i % 3, 1], [2, i % 3])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert bool(torch.isfinite(data["pos"]).all()) and bool(torch.isfinite(data_u["pos_s"]).all())


def _new_step():
    from geot_amd import train_step as ts
    torch.manual_seed(5)
    return ts.build_fixmatch(DEV, seg_cfg=SMALL, cfg=dict(ts.NTM_CFG, threed_k=8), use_ddp=False)


def test_a_side_stream_batch_beside_a_running_step_equals_the_inline_batch():
    from geot_amd.openpoints.dataset import FixMatchBatcher
    lab, unl = _synthetic_sets()
    inline = FixMatchBatcher(lab, unl, M_STEP)
    side = FixMatchBatcher(lab, unl, M_STEP, stream=torch.cuda.Stream(device=DEV))
    np.random.seed(9)
    torch.manual_seed(9)
    sel, params = inline.draw([1, 2], [0, 2])
    cur = inline.batch([0, 1], [1, 2])
    want = inline.batch([1, 2], [0, 2], sel_l=sel[:2], sel_u=sel[2:], params=params)
    step = _new_step()
    step(cur[0], cur[1])                                 # warm: allocations, kernels
    torch.cuda.synchronize()
    losses = step(cur[0], cur[1])                        # queued on the main stream, still running ...
    got = side.batch([1, 2], [0, 2], sel_l=sel[:2], sel_u=sel[2:], params=params)      # ... while this is queued beside it
    side.join(*got)
    torch.cuda.synchronize()
    _equal_batches(want, got)
    assert all(bool(torch.isfinite(v)) for v in losses.values())


def test_batches_feed_the_step_and_its_look_ahead():
    from geot_amd.openpoints.dataset import FixMatchBatcher
    lab, unl = _synthetic_sets()
    batcher = FixMatchBatcher(lab, unl, M_STEP)
    np.random.seed(21)
    torch.manual_seed(21)
    first, second = batcher.batch([0, 1], [2, 0]), batcher.batch([2, 0], [1, 2])
    step = _new_step()
    seen = []
    iteration = step.iteration

    def spy(data, data_u, geoms=(None, None), next_batches=None):
        seen.append(geoms)
        return iteration(data, data_u, geoms, next_batches)
    step.iteration = spy
    l0 = step(first[0], first[1], next_batches=second)
    assert step._geometry[0] is not None and step._geometry[0].describes([second[0]["pos"], second[1]["pos_s"], second[1]["pos_w"]])
    l1 = step(second[0], second[1])
    torch.cuda.synchronize()
    assert seen[0] == (None, None) and seen[1][0] is not None, "the look-ahead geometry was recomputed, not accepted"
    for losses in (l0, l1):
        assert all(bool(torch.isfinite(v)) for v in losses.values()), losses
