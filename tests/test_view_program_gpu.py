"""GPU suite of the view programs (geot_view_program; geot_amd/openpoints/dataset/view_program.py, supervised_batch.py, the
`transforms=` route of FixMatchBatcher) against geot_fixmatch_views, the reference-executed fixture
tests/golden/view_program_ref.npz and the restatement of tests/_view_program_ref.py.

Bounds.  Whatever the reference reaches through single fp32 elementwise operations from identical inputs is compared bit for
bit: x where the list separates it from pos before any reduction (cases a, b, d), heights given the same cloud, zeroed rows,
the signs mirroring and flipping leave.  Everything behind a mean, a maximum norm or a rotation is held to B_POS = 1e-5
(atol), the project's figure for this pipeline (tests/test_views_gpu.py); the fixture's own distance e_ref from the fp64
restatement is asserted to be below that bound, so the reference alone stays inside it, and a missing op cannot pass: the
jitter of case a has sigma 1e-3, a hundred times the bound.  Against a rotation in fp64 of the kernel's own arithmetic the
bound is 1e-6 as in tests/test_views_gpu.py: twice the fp32 bound of a 3-term dot product with |p|, |R| <= 1 plus one add."""
import functools
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _view_program_ref as vpr  # noqa: E402
import _views_ref as vr  # noqa: E402
from _view_program_ref import fixture_params  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "view_program_ref.npz")
VIEWS_GOLDEN = os.path.join(HERE, "golden", "fixmatch_views_ref.npz")
B_POS = 1e-5
CASES = ("a", "b", "c", "d")
EXACT_X = ("a", "b", "d")        # x leaves pos before any reduction: single fp32 elementwise operations of the sample


def _fx():
    return np.load(GOLDEN, allow_pickle=False)


def _case(fx, case):
    return [str(n) for n in fx[case + "_names"]], json.loads(str(fx[case + "_kwargs"]))


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def _seed(s):
    np.random.seed(s)
    torch.manual_seed(s)
    random.seed(s)


# ------------------------------------------------------------------------------- 1. the configured lists: geot_fixmatch_views' bits
def _configured():
    meta = json.loads(str(np.load(VIEWS_GOLDEN, allow_pickle=False)["meta"]))
    return {k: [str(n) for n in meta["lists"][k]] for k in ("train", "train_w", "train_s")}


def _as_program_params(names, p):
    """draw_view_params' s / R / t as the per-transform dicts of the three configured lists."""
    pick = {"PointCloudScaling": {"scale": p["s"]}, "PointCloudScaling_s": {"scale": p["s"]}, "PointCloudRotation_s": {"R": p["R"]},
            "PointCloudTranslation_s": {"t": p["t"]}}
    return [dict(pick.get(n, {})) for n in names]


@pytest.mark.parametrize("m", (768, 24576, 30000, 1, 5))
def test_configured_lists_carry_the_bits_of_fixmatch_views(m):
    """m = 24 576 is the largest register-resident cloud, 30 000 streams through the pos row."""
    from geot_amd.openpoints.dataset import TOOTH_VIEW_KWARGS, ViewProgram, draw_view_params, fixmatch_views, view_program_views
    lists = _configured()
    kwargs = dict(TOOTH_VIEW_KWARGS, angle_s=[1, 1, 1])          # real rotations
    programs = {k: ViewProgram(v, kwargs) for k, v in lists.items()}
    rng = np.random.default_rng(m)
    raw = (rng.standard_normal((3, m, 3)) * np.array([.3, .2, .08]) + np.array([.1, -.2, .05])).astype(np.float32)
    if m == 768:
        raw[2, 17, 1] = np.nan                                   # a NaN vertex: both kernels propagate it alike
    _seed(m)
    old, new = [], []
    for row, kind in enumerate(("train", "train_w", "train_s", "train", "train_s", "train_w", "train_s", "train", "train_w")):
        p = draw_view_params(kind, kwargs)
        old.append((row % 3, row, p))
        new.append((row % 3, row, programs[kind], _as_program_params(lists[kind], p)))
    dev_raw = torch.from_numpy(raw).to(DEV)
    want = fixmatch_views(dev_raw, old, kwargs["gravity_dim"], 9)
    got = view_program_views(dev_raw, new, 9)
    torch.cuda.synchronize()
    for k in ("x", "heights", "pos", "view_center", "view_scale"):
        assert _same_bits(got[k], want[k]), (m, k)
    if m == 768:
        assert torch.isnan(got["pos"][2::3]).all() and torch.isfinite(got["pos"][0]).all()
    if m == 1:                                                   # 0 / 0, as the reference: NaN positions, finite x and heights
        assert torch.isnan(got["pos"]).all() and torch.isfinite(got["x"]).all() and torch.isfinite(got["heights"]).all()


def _same_bits_off_nan(got, want):
    """The NaNs where the restatement has them (positions, not payloads), identical bits everywhere else."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


@pytest.mark.parametrize("m, g", ((1, 1), (5, 1), (513, 1), (768, 0), (768, 1), (768, 2), (24576, 1), (24577, 1), (30000, 1)))
def test_configured_lists_against_numpy_alone(m, g):
    """The nine jobs of the test above with every output pinned by numpy, no second kernel: x and heights are the fp32
    statements, view_center the reduction tree of csrc/views.h restated in fp64 (tests/_views_ref.py mean_tree_f64) and
    rounded once, view_scale and pos the fp32 statements given those.  m = 1 and 5 stay below one wave, 513 is the first
    wrap of the 512 threads, 24 576 / 24 577 lie on either side of the register / streaming switch, 30 000 is 59 streaming
    rounds with a last chunk of 3 of VIEW_CHUNK = 4; g: the gravity column.  Where the restatement has a NaN, its place is
    compared, not its sign and payload (which IEEE 754 leaves open, and numpy's subtract and the GPU's differ on: the heights
    of the NaN cloud at g = 1 are finite - NaN); x is the input's own NaN through one multiply and carries identical bits."""
    from geot_amd.openpoints.dataset import TOOTH_VIEW_KWARGS, ViewProgram, draw_view_params, view_program_views
    lists = _configured()
    kwargs = dict(TOOTH_VIEW_KWARGS, angle_s=[1, 1, 1], gravity_dim=g)          # real rotations
    programs = {k: ViewProgram(v, kwargs) for k, v in lists.items()}
    rng = np.random.default_rng(m)
    raw = (rng.standard_normal((3, m, 3)) * np.array([.3, .2, .08]) + np.array([.1, -.2, .05])).astype(np.float32)
    if m == 768:
        raw[2, 17, 1] = np.nan
    _seed(m)
    jobs = []
    for row, kind in enumerate(("train", "train_w", "train_s", "train", "train_s", "train_w", "train_s", "train", "train_w")):
        p = draw_view_params(kind, kwargs)
        jobs.append((row % 3, row, programs[kind], _as_program_params(lists[kind], p)))
    got = view_program_views(torch.from_numpy(raw).to(DEV), jobs, 9)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    for src, row, program, params in jobs:
        f32 = vpr.run(raw[src], program.names, kwargs, params, np.float32)
        q = f32["x"]                                             # the scaled cloud: what the centring op sums
        center = vr.mean_tree_f64(q).astype(np.float32)
        scale = np.float32(vr.norm_f32(q, center))
        want = vpr.run(raw[src], program.names, kwargs, params, np.float32, stats=(center, scale))
        same = {"x": _same_bits(got["x"][row], q.T), "heights": _same_bits_off_nan(got["heights"][row], f32["heights"]),
                "view_center": _same_bits_off_nan(got["view_center"][row], center),
                "view_scale": _same_bits_off_nan(got["view_scale"][row], scale),
                "pos": _same_bits_off_nan(got["pos"][row], want["pos"])}
        print("m=%d g=%d job %d (%d ops): %s" % (m, g, row, len(program.names), same))
        assert all(same.values()), (m, g, row, same)
    if m == 768:
        assert np.isnan(got["pos"][2::3]).all() and np.isfinite(got["pos"][0]).all()
    if m == 1:                                                   # 0 / 0, as the reference: NaN positions, finite x and heights
        assert np.isnan(got["pos"]).all() and np.isfinite(got["x"]).all() and np.isfinite(got["heights"]).all()


# ------------------------------------------------------------------------------------------------ 2. the fixture
def _check_against(case, got, want_f64, want_f32, fixture, i, e_ref):
    """got: pos (m, 3), x (3, m), heights (m, 1) or None of one item (numpy); want_*: restatements of the SAME sample;
    fixture: the reference's values when the sample is the fixture's own (else None)."""
    if case in EXACT_X:
        assert _same_bits(got["x"], want_f32["x"].T), (case, i, "x")
        assert _same_bits(got["heights"], want_f32["heights"]), (case, i, "heights")
        if fixture is not None:
            assert _same_bits(got["x"], fixture["x"]) and _same_bits(got["heights"], fixture["heights"]), (case, i)
    else:
        assert got["heights"] is None and want_f64["heights"] is None
        assert np.array_equal(got["x"].T, got["pos"]), "nothing rebinds: x is pos"
    assert np.array_equal(got["x"] == 0, want_f32["x"].T == 0), (case, i, "zeroed rows")
    if case in ("c", "d"):        # the lists that mirror (both) and flip (c): the signs they leave
        assert np.array_equal(np.signbit(got["pos"]), np.signbit(want_f32["pos"])), (case, i, "flip / mirror signs")
        assert np.array_equal(np.signbit(got["x"]), np.signbit(want_f32["x"].T)), (case, i, "flip / mirror signs of x")
    for key in ("pos", "x"):
        ref = want_f64[key] if key == "pos" else want_f64["x"].T
        err = float(np.abs(got[key].astype(np.float64) - ref).max())
        print("%s %s[%d]: |kernel - fp64| = %.3e (bound %.0e, e_ref %.3e)" % (case, key, i, err, B_POS, e_ref[key]))
        assert err <= B_POS, (case, key, i, err)
        if fixture is not None:
            err = float(np.abs(got[key].astype(np.float64) - fixture[key].astype(np.float64)).max())
            print("%s %s[%d]: |kernel - reference| = %.3e" % (case, key, i, err))
            assert err <= B_POS, (case, key, i, err)


def _e_ref(fx, case):
    e = {k: float(fx["%s_eref_%s" % (case, k)]) for k in ("pos", "x")}
    assert all(v < B_POS for v in e.values()), "the reference alone must stay inside the bound"
    return e


@pytest.mark.parametrize("case", CASES)
def test_fixture_stage_i_programs_on_the_fixtures_own_samples(case):
    from geot_amd.openpoints.dataset import ViewProgram, view_program_views
    fx = _fx()
    names, kwargs = _case(fx, case)
    program = ViewProgram(names, kwargs)
    raw = fx[case + "_raw_pos"]
    params = [fixture_params(fx, case, i) for i in range(3)]
    v = view_program_views(torch.from_numpy(raw).to(DEV), [(i, i, program, params[i]) for i in range(3)], 3)
    assert (v["heights"] is None) == (case == "c")
    for i in range(3):
        got = {k: (None if v[k] is None else v[k][i].cpu().numpy()) for k in ("pos", "x", "heights")}
        fixture = {"pos": fx[case + "_b_pos"][i], "x": fx[case + "_b_x"][i],
                   "heights": fx[case + "_b_heights"][i] if case != "c" else None}
        _check_against(case, got, vpr.run(raw[i], names, kwargs, params[i], np.float64),
                       vpr.run(raw[i], names, kwargs, params[i], np.float32), fixture, i, _e_ref(fx, case))


def _fixture_set(fx):
    from geot_amd.openpoints.dataset import DeviceScanSet
    return DeviceScanSet([fx["scan%d" % i] for i in range(3)], [fx["lab%d" % i] for i in range(3)], cls=fx["cls"], device=DEV)


@pytest.mark.parametrize("case", CASES)
def test_fixture_stage_ii_the_supervised_batcher_on_the_fixtures_scans(case):
    from geot_amd.openpoints.dataset import SupervisedBatcher, cloud_sample_batch
    fx = _fx()
    names, kwargs = _case(fx, case)
    scans = _fixture_set(fx)
    batcher = SupervisedBatcher(scans, int(fx["num_points"]), int(fx["num_classes"]), transforms=names, kwargs=kwargs)
    params = [fixture_params(fx, case, i) for i in range(3)]
    data = batcher.batch([0, 1, 2], sel=fx[case + "_sel"], params=params, check=True)
    prefix = case + "_b_"
    want_keys = {k[len(prefix):] for k in fx.files if k.startswith(prefix)}
    assert set(data) == want_keys, sorted(set(data) ^ want_keys)
    for k in sorted(want_keys):
        want = fx[prefix + k]
        assert tuple(data[k].shape) == want.shape and data[k].is_cuda and data[k].is_contiguous(), (k, data[k].shape, want.shape)
        assert str(data[k].dtype).replace("torch.", "") == str(want.dtype), (k, data[k].dtype, want.dtype)
        if k in ("y", "cls", "class_weights"):
            assert np.array_equal(data[k].cpu().numpy(), want), k
    # the views against the restatement applied to OUR samples (the reference's numpy pc_norm sums in fp32, ours in fp64:
    # the samples agree to prepare_sample's bound, not in bits)
    ours = cloud_sample_batch(scans, [0, 1, 2], fx[case + "_sel"], int(fx["num_classes"]))["raw"].cpu().numpy()
    np.testing.assert_allclose(ours, fx[case + "_raw_pos"], rtol=0, atol=1e-5)
    for i in range(3):
        got = {k: (data[k][i].cpu().numpy() if k in data else None) for k in ("pos", "x", "heights")}
        _check_against(case, got, vpr.run(ours[i], names, kwargs, params[i], np.float64),
                       vpr.run(ours[i], names, kwargs, params[i], np.float32), None, i, _e_ref(fx, case))
    # seeded as the fixture's maker was, the batcher's own draws are the recorded ones: the same batch
    _seed(int(fx[case + "_seed"]))
    again = batcher.batch([0, 1, 2])
    assert all(_same_bits(again[k], data[k]) for k in data), case


# ------------------------------------------------------------------------------------------------ 3. full size
SCAN_VERTICES = (90000, 130000, 104729, 117000)


@functools.lru_cache(maxsize=None)
def _full_size_scans():
    from geot_amd.openpoints.dataset import DeviceScanSet
    rng = np.random.default_rng(2025)
    scans, labels = [], []
    for n in SCAN_VERTICES:           # millimetres, far from the origin, anisotropic
        scans.append((rng.standard_normal((n, 3)) * np.array([30, 20, 8]) + np.array([250, -400, 120])).astype(np.float32))
        labels.append(rng.integers(0, 17, n).astype(np.int32))
    return DeviceScanSet(scans, labels, device=DEV)


@functools.lru_cache(maxsize=None)
def _full(m):
    """The fixture's four lists on four full-size samples each, fresh draws -> numpy results, job 4 * case + scan."""
    from geot_amd.openpoints.dataset import ViewProgram, cloud_sample_batch, view_program_views
    fx = _fx()
    rng = np.random.default_rng(m)
    sel = np.stack([rng.choice(n, m, replace=n < m) for n in SCAN_VERTICES])
    raw = cloud_sample_batch(_full_size_scans(), [0, 1, 2, 3], sel, 17)["raw"]
    _seed(m)
    jobs, meta = [], []
    for c, case in enumerate(CASES):
        names, kwargs = _case(fx, case)
        program = ViewProgram(names, kwargs)
        for i in range(4):
            params = program.draw(m)
            jobs.append((i, 4 * c + i, program, params))
            meta.append((case, names, kwargs, params, i))
    v = view_program_views(raw, jobs, 16)
    again = view_program_views(raw, jobs, 16)
    rows_h = [r for r in range(16) if meta[r][0] != "c"]           # (the heights rows of case c's jobs are never written)
    for k in ("pos", "x", "view_center", "view_scale"):
        assert _same_bits(v[k], again[k]), "not reproducible call to call: " + k
    assert _same_bits(v["heights"][rows_h], again["heights"][rows_h])
    return raw.cpu().numpy(), meta, {k: t.cpu().numpy() for k, t in v.items()}


@pytest.mark.parametrize("m", (16000, 24000, 30000))
def test_full_size_against_fp64(m):
    raw, meta, v = _full(m)
    for row, (case, names, kwargs, params, i) in enumerate(meta):
        ref = vpr.run(raw[i], names, kwargs, params, np.float64)
        f32 = vpr.run(raw[i], names, kwargs, params, np.float32)
        for key, want in (("pos", ref["pos"]), ("x", ref["x"].T)):
            err = float(np.abs(v[key][row].astype(np.float64) - want).max())
            print("m=%d case %s scan %d: |%s - fp64| = %.3e" % (m, case, i, key, err))
            assert err <= B_POS, (m, case, i, key, err)
        if case in EXACT_X:
            assert _same_bits(v["x"][row], f32["x"].T) and _same_bits(v["heights"][row], f32["heights"]), (m, case, i)
        else:
            assert np.array_equal(v["x"][row].T, v["pos"][row])
            dropped = params[-1]["mask"] == 0
            assert dropped.any() and not v["pos"][row][dropped].any() and v["pos"][row][~dropped].any(axis=1).all()
        if case != "d":
            # the mean: every coordinate entering it has been through at most 4 fp32 roundings at magnitude <= 2 (the fp64
            # restatement rounds none of them): 4 * 2^-23 = 4.8e-7 each, the mean of them no more, plus its own rounding
            assert (np.abs(v["view_center"][row].astype(np.float64) - ref["center"]) <= 1e-6).all()
        else:
            assert not v["view_center"][row].any()
        if case == "c":
            assert v["view_scale"][row] == 1
        else:
            assert abs(float(v["view_scale"][row]) - float(ref["scale"])) <= 1e-5 * float(ref["scale"])


@pytest.mark.parametrize("m", (16000, 24000, 30000))
def test_bits_given_the_kernels_statistics(m):
    """The kernel's mean and maximum norm fed to the fp32 statements on the CPU: what follows them is single fp32 operations
    and carries identical bits (the idiom of tests/test_views_gpu.py).  Case b rotates: against the same statements the
    bound is the rotation's, 1e-6, and whether the bits agree as well is printed."""
    raw, meta, v = _full(m)
    for row, (case, names, kwargs, params, i) in enumerate(meta):
        want = vpr.run(raw[i], names, kwargs, params, np.float32, stats=(v["view_center"][row], v["view_scale"][row]))
        same = np.array_equal(_bits(v["pos"][row]), _bits(want["pos"]))
        if case == "b":
            err = float(np.abs(v["pos"][row].astype(np.float64) - want["pos"].astype(np.float64)).max())
            print("m=%d case b scan %d: bits equal: %s, |pos - fp32 statements| = %.3e" % (m, i, same, err))
            assert err <= 1e-6
        else:
            assert same, (m, case, i)
        assert _same_bits(v["x"][row], want["x"].T), (m, case, i)
        if case in EXACT_X:
            assert _same_bits(v["heights"][row], want["heights"]), (m, case, i)


# ------------------------------------------------------------------------------------------------ 4. reproducibility and hygiene
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


def _equal(a, b):
    assert set(a) == set(b)
    for k in a:
        assert _same_bits(a[k], b[k]), k


def test_two_calls_and_two_batchers_agree():
    from geot_amd.openpoints.dataset import SupervisedBatcher
    lab, _ = _synthetic_sets()
    first, second = SupervisedBatcher(lab, M_STEP), SupervisedBatcher(lab, M_STEP)
    _seed(5)
    sel, params = first.draw([0, 2, 1])
    runs = [b.batch([0, 2, 1], sel=sel, params=params) for b in (first, first, second)]
    _equal(runs[0], runs[1])
    _equal(runs[0], runs[2])
    assert runs[0]["pos"].data_ptr() != runs[1]["pos"].data_ptr()                  # freshly allocated
    _seed(5)
    _equal(runs[0], first.batch([0, 2, 1]))       # seeded alike, the default draws give the same batch as the explicit ones
    assert set(runs[0]) == {"pos", "x", "heights", "y", "cls", "class_weights"}
    assert runs[0]["pos"].shape == (3, M_STEP, 3) and runs[0]["x"].shape == (3, 3, M_STEP) and runs[0]["heights"].shape == (3, M_STEP, 1)
    assert runs[0]["y"].dtype == torch.int64 and runs[0]["cls"].shape == (3, 1) and runs[0]["class_weights"].shape == (3, 17)
    # the jitter is there: pos is not what the list gives without it (sigma 1e-3 against a bound of 1e-5)
    plain = SupervisedBatcher(lab, M_STEP, transforms=["PointsToTensor", "PointCloudScaling", "PointCloudCenterAndNormalize"])
    bare = plain.batch([0, 2, 1], sel=sel, params=[p[:3] for p in params])
    assert _same_bits(bare["x"], runs[0]["x"]) or any(p[4]["drop"] for p in params)
    assert float((bare["pos"] - runs[0]["pos"]).abs().max()) > 1e-4


def test_a_batch_does_not_synchronise():
    """torch's sync debug mode raises on a synchronising HIP call (checked first: .item() under it raises here)."""
    from geot_amd.openpoints.dataset import SupervisedBatcher
    lab, _ = _synthetic_sets()
    batcher = SupervisedBatcher(lab, M_STEP)
    warm = batcher.batch([0, 1])                        # warm: kernels, the pinned pool, the allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError, match="synchroniz"):
            warm["pos"].sum().item()
        for i in range(3):
            data = batcher.batch([i % 3, 1])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert bool(torch.isfinite(data["pos"]).all()) and bool(torch.isfinite(data["x"]).all())


def _new_step():
    from geot_amd.openpoints.models.backbone.transformer import PointTransformer_seg_T
    from geot_amd.train_step import SupervisedStep
    torch.manual_seed(5)
    net = PointTransformer_seg_T(**SMALL).to(DEV)
    return net, SupervisedStep(net)


def test_a_side_stream_batch_beside_a_running_step_equals_the_inline_batch():
    from geot_amd.openpoints.dataset import SupervisedBatcher
    lab, _ = _synthetic_sets()
    inline = SupervisedBatcher(lab, M_STEP)
    side = SupervisedBatcher(lab, M_STEP, stream=torch.cuda.Stream(device=DEV))
    _seed(9)
    sel, params = inline.draw([1, 2])
    cur = inline.batch([0, 1])
    want = inline.batch([1, 2], sel=sel, params=params)
    _, step = _new_step()
    step(cur["pos"], cur["cls"], cur["y"])              # warm: allocations, kernels
    torch.cuda.synchronize()
    loss = step(cur["pos"], cur["cls"], cur["y"])       # queued on the main stream, still running ...
    got = side.batch([1, 2], sel=sel, params=params)    # ... while this is queued beside it
    side.join(got)
    torch.cuda.synchronize()
    _equal(want, got)
    assert bool(torch.isfinite(loss))


def test_batches_feed_the_supervised_step_and_its_look_ahead():
    from geot_amd.openpoints.dataset import SupervisedBatcher
    lab, _ = _synthetic_sets()
    batcher = SupervisedBatcher(lab, M_STEP)
    _seed(21)
    first, second = batcher.batch([0, 1]), batcher.batch([2, 0])
    net, step = _new_step()
    grouped, offered = [], []
    net.group_divider.register_forward_hook(lambda mod, args, out: grouped.append(args[0]))
    forward = net._forward

    def spy(pts, x, cls_label, T, geometry=None):
        offered.append(geometry is not None and geometry.pts is pts and geometry.version == pts._version)
        return forward(pts, x, cls_label, T, geometry)
    net._forward = spy
    l0 = step(first["pos"], first["cls"], first["y"], next_pos=second["pos"])
    assert step._geometry is not None and step._geometry.pts is second["pos"]
    assert len(grouped) == 2 and grouped[0] is first["pos"] and grouped[1] is second["pos"]
    l1 = step(second["pos"], second["cls"], second["y"])
    torch.cuda.synchronize()
    assert offered == [False, True], "the queued geometry did not reach the model, or not for this tensor and version"
    assert len(grouped) == 2, "the look-ahead geometry was recomputed, not used"
    assert bool(torch.isfinite(l0)) and bool(torch.isfinite(l1))


# ------------------------------------------------------------------------------------------------ 5. FixMatchBatcher
def test_fixmatch_batcher_default_is_the_parents_path_and_the_programs_give_its_bits():
    from geot_amd.openpoints.dataset import FixMatchBatcher, TOOTH_VIEW_KWARGS, cloud_sample_batch, fixmatch_views
    lab, unl = _synthetic_sets()
    lists = _configured()
    for kwargs in (TOOTH_VIEW_KWARGS, dict(TOOTH_VIEW_KWARGS, angle_s=[1, 1, 1])):
        plain = FixMatchBatcher(lab, unl, M_STEP, kwargs=kwargs)
        assert plain.programs is None
        routed = FixMatchBatcher(lab, unl, M_STEP, kwargs=kwargs, transforms=lists)
        _seed(31)
        sel, params = plain.draw([0, 2], [1, 0])
        data, data_u = plain.batch([0, 2], [1, 0], sel_l=sel[:2], sel_u=sel[2:], params=params)
        # transforms=None: what the parent composes -- cloud_sample_batch + geot_fixmatch_views on these draws
        s = cloud_sample_batch(plain.scans, [0, 2, 3 + 1, 3 + 0], sel, 17)
        jobs = [(i, i, params[i]) for i in range(2)] + [(2 + i, 2 + i, params[2 + i][0]) for i in range(2)] + \
            [(2 + i, 4 + i, params[2 + i][1]) for i in range(2)]
        v = fixmatch_views(s["raw"], jobs, kwargs["gravity_dim"], 6)
        for k in ("pos", "x", "heights"):
            assert _same_bits(data[k], v[k][:2]) and _same_bits(data_u[k + "_w"], v[k][2:4]) and _same_bits(data_u[k + "_s"], v[k][4:])
        assert _same_bits(data_u["raw_pos"], s["raw"][2:]) and _same_bits(data["y"], s["y"][:2])
        # transforms = the configured lists: seeded alike, the programs draw the same numbers and give the same bits
        _seed(31)
        got, got_u = routed.batch([0, 2], [1, 0])
        _equal(data, got)
        _equal(data_u, got_u)
    with pytest.raises(RuntimeError, match="PointCloudCenterAndNormalize"):
        FixMatchBatcher(lab, unl, M_STEP, transforms=dict(lists, train_w=["PointsToTensor"]))
    with pytest.raises(NotImplementedError, match="RandomDropout"):
        FixMatchBatcher(lab, unl, M_STEP, transforms=dict(lists, train_s=lists["train_s"] + ["RandomDropout"]))
    # an alternative strong list of the yaml's comment runs on the device path
    strong = ["PointsToTensor", "PointCloudScaling_s", "PointCloudJitter_s", "PointCloudCenterAndNormalize", "PointCloudRotation_s",
              "PointCloudTranslation_s"]
    other = FixMatchBatcher(lab, unl, M_STEP, kwargs=dict(TOOTH_VIEW_KWARGS, mirror=[0.5, 0.5, 0.5]), transforms=dict(lists, train_s=strong))
    _seed(32)
    d, du = other.batch([0, 1], [2, 0])
    assert bool(torch.isfinite(du["pos_s"]).all()) and du["pos_s"].shape == (2, M_STEP, 3) and du["x_s"].shape == (2, 3, M_STEP)
