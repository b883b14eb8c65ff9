"""curvatures=True on the four batchers: every dict of a batch holds "curvatures" (B, m) float32 equal, bit for bit, to the numpy
restatement (tests/_curvature_ref.py) of the scan's curvature, normalised over the WHOLE scan and gathered at the sample -- the
given sel, or the "sel" of a covering batch.  With the switch off a batch is the same C-ABI calls, keys and bits as before; with
it on, one geot_curvature_sample more.  Every ValueError comes before any device call."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _curvature_ref as cref  # noqa: E402
import _mesh_ref as mref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, RADIUS = 256, 1.3
_cache = {}


def _world():
    """Two sets of small height-field scans with their meshes and curvature, and the restatement's normalised curvature of
    every scan, computed once."""
    if not _cache:
        from geot_amd.openpoints.dataset import DeviceScanSet
        shapes = [(21, 25), (12, 12), (30, 11), (17, 19)]                  # 525, 144 (fewer than N vertices), 330, 323
        scans = [cref.height_field(r, c, 20 + i) for i, (r, c) in enumerate(shapes)]
        meshes = [mref.shuffled(mref.grid(r, c), i, corners=True) for i, (r, c) in enumerate(shapes)]
        labels = [(np.arange(len(p)) % 17).astype(np.int32) for p in scans]
        want = []
        for p, f in zip(scans, meshes):
            cur, rng, _, _ = cref.curvature(p, f, RADIUS)
            assert rng[1] > rng[0]
            want.append(cref.normalise(cur, rng))
        make = lambda lo, hi, **kw: DeviceScanSet(scans[lo:hi], labels[lo:hi], cls=[0, 1], device=DEV, **kw)       # noqa: E731
        _cache.update(scans=scans, meshes=meshes, labels=labels, want=want,
                      lab=make(0, 2, faces=meshes[0:2]).compute_curvature(RADIUS), unl=make(2, 4, faces=meshes[2:4]).compute_curvature(RADIUS),
                      plain=make(0, 2, faces=meshes[0:2]), bare=make(0, 2), half=make(0, 2, faces=[meshes[0], None]).compute_curvature(RADIUS))
    return _cache


def _sel(sizes, seed):
    rng = np.random.default_rng(seed)
    sel = np.stack([rng.integers(0, n, size=N) for n in sizes])
    sel[:, :4] = [[0, 0, n - 1, n - 1] for n in sizes]                      # first, last, repeated
    return sel


def _same(got, want_rows):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (len(want_rows), N)
    return all(np.array_equal(g, w) for g, w in zip(got, want_rows))


def _traced(fn):
    from geot_amd.ext import _common
    seen = []
    _common.trace = lambda launch, name: (seen.append(name), launch())[1]
    try:
        out = fn()
    finally:
        _common.trace = None
    return seen, out


def _refused(fn, msg, exc=ValueError):
    """fn raises, and not one C-ABI call was made before it did."""
    from geot_amd.ext import _common
    seen = []
    _common.trace = lambda launch, name: (seen.append(name), launch())[1]
    try:
        with pytest.raises(exc, match=msg):
            fn()
    finally:
        _common.trace = None
    assert seen == [], seen


def _seed(k):
    import random
    np.random.seed(k)
    random.seed(k)
    torch.manual_seed(k)


def test_supervised_and_val_and_vote_batches_hold_the_restatement_at_their_sample():
    from geot_amd.openpoints.dataset import SupervisedBatcher, ValBatcher, VoteBatcher
    w = _world()
    idx = [1, 0, 1]
    sel = _sel([len(w["scans"][i]) for i in idx], 1)
    want = [w["want"][i][s] for i, s in zip(idx, sel)]
    for make in (SupervisedBatcher, ValBatcher, VoteBatcher):
        on, off = make(w["lab"], N, curvatures=True), make(w["lab"], N)
        _seed(3)
        launches_on, got = _traced(lambda: on.batch(idx, sel=sel, check=True))
        _seed(3)
        launches_off, base = _traced(lambda: off.batch(idx, sel=sel))
        assert _same(got["curvatures"], want), make.__name__
        assert got["curvatures"].min() >= 0 and got["curvatures"].max() <= 1
        # one launch more, behind the others; every other key holds the same bits
        assert launches_on == launches_off + ["geot_curvature_sample"] and set(got) == set(base) | {"curvatures"}
        assert all(torch.equal(got[k], base[k]) for k in base if torch.is_tensor(base[k]))
        # a sample on the device (a tensor) serves too
        again = on.batch(idx, sel=torch.from_numpy(sel).to(DEV))
        assert torch.equal(again["curvatures"], got["curvatures"])
        # on a side stream, joined
        side = make(w["lab"], N, curvatures=True, stream=torch.cuda.Stream(DEV))
        batch = side.batch(idx, sel=sel)
        side.join(batch)
        assert _same(batch["curvatures"], want)


def test_covering_and_voted_batches_hold_it_at_their_own_sel():
    from geot_amd.openpoints.dataset import ValBatcher, VoteBatcher
    from geot_amd.openpoints.dataset.sample_draw import DeviceDraws
    w = _world()
    idx = [0, 1]
    for make in (ValBatcher, VoteBatcher):
        batcher = make(w["lab"], N, curvatures=True, draws=DeviceDraws(7))
        seen = 0
        for batch in batcher.cover(idx):
            sel = batch["sel"].cpu().numpy()
            assert _same(batch["curvatures"], [w["want"][i][s] for i, s in zip(idx, sel)])
            seen += 1
        assert seen == 3                                    # 525 vertices in passes of 256
        # a drawn batch: the sample is the device's; the values lie in [0, 1] and every one is a value of its scan
        drawn = batcher.batch(idx)["curvatures"].cpu().numpy()
        assert all(np.isin(row, w["want"][i]).all() for i, row in zip(idx, drawn))


def test_fixmatch_batches_hold_it_in_data_and_data_u():
    from geot_amd.openpoints.dataset import FixMatchBatcher
    w = _world()
    idx_l, idx_u = [1, 0], [0, 1, 1]
    sel_l, sel_u = _sel([len(w["scans"][i]) for i in idx_l], 4), _sel([len(w["scans"][2 + i]) for i in idx_u], 5)
    on, off = FixMatchBatcher(w["lab"], w["unl"], N, curvatures=True), FixMatchBatcher(w["lab"], w["unl"], N)
    assert on.scans.curvature_radius == RADIUS and off.scans.curvature is not None           # carried over by _merged
    _seed(5)
    launches_on, (data, data_u) = _traced(lambda: on.batch(idx_l, idx_u, sel_l=sel_l, sel_u=sel_u, check=True))
    _seed(5)
    launches_off, (base, base_u) = _traced(lambda: off.batch(idx_l, idx_u, sel_l=sel_l, sel_u=sel_u))
    assert _same(data["curvatures"], [w["want"][i][s] for i, s in zip(idx_l, sel_l)])
    assert _same(data_u["curvatures"], [w["want"][2 + i][s] for i, s in zip(idx_u, sel_u)])     # ONE tensor for both views
    assert launches_on == launches_off + ["geot_curvature_sample"]
    assert set(data) == set(base) | {"curvatures"} and set(data_u) == set(base_u) | {"curvatures"}
    assert all(torch.equal(data[k], base[k]) for k in base) and all(torch.equal(data_u[k], base_u[k]) for k in base_u)
    on.join(data, data_u)


def test_with_the_switch_off_a_batch_is_the_same_calls_keys_and_bits():
    """A set that holds its curvature, the same set without it and a set without faces: the same C-ABI calls in the same
    order, the same keys (but "ids", which a set with faces has always carried) and the same bits."""
    from geot_amd.openpoints.dataset import FixMatchBatcher, SupervisedBatcher, ValBatcher, VoteBatcher
    w = _world()
    idx = [0, 1]
    sel = _sel([len(w["scans"][i]) for i in idx], 9)
    for make in (SupervisedBatcher, ValBatcher, VoteBatcher):
        runs = []
        for dset in (w["lab"], w["plain"], w["bare"]):
            _seed(6)
            runs.append(_traced(lambda: make(dset, N).batch(idx, sel=sel)))
        assert runs[0][0] == runs[1][0] == runs[2][0] and "geot_curvature_sample" not in runs[0][0]
        assert set(runs[0][1]) == set(runs[1][1]) == set(runs[2][1]) | ({"ids"} if make is not SupervisedBatcher else set())
        assert "curvatures" not in runs[0][1]
        for key, value in runs[2][1].items():
            if torch.is_tensor(value):
                assert torch.equal(runs[0][1][key], value) and torch.equal(runs[1][1][key], value), key
    _seed(6)
    a = _traced(lambda: FixMatchBatcher(w["lab"], w["unl"], N).batch([0], [1], sel_l=sel[:1], sel_u=sel[:1] % 144))
    _seed(6)
    b = _traced(lambda: FixMatchBatcher(w["bare"], w["bare"], N).batch([0], [1], sel_l=sel[:1], sel_u=sel[:1] % 144))
    assert a[0] == b[0] and [set(d) for d in a[1]] == [set(d) for d in b[1]] and "curvatures" not in a[1][1]


def test_every_refusal_comes_before_a_device_call():
    from geot_amd.openpoints.dataset import FixMatchBatcher, SupervisedBatcher, ValBatcher, VoteBatcher, mesh_curvature
    from geot_amd.openpoints.dataset.sample_draw import DeviceDraws
    w = _world()
    for make in (SupervisedBatcher, ValBatcher, VoteBatcher):
        for dset, idx, msg in ((w["plain"], [0], r"call scans.compute_curvature\(\) first"), (w["bare"], [0], "compute_curvature"),
                               (w["half"], [0, 1], r"batch slot 1 \(scan 1\) has no mesh")):
            batcher = make(dset, N, curvatures=True, draws=DeviceDraws(3))          # a device draw would be the first launch
            _refused(lambda: batcher.batch(idx), msg)
            if make is not SupervisedBatcher:
                _refused(lambda: batcher.cover(idx), msg)
        assert make(w["half"], N, curvatures=True).batch([0, 0])["curvatures"].shape == (2, N)     # the scan WITH a mesh serves
    both = FixMatchBatcher(w["lab"], w["plain"], N, curvatures=True, draws=DeviceDraws(3))         # one side without: dropped
    assert both.scans.curvature is None
    _refused(lambda: both.batch([0], [0]), r"call scans.compute_curvature\(\) first")
    for bad in (0, -1.0, float("nan"), float("inf"), None, "0.1"):
        _refused(lambda: w["plain"].compute_curvature(bad), "radius must be a finite positive number")
        _refused(lambda: mesh_curvature(w["plain"], bad), "radius must be a finite positive number")
    _refused(lambda: w["bare"].compute_curvature(), "the scan set holds no faces")
    _refused(lambda: mesh_curvature(w["bare"]), "the scan set holds no faces")
    assert w["plain"].curvature is None
    # check=True: an index outside its scan is an IndexError, with the switch on as with it off
    sel = _sel([525], 2)
    sel[0, 9] = 525
    with pytest.raises(IndexError, match="batch slot 0"):
        ValBatcher(w["lab"], N, curvatures=True).batch([0], sel=sel, check=True)
    got = ValBatcher(w["lab"], N, curvatures=True).batch([0], sel=sel)["curvatures"].cpu().numpy()
    assert got[0, 9] == 0 and np.array_equal(np.delete(got[0], 9), w["want"][0][np.delete(sel[0], 9)])
