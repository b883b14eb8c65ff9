"""geot_tooth_moments on the GPU against its numpy int64 restatement (tests/_tooth_scores_ref.py moments_ref), array_equal
throughout, in both GEOT_TOOTH_MOMENTS_IMPL forms and for c in {1, 2, 17, 32}.  The set holds scans of 1, 67 and 4099 vertices
(a record shorter than a wave, a remainder record, several records per slot), one of 300 vertices of a single class (the
wave-uniform path under maximal contention) and one of 64 vertices whose classes cycle (no two neighbouring lanes agree);
classes absent on one side only; predictions of -1, c and 2^40; labels outside [0, c); positions that are NaN, +-Inf, just below
and at 16384 from the centre; d * 65536 exactly on .5 on both signs; one scan in two slots; an out-of-range scan id and bad work
records; the work table split over two calls; the same call twice; b = 0 and n_work = 0; every refusal with the rows untouched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tooth_scores_ref as tref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = [1, 67, 4099, 300, 64]
CLASSES = [1, 2, 17, 32]
IMPLS = ["combined", "basic"]
_cache = {}


def _runs(rng, m, c, mean=90):
    """Spatially coherent classes: runs of one class, about `mean` vertices long."""
    out = np.empty(m, np.int64)
    at = 0
    while at < m:
        n = int(rng.integers(1, 2 * mean))
        out[at:at + n] = rng.integers(0, c)
        at += n
    return out


def _world(c):
    """The scan set for c classes, on the host and on the device; made once per c."""
    if c in _cache:
        return _cache[c]
    rng = np.random.default_rng(100 + c)
    offsets = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    total = int(offsets[-1])
    points = (rng.normal(size=(total, 3)) * [9.0, 6.0, 4.0] + [14.0, -37.0, 61.0]).astype(np.float32)
    labels = np.concatenate([_runs(rng, m, c, max(4, m // 40)) for m in SIZES])
    labels[offsets[1]:offsets[1] + 20] = min(1, c - 1)      # class 1 is a label of the second scan
    big = slice(int(offsets[2]), int(offsets[3]))
    if c >= 3:
        labels[big][labels[big] == c - 1] = 0               # class c - 1 is never a label of the large scan
    labels[offsets[3]:offsets[4]] = min(3, c - 1)           # the scan of one class
    labels[offsets[4]:offsets[5]] = np.arange(64) % c       # the scan whose classes cycle
    labels[offsets[2] + 5] = -1                             # labels outside [0, c)
    labels[offsets[2] + 700] = c
    labels[offsets[1] + 9] = c + 5
    w = dict(c=c, total=total, offsets=offsets, points=points, labels=labels.astype(np.int32), rng=rng)
    w["d_points"], w["d_labels"] = torch.from_numpy(points).to(DEV), torch.from_numpy(w["labels"]).to(DEV)
    w["d_offsets"] = torch.from_numpy(offsets).to(DEV)
    _cache[c] = w
    return w


def _preds(w, scan_ids, seed=0):
    """Per-vertex predictions for the slots, slot after slot: the labels with a fifth redrawn, then the special values."""
    rng = np.random.default_rng(seed)
    c, parts = w["c"], []
    for sid in scan_ids:
        lab = w["labels"][w["offsets"][sid]:w["offsets"][sid + 1]].astype(np.int64).copy()
        flip = rng.random(len(lab)) < 0.2
        lab[flip] = rng.integers(0, c, size=int(flip.sum()))
        lab[lab < 0] = 0
        lab[lab >= c] = 0
        if sid == 1 and c >= 2:
            lab[lab == 1] = 0                               # class 1 is a label of this scan and never a prediction
        if sid == 3:
            lab[:] = min(3, c - 1)
        if sid == 4:
            lab[:] = (np.arange(64) + (seed % 2)) % c
        if len(lab) > 40:
            lab[[11, 23, 37]] = [-1, c, 1 << 40]
        parts.append(lab)
    return parts


def _launch(w, b, scan_ids, center, work, pred, out_offsets, rows):
    """One call; every argument a host array (rows: the device tensor that is added into)."""
    from geot_amd.ext._common import call, ptr
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
    keep = [dev(scan_ids, np.int64), dev(center, np.float32), dev(np.asarray(work).reshape(-1, 4), np.int32), dev(out_offsets, np.int64),
            dev(pred, np.int64)]
    call("geot_tooth_moments", DEV, b, w["c"], len(SIZES), w["total"], ptr(w["d_points"]), ptr(w["d_labels"]), ptr(w["d_offsets"]),
         ptr(keep[0]), ptr(keep[1]), int(keep[2].shape[0]), ptr(keep[2]), ptr(keep[3]), ptr(keep[4]), ptr(rows))
    torch.cuda.synchronize()
    return rows.cpu().numpy()


def _case(w, scan_ids, center=None, seed=0, chunk=64):
    from geot_amd.validation import scan_work_table
    b = len(scan_ids)
    sizes = [SIZES[s] for s in scan_ids]
    preds = _preds(w, scan_ids, seed)
    out_offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    if center is None:
        center = np.stack([w["points"][w["offsets"][s]:w["offsets"][s + 1]].mean(0) for s in scan_ids]).astype(np.float32)
    return dict(b=b, scan_ids=np.asarray(scan_ids, np.int64), center=center, work=scan_work_table(sizes, min_chunk=chunk),
                pred=np.concatenate(preds), out_offsets=out_offsets)


def _want(w, k, rows=None):
    return tref.moments_ref(k["b"], w["c"], w["points"], w["labels"], w["offsets"], k["scan_ids"], k["center"], k["work"],
                            k["out_offsets"], k["pred"], rows)


def _got(w, k, rows=None, work=None):
    rows = torch.zeros((max(k["b"], 1), tref.ENTRIES * w["c"] + 2), dtype=torch.int64, device=DEV) if rows is None else rows
    return _launch(w, k["b"], k["scan_ids"], k["center"], k["work"] if work is None else work, k["pred"], k["out_offsets"], rows)


@pytest.fixture(params=IMPLS)
def impl(request, monkeypatch):
    if request.param == "basic":
        monkeypatch.setenv("GEOT_TOOTH_MOMENTS_IMPL", "basic")
    else:
        monkeypatch.delenv("GEOT_TOOTH_MOMENTS_IMPL", raising=False)
    return request.param


@pytest.mark.parametrize("c", CLASSES)
def test_ragged_scans_every_record_shape(c, impl):
    """b = 3 scans of 1, 67 and 4099 vertices, records of 64 (one wave works, three idle) and of 256 vertices."""
    w = _world(c)
    for chunk in (64, 256):
        k = _case(w, [0, 1, 2], chunk=chunk)
        counts = np.bincount(k["work"][:, 0], minlength=3)
        assert counts[0] == 1 and counts[1] == (2 if chunk == 64 else 1) and counts[2] > 4
        want = _want(w, k)
        assert np.array_equal(_got(w, k), want)
        m = want[2][:tref.ENTRIES * c].reshape(c, tref.ENTRIES)
        if c >= 3:
            assert m[c - 1, 0] == 0 and m[c - 1, 10] > 0                  # absent on the label side only
        if c >= 2:
            m1 = want[1][:tref.ENTRIES * c].reshape(c, tref.ENTRIES)
            assert m1[1, 0] > 0 and m1[1, 10] == 0                        # absent on the prediction side only
        assert want[2][-1] == 0 and want[:, :-2].any()


@pytest.mark.parametrize("c", CLASSES)
def test_one_class_only_and_cycling_classes(c, impl):
    w = _world(c)
    k = _case(w, [3, 4, 4], seed=1)                                       # the cycling scan twice: predictions shifted by one
    want = _want(w, k)
    assert np.array_equal(_got(w, k), want)
    only = min(3, c - 1)                                                  # (three of its predictions are -1, c and 2^40)
    assert want[0][tref.ENTRIES * only] == 300 and want[0][tref.ENTRIES * only + 10] == 297 == want[0][tref.ENTRIES * only + 20]
    if c == 32:
        assert (want[1][:tref.ENTRIES * c].reshape(c, tref.ENTRIES)[:, 0] == 2).all()      # 64 lanes, 32 classes, none adjacent


def test_one_scan_in_two_slots_and_special_positions(impl):
    """Slots 0 and 2 are the same scan under different centres and predictions; slot 1's scan carries the special positions."""
    c = 17
    base = _world(c)
    w = dict(base)
    points = base["points"].copy()
    lo = int(base["offsets"][1])
    center = np.array([[14.0, -37.0, 61.0], [1.0, -2.0, 0.0], [0.0, 0.0, 0.0]], np.float32)
    f = np.float32
    points[lo + 0] = [np.nan, 0, 0]
    points[lo + 1] = [1, np.inf, 0]
    points[lo + 2] = [1, -2, -np.inf]
    points[lo + 3] = [1, -2, np.nextafter(f(16384), f(0))]                # just below the limit: usable
    points[lo + 4] = [1, -2, 16384]                                       # at the limit: not
    points[lo + 5] = [1, -2, -np.nextafter(f(16384), f(0))]
    points[lo + 6] = [1, -2, -16384]
    points[lo + 7] = [16385, -2, 0]                                       # d = 16384 after the subtraction
    for i, half in enumerate((0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 1023.5, -1023.5)):      # d * 65536 on .5: ties to even
        points[lo + 10 + i] = [1 + half / 65536, -2 + half / 65536, half / 65536]
    w["points"], w["d_points"] = points, torch.from_numpy(points).to(DEV)
    usable, q = tref.quantise(points[lo:lo + 18], center[1])
    assert usable.tolist() == [False] * 3 + [True, False, True, False, False] + [True] * 10
    assert q[10:18, 0].tolist() == [0, 2, 2, 0, -2, -2, 1024, -1024] and q[10:18, 1].tolist() == q[10:18, 2].tolist() == q[10:18, 0].tolist()
    assert q[3, 2] == (1 << 30) - 64 and q[5, 2] == -((1 << 30) - 64)
    k = _case(w, [2, 1, 2], center=center, seed=3)
    k["pred"][SIZES[2] + SIZES[1]:] = np.roll(k["pred"][:SIZES[2]], 17)   # the second copy of the scan: other predictions
    want = _want(w, k)
    got = _got(w, k)
    assert np.array_equal(got, want)
    assert want[1][-1] == 6 and want[0][-1] == 0 and not np.array_equal(want[0], want[2])
    label_side = [tref.ENTRIES * j + e for j in range(c) for e in range(1)]
    assert np.array_equal(want[0][label_side], want[2][label_side])       # the same scan: the same label counts


def test_skipped_slots_and_records_leave_their_rows_zero(impl):
    w = _world(17)
    k = _case(w, [2, 1, 0])
    k["scan_ids"] = np.array([2, 99, -1], np.int64)                       # slots 1 and 2 name no scan
    bad = np.array([[-1, 0, 64, 0], [3, 0, 64, 0], [0, SIZES[2], 64, 0], [0, -1, 64, 0], [0, 0, 0, 0], [0, 128, -5, 0]], np.int32)
    work = np.concatenate([bad[:3], k["work"], bad[3:]])
    want = _want(w, dict(k, work=work))
    got = _got(w, k, work=work)
    assert np.array_equal(got, want) and not got[1:].any() and got[0].any()
    assert np.array_equal(want, _want(w, k))                              # the bad records add nothing
    # a record that runs past the end of its scan is cut there
    over = np.array([[0, SIZES[2] - 10, 1 << 30, 0]], np.int32)
    assert np.array_equal(_got(w, k, work=over), _want(w, dict(k, work=over)))


@pytest.mark.parametrize("c", [2, 17])
def test_split_tables_repeats_and_nothing_to_do(c, impl):
    w = _world(c)
    k = _case(w, [1, 2, 4], chunk=256)
    want = _want(w, k)
    words = tref.ENTRIES * c + 2
    rows = torch.zeros((3, words), dtype=torch.int64, device=DEV)
    half = len(k["work"]) // 2
    _got(w, k, rows=rows, work=k["work"][half:])                          # the second half first
    assert np.array_equal(_got(w, k, rows=rows, work=k["work"][:half]), want)
    assert np.array_equal(_got(w, k), want) and np.array_equal(_got(w, k), want)       # the same call twice, the same bits
    sentinel = torch.full((3, words), 7, dtype=torch.int64, device=DEV)
    assert (_got(w, dict(k, b=0), rows=sentinel) == 7).all()
    assert (_got(w, k, rows=sentinel, work=np.zeros((0, 4), np.int32)) == 7).all()


def test_refusals_leave_the_rows_untouched():
    from geot_amd import _lib
    from geot_amd.ext._common import ptr
    w = _world(17)
    k = _case(w, [1, 2])
    lib = _lib.load()
    rows = torch.full((2, tref.ENTRIES * 17 + 2), 7, dtype=torch.int64, device=DEV)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
    keep = dict(scan_ids=t(k["scan_ids"], np.int64), center=t(k["center"], np.float32), work=t(k["work"], np.int32),
                out_offsets=t(k["out_offsets"], np.int64), pred=t(k["pred"], np.int64))
    good = dict(b=2, c=17, n_scans=len(SIZES), total=w["total"], points=ptr(w["d_points"]), labels=ptr(w["d_labels"]),
                offsets=ptr(w["d_offsets"]), scan_ids=ptr(keep["scan_ids"]), center=ptr(keep["center"]), n_work=len(k["work"]),
                work=ptr(keep["work"]), out_offsets=ptr(keep["out_offsets"]), pred=ptr(keep["pred"]), moments=ptr(rows), stream=None)
    bad = [dict(b=-1), dict(b=65536), dict(c=0), dict(c=33), dict(n_scans=0), dict(total=0), dict(n_work=-1), dict(work=None),
           dict(work=good["work"] + 4)] + [{name: None} for name in ("points", "labels", "offsets", "scan_ids", "center", "out_offsets", "pred")]
    for over in bad:
        assert lib.geot_tooth_moments(*dict(good, **over).values()) == 1, over
    assert lib.geot_tooth_moments(*dict(good, moments=None).values()) == 1
    torch.cuda.synchronize()
    assert (rows == 7).all()


def test_tooth_scores_and_instances_from_a_batch():
    """ToothScores.update / read and tooth_instances on a ValBatcher batch: the rows are the restatement's, the scores the fp64
    computation's within its bound, the instances the predicted vertices' own centroids and boxes."""
    from geot_amd.openpoints.dataset import DeviceScanSet, ValBatcher
    from geot_amd.validation import TOOTH_CHUNK_MIN, ToothScores, scan_work_table, tooth_instances
    c = 17
    w = _world(c)
    ids = [2, 3]
    scans = [w["points"][w["offsets"][s]:w["offsets"][s + 1]] for s in range(len(SIZES))]
    labels = [np.clip(w["labels"][w["offsets"][s]:w["offsets"][s + 1]], 0, c - 1) for s in range(len(SIZES))]
    dset = DeviceScanSet(scans, labels, cls=[0, 1, 0, 1, 0], device=DEV)
    batch = ValBatcher(dset, 64).batch(ids)
    preds_np = [np.clip(p, 0, c - 1) for p in _preds(w, ids, seed=5)]
    flat = torch.from_numpy(np.concatenate(preds_np)).to(DEV)
    preds = [p.view(1, -1) for p in torch.split(flat, [SIZES[s] for s in ids])]
    teeth = ToothScores(c, DEV)
    teeth.update(preds, batch)                                            # warm: the kernel, the pinned pool
    tooth_instances(preds, batch, c)
    teeth.reset()
    torch.cuda.synchronize()
    from geot_amd.ext import _common
    seen = []
    torch.cuda.set_sync_debug_mode("error")                               # update() and tooth_instances() must not synchronise
    _common.trace = lambda launch, name: (seen.append(name), launch())[1]
    try:
        for _ in range(5):                                                # ten scans: the buffers grow past their first eight rows
            teeth.update(preds, batch)
        geo = tooth_instances(preds, batch, c)
    finally:
        _common.trace = None
        torch.cuda.set_sync_debug_mode(0)
    assert seen == ["geot_tooth_moments"] * 6                             # one launch per call, whatever the batch holds
    assert teeth.scans == 10 and teeth.moments.shape[0] >= 10
    center = batch["center"].cpu().numpy()
    sizes = [SIZES[s] for s in ids]
    want = tref.moments_ref(2, c, np.concatenate([scans[s] for s in ids]), np.concatenate([labels[s] for s in ids]).astype(np.int32),
                            np.array([0, sizes[0], sum(sizes)]), np.array([0, 1]), center, scan_work_table(sizes, min_chunk=TOOTH_CHUNK_MIN),
                            np.array([0, sizes[0]]), np.concatenate(preds_np))
    assert np.array_equal(teeth.moments[:10].cpu().numpy(), np.tile(want, (5, 1)))
    out = teeth.read()
    assert out["scans"] == 10 and out["unusable"] == 0 and len(out["tla_list"]) == 10
    for i, s in enumerate(ids):
        ref = tref.scores_fp64(scans[s], labels[s], preds_np[i], c)
        if ref["teeth"]:
            assert abs(out["tla_list"][i] - ref["tla"]) <= tref.tla_bound(scans[s], center[i], labels[s], c)
            assert out["tir_list"][i] == ref["tir"]
        assert out["tsa_list"][i] == ref["tsa"] and out["tsa_instance_list"][i] == ref["tsa_instance"]
    teeth.reset()
    assert teeth.scans == 0 and not teeth.moments.any()
    assert geo["count"].device == flat.device and geo["centroid"].dtype == torch.float64
    e = 2.0 ** -17 + np.spacing(np.float32(np.abs(np.concatenate([scans[s] for s in ids])).max()))
    for i, s in enumerate(ids):
        for j in range(c):
            mine = scans[s][preds_np[i] == j].astype(np.float64)
            assert int(geo["count"][i, j]) == len(mine)
            if len(mine):
                assert np.abs(geo["centroid"][i, j].cpu().numpy() - mine.mean(0)).max() <= e
                assert np.abs(geo["box_min"][i, j].cpu().numpy() - mine.min(0)).max() <= e
                assert np.abs(geo["box_max"][i, j].cpu().numpy() - mine.max(0)).max() <= e
            else:
                assert torch.isnan(geo["centroid"][i, j]).all() and torch.isnan(geo["box_min"][i, j]).all()
