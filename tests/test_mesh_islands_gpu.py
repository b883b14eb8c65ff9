"""Scan meshes through the Python surface (geot_amd/validation.py): DeviceScanSet(faces=), mesh_neighbours, mesh= on
scan_components and clean_scans, islands={"mesh": ...} on predict_scans and validate_scans, and the set's table cache
(keep_tables) for both kinds of table.  The scans: two sheets closer to each other than a mesh edge is long (tests/_mesh_ref.py
two_sheets; tests/test_mesh_neighbours_cpu.py shows the property on the restatements alone) and a plain grid; the model is the
tiny one of the decode tests.  Everything is compared with array_equal / torch.equal against the numpy restatements."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_ref as mref  # noqa: E402
import _scan_decode_ref as dref  # noqa: E402
import _scan_islands_ref as iref  # noqa: E402
import _seg_metrics_ref as sref  # noqa: E402
from _seg_metrics_ref import quiet  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N = dref.N_SAMPLE
G = 40                                  # two sheets of 40 x 40: one scan of 3 200 vertices
R2 = 30                                 # the second scan: a 30 x 30 grid
IDS = [0, 1]
KEEP = 0x1fffe                          # keep_largest=True at 17 classes
_cache = {}


def _world():
    if not _cache:
        from geot_amd.openpoints.dataset import DeviceScanSet
        from geot_amd.openpoints.models.segmentation import WholePartSeg
        pts, faces = mref.two_sheets(G, 0.25)
        labels = np.concatenate([np.full(G * G, 1), np.full(G * G, 2)]).astype(np.int32)
        patch = G * G + np.array([y * G + x for y in range(10, 15) for x in range(20, 25)])       # 25 vertices on the second sheet
        labels[patch] = 1
        pts2, faces2 = mref.grid_points(R2, R2) * np.float32(0.5), mref.grid(R2, R2)
        labels2 = (np.arange(R2 * R2) % R2 // 8).astype(np.int32)
        scans, labs, meshes = [pts, pts2], [labels, labels2], [mref.shuffled(faces, 1, corners=True), faces2]
        _cache.update(pts=scans, labels=labs, faces=meshes, patch=patch,
                      dset=DeviceScanSet(scans, labs, cls=[0, 1], device=DEV, faces=meshes),
                      bare=DeviceScanSet(scans, labs, cls=[0, 1], device=DEV),
                      model=WholePartSeg(segmentor_args=dref.tiny_model().to(DEV)).eval(),
                      cfg=type("Cfg", (), {"num_classes": 17, "num_points": N, "epoch": 1, "epochs": 2})(),
                      tables=[mref.mesh_table(f, len(p), 16) for f, p in zip(meshes, scans)])
    return _cache


def _seed():
    np.random.seed(2)
    random.seed(2)
    torch.manual_seed(2)


def _batcher(dset):
    from geot_amd.openpoints.dataset import ValBatcher
    from geot_amd.openpoints.dataset.sample_draw import DeviceDraws
    return ValBatcher(dset, N, draws=DeviceDraws(5))             # the same counter: the same batches


def _traced(fn):
    from geot_amd.ext import _common
    seen = []
    _common.trace = lambda launch, name: (seen.append(name), launch())[1]
    try:
        out = fn()
    finally:
        _common.trace = None
    return seen, out


def _preds(w, ids=IDS):
    return [torch.from_numpy(w["labels"][i].astype(np.int64)).to(DEV).view(1, -1) for i in ids]


def test_the_set_holds_the_faces_and_the_batch_its_scan_numbers():
    from geot_amd.openpoints.dataset import DeviceScanSet
    w = _world()
    dset = w["dset"]
    assert dset.faces.dtype == torch.int32 and dset.faces.is_cuda and tuple(dset.faces.shape) == (sum(len(f) for f in w["faces"]), 3)
    assert dset.face_sizes == [len(f) for f in w["faces"]] and dset.has_mesh == [True, True]
    assert dset.face_offsets.dtype == torch.int64 and dset.face_offsets.cpu().tolist() == [0, len(w["faces"][0]), sum(dset.face_sizes)]
    assert np.array_equal(dset.faces.cpu().numpy(), np.concatenate(w["faces"]))
    bare = w["bare"]
    assert bare.faces is None and bare.face_offsets is None and bare.face_sizes is None and bare.has_mesh is None
    # None: no mesh; (0, 3): a mesh with no faces; an index that does not fit int32 stays outside every scan
    part = DeviceScanSet(w["pts"], w["labels"], device=DEV, faces=[None, np.zeros((0, 3), dtype=np.int64)])
    assert part.face_sizes == [0, 0] and part.has_mesh == [False, True] and tuple(part.faces.shape) == (0, 3)
    wide = DeviceScanSet(w["pts"][1:], w["labels"][1:], device=DEV, faces=[np.array([[0, 1, 2 ** 40], [-2 ** 40, 1, 2]])])
    assert wide.faces.cpu().tolist() == [[0, 1, 2 ** 31 - 1], [-1, 1, 2]]
    # _merged: the side without faces counts as mesh-less
    both = DeviceScanSet._merged(bare, dset)
    assert both.face_sizes == [0, 0] + dset.face_sizes and both.has_mesh == [False, False, True, True]
    assert both.face_offsets.cpu().tolist() == [0, 0, 0] + dset.face_offsets.cpu().tolist()[1:] and torch.equal(both.faces, dset.faces)
    assert DeviceScanSet._merged(bare, bare).faces is None
    batch = _batcher(dset).batch([1, 0])
    assert batch["ids"] == [1, 0] and batch["scan_ids"].cpu().tolist() == [1, 0]
    # a set without faces and with the cache off keeps the batch's key set; with the cache on the ids are there
    plain = DeviceScanSet(w["pts"], w["labels"], device=DEV)
    assert set(batch) - set(_batcher(plain).batch([1, 0])) == {"ids"}
    assert _batcher(plain.keep_tables()).batch([1, 0])["ids"] == [1, 0]


def test_mesh_neighbours_is_the_restatement_slot_after_slot():
    from geot_amd.validation import mesh_neighbours
    w = _world()
    for ids in ([0, 1], [1, 0, 1]):
        batch = _batcher(w["dset"]).batch(ids)
        launches, (table, stats) = _traced(lambda: mesh_neighbours(batch, stats=True))
        assert launches == ["geot_mesh_neighbours"]
        assert table.dtype == torch.int32 and tuple(table.shape) == (sum(batch["sizes"]), 16) and tuple(stats.shape) == (len(ids), 4)
        assert np.array_equal(table.cpu().numpy(), np.concatenate([w["tables"][i][0] for i in ids]))
        assert stats.cpu().tolist() == [w["tables"][i][1] for i in ids]
    narrow = mesh_neighbours(batch, k=4)
    assert np.array_equal(narrow.cpu().numpy(), np.concatenate([mref.mesh_table(w["faces"][i], len(w["pts"][i]), 4)[0] for i in ids]))


def test_two_sheets_are_two_pieces_over_the_mesh_and_one_by_distance():
    from geot_amd.validation import scan_components, scan_neighbours
    w = _world()
    batch = _batcher(w["dset"]).batch([0])
    ones = [torch.ones(1, 2 * G * G, dtype=torch.int64, device=DEV)]
    knn = scan_neighbours(batch, k=8)
    by_distance = scan_components(ones, batch, num_classes=17)
    over_mesh, stats = scan_components(ones, batch, num_classes=17, mesh=True, stats=True)
    labels = np.ones(2 * G * G, dtype=np.int64)
    assert np.array_equal(by_distance[0].cpu().numpy().reshape(-1), iref.components(labels, knn.cpu().numpy(), 17))
    assert np.array_equal(over_mesh[0].cpu().numpy().reshape(-1), iref.components(labels, w["tables"][0][0], 17))
    assert (by_distance[0] == 0).all()                                                   # ONE piece
    assert stats[0, 0] == 2 and sorted(set(over_mesh[0].cpu().numpy().reshape(-1).tolist())) == [0, G * G]      # TWO
    assert (over_mesh[0][0, :G * G] == 0).all() and (over_mesh[0][0, G * G:] == G * G).all()
    # an int is the width; the width of the kNN table (k) is ignored with mesh set
    same = scan_components(ones, batch, num_classes=17, mesh=16, k=3)
    assert torch.equal(same[0], over_mesh[0])


def test_clean_scans_over_the_mesh_relabels_the_patch_the_knn_table_keeps():
    from geot_amd.validation import clean_scans, scan_neighbours
    w = _world()
    batch = _batcher(w["dset"]).batch(IDS)
    knn = [t.cpu().numpy() for t in torch.split(scan_neighbours(batch, k=8), batch["sizes"])]
    kept, kept_stats = clean_scans(_preds(w), batch, keep_largest=True, num_classes=17, stats=True)
    moved, moved_stats = clean_scans(_preds(w), batch, keep_largest=True, num_classes=17, stats=True, mesh=True)
    for s in IDS:
        labels = w["labels"][s].astype(np.int64)
        want, _, st = iref.scan_islands_slot(labels, knn[s], 17, 10, keep=KEEP)
        assert np.array_equal(kept[s].cpu().numpy().reshape(-1), want) and kept_stats[s].cpu().tolist() == st
        want, _, st = iref.scan_islands_slot(labels, w["tables"][s][0], 17, 10, keep=KEEP)
        assert np.array_equal(moved[s].cpu().numpy().reshape(-1), want) and moved_stats[s].cpu().tolist() == st
    patch = w["patch"]
    assert (kept[0][0, patch] == 1).all()            # by distance the patch touches tooth 1 on the other sheet: one piece with it
    assert (moved[0][0, patch] == 2).all()           # over the surface it is a stray piece of class 1 inside tooth 2
    assert moved_stats[0].cpu().tolist() == [3, 1, 25, 0] and kept_stats[0].cpu().tolist() == [2, 0, 0, 0]


def test_islands_mesh_through_predict_scans_and_validate_scans():
    from geot_amd import validation as V
    w = _world()
    batch = _batcher(w["dset"]).batch(IDS)
    logits = torch.randn(2, 17, N, generator=torch.Generator().manual_seed(3)).to(DEV)
    plain = V.predict_scans(logits, batch)
    want = V.clean_scans([p.clone() for p in plain], batch, num_classes=17, mesh=True)
    launches, got = _traced(lambda: V.predict_scans(logits, batch, islands={"mesh": True}))
    assert all(torch.equal(g, w_) for g, w_ in zip(got, want)) and not all(torch.equal(g, p) for g, p in zip(got, plain))
    assert launches.count("geot_mesh_neighbours") == 1 and "geot_knn_sorted_ws" not in launches
    by_distance = V.predict_scans(logits, batch, islands=True)
    print("cleaned over the mesh / by distance: %d / %d of %d labels changed, %d differ" % (
        sum(int((g != p).sum()) for g, p in zip(got, plain)), sum(int((g != p).sum()) for g, p in zip(by_distance, plain)),
        sum(batch["sizes"]), sum(int((g != p).sum()) for g, p in zip(got, by_distance))))
    # the validator: the model's own labels, cleaned over the 16-wide mesh table and counted
    _seed()
    with quiet(), torch.no_grad():
        data = _batcher(w["dset"]).batch(IDS)
        labels = V.predict_scans(w["model"](data)[0], data)
        cleaned = V.clean_scans([p.clone() for p in labels], data, num_classes=17, mesh=16)
        metrics = V.SegMetrics(17, DEV)
        metrics.update(cleaned, V._scan_labels(data), [0 if m else 1 for m in data["mandible"]])
        out = metrics.read()
        _seed()
        launches, scored = _traced(lambda: V.validate_scans(w["model"], _batcher(w["dset"]), w["cfg"], islands={"mesh": 16}))
        _seed()
        off, _ = _traced(lambda: V.validate_scans(w["model"], _batcher(w["dset"]), w["cfg"]))
        _seed()
        by_distance, _ = _traced(lambda: V.validate_scans(w["model"], _batcher(w["dset"]), w["cfg"], islands=True))
    triple = (out["whole_macc"], out["whole_miou"], out["whole_mdsc"])
    assert len(scored) == 3 and all(sref.same_value(a, b) for a, b in zip(scored, triple))
    # no search for the table (the model's own searches remain): one geot_mesh_neighbours call in place of one search per scan
    searches = [run.count("geot_knn_sorted_ws") for run in (off, launches, by_distance)]
    assert launches.count("geot_mesh_neighbours") == 1 and searches[1] == searches[0] and searches[2] == searches[0] + 2
    assert "geot_mesh_neighbours" not in off + by_distance
    assert launches.index("geot_mesh_neighbours") < launches.index("geot_scan_islands") < launches.index("geot_seg_confusion")


def test_the_table_cache_builds_once_and_gives_the_same_bits():
    from geot_amd import validation as V
    from geot_amd.openpoints.dataset import DeviceScanSet
    w = _world()
    dset = DeviceScanSet(w["pts"], w["labels"], cls=[0, 1], device=DEV, faces=w["faces"])        # a set of its own: the switch is the set's
    batch = _batcher(dset).batch(IDS)
    clean = lambda **kw: V.clean_scans(_preds(w), batch, num_classes=17, stats=True, **kw)      # noqa: E731
    off_launches, off = _traced(lambda: clean(mesh=True))
    knn_launches, knn_off = _traced(lambda: clean())
    table_off, stats_off = V.mesh_neighbours(batch, stats=True)
    search_off = V.scan_neighbours(batch, k=8)
    assert dset._tables == {} and dset.keep_tables() is dset
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and torch.equal(a[1], b[1])       # noqa: E731
    first_launches, first = _traced(lambda: clean(mesh=True))
    second_launches, second = _traced(lambda: clean(mesh=True))
    assert first_launches == off_launches and first_launches.count("geot_mesh_neighbours") == 1
    assert second_launches == ["geot_scan_islands"] and same(first, off) and same(second, off)
    assert sorted(dset._tables) == [(0, "mesh", 16), (1, "mesh", 16)]
    table_on, stats_on = V.mesh_neighbours(batch, stats=True)
    assert torch.equal(table_on, table_off) and torch.equal(stats_on, stats_off)
    # the same bits on another stream, which waits for the event of the stream that built the tables; nothing is built
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        side_launches, third = _traced(lambda: clean(mesh=True))
    side.synchronize()
    assert side_launches == ["geot_scan_islands"] and same(third, off)
    # the kNN kind: built once per scan and width, equal to the uncached search; another width is another table
    launches, search_on = _traced(lambda: V.scan_neighbours(batch, k=8))
    assert launches.count("geot_knn_sorted_ws") == 2 and torch.equal(search_on, search_off)
    launches, again = _traced(lambda: V.scan_neighbours(batch, k=8))
    assert launches == [] and torch.equal(again, search_off)
    launches, cached = _traced(lambda: clean())
    assert launches == ["geot_scan_islands"] and same(cached, knn_off) and knn_launches.count("geot_knn_sorted_ws") == 2
    launches, _ = _traced(lambda: V.scan_neighbours(batch, k=5))
    assert launches.count("geot_knn_sorted_ws") == 2 and (0, "knn", 6) in dset._tables and (0, "knn", 9) in dset._tables
    # only what is missing is built: scan 1 is kept, scan 0 is not
    dset.drop_tables()
    assert dset._tables == {}
    V.mesh_neighbours(_batcher(dset).batch([1]))
    three = _batcher(dset).batch([1, 0, 1])
    launches, (table, stats) = _traced(lambda: V.mesh_neighbours(three, stats=True))
    assert launches == ["geot_mesh_neighbours"] and sorted(dset._tables) == [(0, "mesh", 16), (1, "mesh", 16)]
    assert np.array_equal(table.cpu().numpy(), np.concatenate([w["tables"][i][0] for i in (1, 0, 1)]))
    assert stats.cpu().tolist() == [w["tables"][i][1] for i in (1, 0, 1)]
    # drop_tables() rebuilds; switching off drops and builds every time; a batch without the host ids is never cached
    dset.drop_tables()
    launches, rebuilt = _traced(lambda: clean(mesh=True))
    assert launches == off_launches and same(rebuilt, off)
    dset.keep_tables(False)
    assert dset._tables == {}
    launches, _ = _traced(lambda: clean(mesh=True))
    assert launches == off_launches and dset._tables == {}
    dset.keep_tables()
    anonymous = {key: value for key, value in batch.items() if key != "ids"}
    launches, search = _traced(lambda: V.scan_neighbours(anonymous, k=8))
    assert launches.count("geot_knn_sorted_ws") == 2 and dset._tables == {} and torch.equal(search, search_off)


def test_with_the_feature_unused_nothing_changes():
    """faces given or not, mesh unset, the cache off: clean_scans and validate_scans(islands=True) make the same sequence of
    C-ABI calls as on a set without faces and give the same labels and counts."""
    from geot_amd import validation as V
    w = _world()
    runs = []
    for dset in (w["bare"], w["dset"]):
        batch = _batcher(dset).batch(IDS)
        clean_launches, (labels, stats) = _traced(lambda: V.clean_scans(_preds(w), batch, num_classes=17, stats=True))
        _seed()
        with quiet():
            val_launches, scored = _traced(lambda: V.validate_scans(w["model"], _batcher(dset), w["cfg"], islands=True))
        runs.append((clean_launches, labels, stats, val_launches, scored))
    bare, held = runs
    assert bare[0] == held[0] and bare[3] == held[3] and "geot_mesh_neighbours" not in held[0] + held[3]
    assert all(torch.equal(a, b) for a, b in zip(bare[1], held[1])) and torch.equal(bare[2], held[2])
    assert all(sref.same_value(a, b) for a, b in zip(bare[4], held[4]))
    assert w["dset"]._tables == {} and w["bare"]._tables == {}


def _refused(call, match):
    """The C-ABI calls made by a call that must raise ValueError."""
    from geot_amd.ext import _common
    seen = []
    _common.trace = lambda launch, name: (seen.append(name), launch())[1]
    try:
        with pytest.raises(ValueError, match=match):
            call()
    finally:
        _common.trace = None
    return seen


def test_a_set_or_a_scan_without_faces_is_refused_before_any_device_call():
    from geot_amd import validation as V
    from geot_amd.openpoints.dataset import DeviceScanSet
    w = _world()
    bare_batcher = _batcher(w["bare"])
    batch = bare_batcher.batch(IDS)
    logits = torch.zeros(2, 17, N, device=DEV)
    preds = _preds(w)
    for call in (lambda: V.mesh_neighbours(batch), lambda: V.clean_scans(preds, batch, mesh=True),
                 lambda: V.scan_components(preds, batch, mesh=8), lambda: V.predict_scans(logits, batch, islands={"mesh": True}),
                 lambda: V.validate_scans(w["model"], bare_batcher, w["cfg"], islands={"mesh": True}),
                 lambda: V.validate_scans_voted(w["model"], w["bare"], w["cfg"], num_votes=2, islands={"mesh": True}),
                 lambda: V.validate_scans_covered(w["model"], bare_batcher, w["cfg"], islands={"mesh": True}),
                 lambda: V.validate_scans_decoded(w["model"], bare_batcher, w["cfg"], islands={"mesh": 4}),
                 lambda: V.cover_scans(w["model"], bare_batcher, IDS, islands={"mesh": True}),
                 lambda: V.decode_scans(w["model"], bare_batcher, IDS, islands={"mesh": True})):
        assert _refused(call, "the scan set holds no faces") == []
    # a scan without a mesh in a set that has faces: the slot and the scan are named; the scan that has one is served
    half = DeviceScanSet(w["pts"], w["labels"], cls=[0, 1], device=DEV, faces=[w["faces"][0], None])
    mixed, turned, alone = (_batcher(half).batch(ids) for ids in ([0, 1], [1, 0], [0]))
    assert _refused(lambda: V.mesh_neighbours(mixed), r"batch slot 1 \(scan 1\) has no mesh") == []
    assert _refused(lambda: V.clean_scans(_preds(w, [1, 0]), turned, mesh=True), r"batch slot 0 \(scan 1\) has no mesh") == []
    launches, own = _traced(lambda: V.mesh_neighbours(alone))
    assert launches == ["geot_mesh_neighbours"] and np.array_equal(own.cpu().numpy(), w["tables"][0][0])
