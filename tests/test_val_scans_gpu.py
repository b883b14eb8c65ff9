"""Validating and predicting whole scans from a device-resident scan set (geot_amd/validation.py validate_scans,
SegMetrics.update_from_scans, predict_scans over csrc/scan_predict.hip; geot_amd/openpoints/dataset/val_batch.py).  Every
comparison of counts, predictions and metrics is exact (torch.equal, NaN matching NaN, dtypes): the new entry point against
the chain it replaces (geot_three_nn_ws per scan -> geot_seg_confusion_interp, and get_pred_whole + torch.bincount), the
batcher against prepare_sample + the weak view on each scan alone and against the reference-made fixture
(tests/golden/val_batches_ref.npz), validate_scans against the existing validate() fed the batcher's own batches."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _seg_metrics_ref as ref  # noqa: E402
from _seg_metrics_ref import quiet  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "val_batches_ref.npz")
CENTER, SCALE = np.array([14.0, -37.0, 61.0], np.float32), np.float32(31.5)


def _scan(m, index, c=17):
    """A scan in scan coordinates (millimetres, far from the origin) with coherent labels in [0, c)."""
    from geot_amd.synth import make_cloud, region_labels
    unit = make_cloud(m, index)[0]
    return (unit * np.float32(1.01) * SCALE + CENTER).astype(np.float32), (region_labels(unit) % c).astype(np.int32)


def _set(sizes, first_index, cls=None, c=17):
    from geot_amd.openpoints.dataset import DeviceScanSet
    data = [_scan(m, first_index + i, c) for i, m in enumerate(sizes)]
    return DeviceScanSet([p for p, _ in data], [lab for _, lab in data], cls=cls, device=DEV)


def _offsets(sizes):
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=DEV)


def _same(a, b):
    """torch.equal with NaN == NaN and the dtype included."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.nan_to_num(a, nan=-7.0) if a.is_floating_point() else a,
                                                                      torch.nan_to_num(b, nan=-7.0) if b.is_floating_point() else b)


# ------------------------------------------------------------------------------------------------ 1. kernel = chain
RAGGED = [1, 63, 64, 65, 100003, 5000, 777]
_ragged = {}


def _ragged_set():
    if "set" not in _ragged:
        _ragged["set"] = _set(RAGGED, 300)
    return _ragged["set"]


def _known_and_logits(b, n, c, seed):
    from geot_amd.synth import make_cloud
    rng = np.random.default_rng(seed)
    known = np.stack([(make_cloud(n, seed + 31 * s)[0] * SCALE + CENTER).astype(np.float32) for s in range(b)])
    logits = (rng.normal(size=(b, c, n)) * 3).astype(np.float32)
    return torch.from_numpy(known).to(DEV), torch.from_numpy(logits).to(DEV)


def _kernel(dset, ids, known, prob, c, counts=None, want_pred=False, with_labels=True):
    """geot_scan_predict through the C ABI: (pred per slot or None)."""
    from geot_amd import _lib
    from geot_amd.ext._common import call, ptr
    from geot_amd.validation import scan_work_table
    b, n = known.shape[0], known.shape[1]
    sizes = [dset.sizes[i] for i in ids]
    ids_dev = torch.tensor(ids, dtype=torch.int64, device=DEV)
    work = torch.from_numpy(scan_work_table(sizes)).to(DEV)
    pred = out_offs = None
    if want_pred:
        pred, out_offs = torch.full((sum(sizes),), -1, dtype=torch.int64, device=DEV), _offsets(sizes)
    nbytes = int(_lib.load().geot_scan_predict_ws_bytes(b, n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    call("geot_scan_predict", DEV, b, c, n, len(dset), int(dset.points.shape[0]), ptr(dset.points),
         ptr(dset.labels) if with_labels else None, ptr(dset.offsets), ptr(ids_dev), ptr(known), ptr(prob), int(work.shape[0]),
         ptr(work), ptr(out_offs), ptr(pred), ptr(counts), ptr(ws), nbytes)
    torch.cuda.synchronize()
    return list(torch.split(pred, sizes)) if want_pred else None


def _chain_counts(dset, ids, known, prob, c, counts):
    """Today's chain on the same inputs: geot_three_nn_ws per scan, then geot_seg_confusion_interp (adds into counts)."""
    from geot_amd.ext._common import call, knn_workspace, ptr
    n = known.shape[1]
    sizes = [dset.sizes[i] for i in ids]
    starts = np.concatenate([[0], np.cumsum(dset.sizes)])
    idx = torch.empty((sum(sizes), 3), dtype=torch.int32, device=DEV)
    dist2 = torch.empty((sum(sizes), 3), dtype=torch.float32, device=DEV)
    labels, at = [], 0
    for s, i in enumerate(ids):
        lo, m = int(starts[i]), sizes[s]
        unknown = dset.points[lo:lo + m].contiguous()
        wp, wb, _keep = knn_workspace(DEV, 1, m, n, 3)
        call("geot_three_nn_ws", DEV, 1, m, n, ptr(unknown), ptr(known[s]), ptr(dist2) + 12 * at, ptr(idx) + 12 * at, wp, wb)
        labels.append(dset.labels[lo:lo + m].to(torch.int64))
        at += m
    label, offs = torch.cat(labels), _offsets(sizes)
    call("geot_seg_confusion_interp", DEV, len(ids), c, n, ptr(offs), ptr(prob), ptr(idx), ptr(dist2), ptr(label), ptr(counts))
    torch.cuda.synchronize()
    return [lab for lab in labels]


# every C of {1, 2, 5, 17, 32}, every n of {1, 2, 3, 8, 2047, 2048, 16000, 24000}, B = 1..4; a 1-vertex scan, 63 / 64 / 65,
# 100 003, one scan in two slots, scan ids not ascending; the full-size cases (C = 17, M = 100 003, n = 16000 / 24000) with B = 2
CASES = [(1, 1, [0]), (2, 2, [3, 1]), (5, 3, [2, 0, 6]), (32, 8, [6, 1, 6, 0]), (17, 2047, [5, 3, 2]), (5, 2048, [5, 0, 1, 5]),
         (32, 2048, [4]), (2, 8, [4, 0]), (17, 16000, [4, 5]), (17, 24000, [5, 4])]


@pytest.mark.parametrize("c,n,ids", CASES)
def test_kernel_equals_the_chain(c, n, ids):
    from geot_amd.validation import get_pred_whole
    dset = _ragged_set()
    b, slots = len(ids), c * (c + 1) + 1
    got = torch.zeros((b, slots), dtype=torch.int64, device=DEV)
    chain = torch.zeros_like(got)
    binc = torch.zeros_like(got)
    for launch in range(2):                                   # two launches accumulate into the same counts
        known, logits = _known_and_logits(b, n, c, 1000 * c + n + launch)
        prob = torch.softmax(logits, dim=1).contiguous()
        preds = _kernel(dset, ids, known, prob, c, counts=got, want_pred=True)
        this = torch.zeros_like(got)                          # the chain's counts of this launch alone
        labels = _chain_counts(dset, ids, known, prob, c, this)
        chain += this
        wholes = [dset.points[int(dset.offsets[i]):int(dset.offsets[i + 1])] for i in ids]
        # get_pred_whole's `point * s + c` with s = 1, c = 0 hands the sampled points over as they are
        want = get_pred_whole(logits, known, wholes, [torch.zeros(1, 3, device=DEV)] * b, [torch.tensor(1.0, device=DEV)] * b)
        for s in range(b):
            assert _same(preds[s], want[s].reshape(-1)), (launch, s, int((preds[s] != want[s].reshape(-1)).sum()))
            binc[s] += torch.bincount(ref.torch_keys(want[s].reshape(-1), labels[s], c), minlength=slots)
        only_counts = torch.zeros_like(got)                   # counts without pred: the same numbers
        _kernel(dset, ids, known, prob, c, counts=only_counts)
        assert torch.equal(only_counts, this), (launch, int((only_counts - this).abs().sum()))
        only_preds = _kernel(dset, ids, known, prob, c, want_pred=True, with_labels=False)   # pred alone: labels may be NULL
        assert all(torch.equal(a, b) for a, b in zip(only_preds, preds)), launch
    print("C=%d n=%d ids=%s: counts differ from the chain by %d, from bincount by %d" %
          (c, n, ids, int((got - chain).abs().sum()), int((got - binc).abs().sum())))
    assert torch.equal(got, chain) and torch.equal(got, binc)
    assert torch.equal(got.sum(1), 2 * torch.tensor([dset.sizes[i] for i in ids], device=DEV))


def test_a_bad_slot_is_skipped_and_the_others_are_counted():
    """A scan id outside the set and work entries outside their scan: nothing of them is read or counted."""
    from geot_amd import _lib
    from geot_amd.ext._common import call, ptr
    from geot_amd.validation import scan_work_table
    dset = _ragged_set()
    c, n, ids = 5, 8, [1, 2]
    known, logits = _known_and_logits(2, n, c, 5)
    prob = torch.softmax(logits, dim=1).contiguous()
    want = torch.zeros((2, c * (c + 1) + 1), dtype=torch.int64, device=DEV)
    _kernel(dset, ids, known, prob, c, counts=want)
    table = scan_work_table([dset.sizes[i] for i in ids])
    extra = np.array([[2, 0, 5, 0], [-1, 0, 5, 0], [0, 63, 5, 0], [0, -1, 5, 0], [1, 0, 0, 0]], dtype=np.int32)   # all unusable
    for bad_ids, tab in (([1, len(dset)], table), ([1, -1], table), (ids, np.concatenate([table, extra]))):
        got = torch.zeros_like(want)
        ids_dev = torch.tensor(bad_ids, dtype=torch.int64, device=DEV)
        work = torch.from_numpy(np.ascontiguousarray(tab)).to(DEV)
        ws = torch.empty(int(_lib.load().geot_scan_predict_ws_bytes(2, n)), dtype=torch.uint8, device=DEV)
        call("geot_scan_predict", DEV, 2, c, n, len(dset), int(dset.points.shape[0]), ptr(dset.points), ptr(dset.labels),
             ptr(dset.offsets), ptr(ids_dev), ptr(known), ptr(prob), int(work.shape[0]), ptr(work), None, None, ptr(got),
             ptr(ws), ws.numel())
        torch.cuda.synchronize()
        if bad_ids == ids:
            assert torch.equal(got, want)
        else:
            assert torch.equal(got[0], want[0]) and int(got[1].sum()) == 0


# ------------------------------------------------------------------------------------------------ 2. adversarial
def _adversarial():
    """test_fused_path_with_exact_ties_nans_and_coincident_vertices on a scan set: a batch of three scans (the third with
    fewer vertices than num_points: duplicate sampled points, exact d2 ties decided by index), logits tied exactly between
    classes 3 and 5 at half the points, NaN logits, and -- in a second set the batch is re-pointed at -- vertices moved onto
    de-normalised sampled points, far outside their bounding box, and one NaN vertex."""
    from geot_amd.openpoints.dataset import DeviceScanSet, ValBatcher
    from geot_amd.synth import make_logits
    n, sizes = 12000, (40000, 25003, 1500)
    data = [_scan(m, 500 + i) for i, m in enumerate(sizes)]
    base = DeviceScanSet([p for p, _ in data], [lab for _, lab in data], cls=[0, 1, 0], device=DEV)
    np.random.seed(4)
    batch = ValBatcher(base, n).batch([1, 0, 2])
    rng = np.random.default_rng(9)
    pos = batch["pos"].cpu().numpy()
    logits = make_logits(pos, 9)
    tie = rng.random(n) < 0.5
    top = logits.max(1) + np.float32(2.0)
    logits[:, 3] = np.where(tie, top, logits[:, 3])
    logits[:, 5] = np.where(tie, top, logits[:, 5])
    logits[0, 7, rng.choice(n, 40, replace=False)] = np.nan
    logits[1, :, rng.choice(n, 25, replace=False)] = np.nan
    known = (batch["pos"] * batch["scale"].view(3, 1, 1) + batch["center"].view(3, 1, 3)).cpu().numpy()
    moved = [p.copy() for p, _ in data]
    for slot, scan in enumerate([1, 0, 2]):
        m = sizes[scan]
        on, at = rng.choice(n, m // 10, replace=False), rng.choice(m, m // 10, replace=False)
        moved[scan][at] = known[slot, on]                                   # d = 0 exactly
        far = rng.choice(m, 50, replace=False)
        moved[scan][far] = moved[scan][far] * np.float32(40.0) - np.float32(900.0)
        moved[scan][int(rng.integers(m))] = np.array([np.nan, 1.0, 2.0], np.float32)
    other = DeviceScanSet(moved, [lab for _, lab in data], cls=[0, 1, 0], device=DEV)
    batch = dict(batch, scans=other, points=list(torch.split(other.points, other.sizes)[i] for i in [1, 0, 2]),
                 labels=list(torch.split(other.labels, other.sizes)[i] for i in [1, 0, 2]))
    return torch.from_numpy(logits).to(DEV), batch


def _scans_and_chain(logits, batch):
    from geot_amd.validation import SegMetrics, get_pred_whole, predict_scans
    b = logits.shape[0]
    new, old = SegMetrics(17, DEV), SegMetrics(17, DEV)
    new.update_from_scans(logits, batch)
    old.update_from_logits(logits, batch["pos"], batch["points"], batch["center"], batch["scale"], batch["labels"], batch["cls"])
    preds = predict_scans(logits, batch)
    want = get_pred_whole(logits, batch["pos"], batch["points"], batch["center"], batch["scale"])
    torch.cuda.synchronize()
    assert len(preds) == len(want) == b and new.mandible == old.mandible
    for p, w in zip(preds, want):
        assert _same(p, w), int((p != w).sum())
    assert torch.equal(new.counts[:b], old.counts[:b]), int((new.counts[:b] - old.counts[:b]).abs().sum())
    return new.counts[:b].clone(), preds


def test_ties_nans_coincident_duplicate_far_and_nan_vertices(monkeypatch):
    logits, batch = _adversarial()
    monkeypatch.delenv("GEOT_NN_IMPL", raising=False)
    counts, preds = _scans_and_chain(logits, batch)
    assert all(int((p == 3).sum()) > 0 and int((p == 5).sum()) < int((p == 3).sum()) for p in preds)
    assert all(int((p == 0).sum()) > 0 for p in preds)
    for impl in ("wave", "grid", "basic"):                     # the library reads the variable at every call
        monkeypatch.setenv("GEOT_NN_IMPL", impl)
        counts_i, preds_i = _scans_and_chain(logits, batch)
        assert torch.equal(counts_i, counts), impl
        assert all(torch.equal(a, b) for a, b in zip(preds_i, preds)), impl


# ------------------------------------------------------------------------------------------------ 3. batcher
def test_batch_equals_prepare_sample_and_the_weak_view_scan_by_scan():
    from geot_amd.openpoints.dataset import ValBatcher, draw_view_params, fixmatch_views, prepare_sample
    sizes, jaws = [5000, 1, 700, 2600, 65], [0, 1, 1, 0, 1]
    dset = _set(sizes, 700, cls=jaws)
    m, ids = 2048, [3, 0, 4, 1, 1, 2]                          # N < m for three scans, a 1-vertex scan, a scan twice
    batcher = ValBatcher(dset, m)
    np.random.seed(12)
    batch = batcher.batch(ids, check=True)
    np.random.seed(12)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    assert batch["sizes"] == [sizes[i] for i in ids] and batch["mandible"] == [jaws[i] == 0 for i in ids]
    assert batch["scans"] is dset and torch.equal(batch["scan_ids"], torch.tensor(ids, device=DEV))
    assert batch["cls"].dtype == torch.int64 and torch.equal(batch["cls"], torch.tensor(jaws, device=DEV)[ids].view(-1, 1))
    assert batch["y"].dtype == torch.int64 and batch["pos"].shape == (6, m, 3) and batch["x"].shape == (6, 3, m)
    for slot, i in enumerate(ids):
        pts, lab = dset.points[starts[i]:starts[i + 1]], dset.labels[starts[i]:starts[i + 1]]
        assert batch["points"][slot].data_ptr() == pts.data_ptr() and torch.equal(batch["points"][slot], pts)   # zero-copy
        assert batch["labels"][slot].data_ptr() == lab.data_ptr() and torch.equal(batch["labels"][slot], lab)
        sel = np.random.choice(sizes[i], m, replace=sizes[i] < m)
        one = prepare_sample(pts, lab, torch.from_numpy(sel).to(DEV))
        view = fixmatch_views(one["pos"][None].contiguous(), [(0, 0, draw_view_params("train_w"))], 1)
        for key, want in (("pos", view["pos"][0]), ("x", view["x"][0]), ("y", one["y"]), ("center", one["center"]),
                          ("scale", one["scale"])):
            assert _same(batch[key][slot], want.reshape(batch[key][slot].shape)), (slot, key)


def test_batches_against_the_reference_fixture():
    from geot_amd.openpoints.dataset import DeviceScanSet, ValBatcher, draw_val_sel
    fx = np.load(FIXTURE, allow_pickle=False)
    count = sum(1 for k in fx.files if k.startswith("scan"))
    dset = DeviceScanSet([fx["scan%d" % i] for i in range(count)], [fx["lab%d" % i] for i in range(count)], cls=fx["cls"], device=DEV)
    batcher = ValBatcher(dset, int(fx["num_points"]), int(fx["num_classes"]))
    seed = int(fx["seed"])
    np.random.seed(seed)
    torch.manual_seed(seed)
    for k in range(int(fx["batches"])):                        # the recorded draws
        ids = fx["b%d_ids" % k]
        assert np.array_equal(draw_val_sel([dset.sizes[i] for i in ids], batcher.m), fx["b%d_sel" % k])
    np.random.seed(seed)
    torch.manual_seed(seed)
    worst = 0.0
    for k in range(int(fx["batches"])):
        batch = batcher.batch(fx["b%d_ids" % k])
        p = "b%d_" % k
        for key in ("y", "cls"):
            got = batch[key].cpu().numpy()
            assert got.dtype == fx[p + key].dtype and np.array_equal(got, fx[p + key]), (k, key)
        for key in ("pos", "x", "center", "scale"):
            got, want = batch[key].cpu().numpy(), fx[p + key]
            assert got.dtype == want.dtype and got.shape == want.shape, (k, key)
            for slot in range(len(want)):                      # 1e-5 relative to the scale of the element's row
                row = float(np.abs(want[slot]).max())
                err = float(np.abs(got[slot].astype(np.float64) - want[slot]).max())
                worst = max(worst, err / row)
                print("batch %d %s[%d]: |ours - reference| = %.3e, row scale %.3e" % (k, key, slot, err, row))
                assert err <= 1e-5 * row, (k, key, slot, err, row)
    assert np.array_equal(np.random.random_sample(4), fx["next_np"])          # the generators' next draws
    assert np.array_equal(torch.rand(4).numpy(), fx["next_torch"])
    print("worst relative difference %.3e" % worst)


# ------------------------------------------------------------------------------------------------ 4. end to end
class _Recorder:
    def __init__(self, model):
        self.model, self.logits = model, []

    def eval(self):
        self.model.eval()
        return self

    def __call__(self, data):
        out = self.model(data)
        self.logits.append(out[0].clone())
        return out


def _same_read(a, b):
    assert a["scans"] == b["scans"] and a["labels_out_of_range"] == b["labels_out_of_range"]
    for key in ("acc_list", "miou_list", "mdsc_list"):
        assert len(a[key]) == len(b[key])
        for x, y in zip(a[key], b[key]):
            assert type(x) is type(y) and np.asarray(x).dtype == np.asarray(y).dtype and ref.same_value(x, y), (key, x, y)
    for key in ref.JAW_KEYS:
        assert np.asarray(a[key]).dtype == np.asarray(b[key]).dtype and ref.same_value(a[key], b[key]), (key, a[key], b[key])


def _check_validate_scans(model, dset, n, batch_size, indices=None):
    from geot_amd.openpoints.dataset import ValBatcher
    from geot_amd.validation import SegMetrics, validate, validate_scans
    cfg = type("Cfg", (), {"num_classes": 17, "num_points": n, "epoch": 3, "epochs": 100})()
    order = list(range(len(dset))) if indices is None else list(indices)
    parts = [order[at:at + batch_size] for at in range(0, len(order), batch_size)]
    with quiet():
        np.random.seed(99)
        rec = _Recorder(model)
        got = validate_scans(rec, dset, cfg, batch_size=batch_size, indices=indices)
        np.random.seed(99)
        on_stream = validate_scans(model, dset, cfg, batch_size=batch_size, indices=indices, stream=torch.cuda.Stream(DEV))
        np.random.seed(99)
        batcher = ValBatcher(dset, n)
        batches = [batcher.batch(p) for p in parts]                               # the very batches validate_scans saw
        loader = [dict(b, x=b["x"].transpose(1, 2).contiguous()) for b in batches]   # collate_fn_val's layout: validate transposes
        rec_old = _Recorder(model)
        want = validate(rec_old, loader, cfg)
        new, old = SegMetrics(17, DEV), SegMetrics(17, DEV)
        for b, logits in zip(batches, rec.logits):
            new.update_from_scans(logits, b)
            old.update_from_logits(logits, b["pos"], b["points"], b["center"], b["scale"], b["labels"], b["cls"])
        _same_read(new.read(), old.read())
    assert len(rec.logits) == len(rec_old.logits) == len(parts)
    assert all(torch.equal(a, b) for a, b in zip(rec.logits, rec_old.logits))
    for g, s, w, k in zip(got, on_stream, want, ("whole_macc", "whole_miou", "whole_mdsc")):
        print("validate_scans %s: %r (validate %r, side stream %r)" % (k, g, w, s))
        assert np.asarray(g).dtype == np.asarray(w).dtype == np.asarray(s).dtype, k
        assert ref.same_value(g, w) and ref.same_value(s, w), (k, g, s, w)
    return got


def test_validate_scans_equals_validate_on_the_same_batches():
    from test_seg_metrics_gpu import _SeededLogits
    dset = _set([30011, 20000, 1500, 25000, 9000], 800, cls=[0, 1, 1, 1, 0])     # mixed jaws, 1500 < num_points
    got = _check_validate_scans(_SeededLogits(), dset, 8000, 2)                  # three batches, the last one short
    assert all(np.isfinite(float(g)) for g in got)
    _check_validate_scans(_SeededLogits(), dset, 8000, 2, indices=[4, 2, 1])     # a rank's shard


def test_validate_scans_with_the_configured_model():
    from geot_amd.openpoints.models.segmentation import WholePartSeg
    from test_seg_metrics_gpu import SMALL
    torch.manual_seed(0)
    model = WholePartSeg(segmentor_args=dict(NAME="PointTransformer_seg_T", **SMALL)).to(DEV)
    _check_validate_scans(model, _set([30011, 19993], 820, cls=[0, 1]), 8000, 2)


# ------------------------------------------------------------------------------------------------ 5. no host synchronisation
def test_nothing_synchronises_and_the_calls_do_not_depend_on_the_batch():
    from geot_amd.ext import _common
    from geot_amd.openpoints.dataset import ValBatcher
    from geot_amd.validation import SegMetrics, predict_scans
    dset = _set([20000, 9999, 3000, 64], 900, cls=[0, 1, 0, 1])
    batcher, metrics = ValBatcher(dset, 4096), SegMetrics(17, DEV)
    logits4 = torch.randn(4, 17, 4096, device=DEV)
    warm = batcher.batch([0, 1, 2, 3])                          # warm: kernels, workspace, pinned pool
    metrics.update_from_scans(logits4, warm)
    predict_scans(logits4, warm)
    metrics.reset()
    torch.cuda.synchronize()
    names = {}
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError, match="synchroniz"):
            logits4.sum().item()
        for ids in ([2], [0, 1, 2, 3], [3, 1], [1, 0, 3, 2], [0, 1, 2, 3]):     # past the first capacity of 8 scans
            batch = batcher.batch(ids)
            logits = logits4[:len(ids)].contiguous()
            seen = []
            _common.trace = lambda launch, name, seen=seen: (seen.append(name), launch())[1]
            try:
                metrics.update_from_scans(logits, batch)
            finally:
                _common.trace = None
            names.setdefault(len(ids), seen)
            predict_scans(logits, batch)
    finally:
        _common.trace = None
        torch.cuda.set_sync_debug_mode(0)
    assert names[1] == names[4] == ["geot_scan_predict"], names
    assert metrics.read()["scans"] == 15


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals():
    from geot_amd import _lib
    from geot_amd.ext._common import call, ptr
    from geot_amd.openpoints.dataset import ValBatcher
    from geot_amd.validation import SegMetrics, predict_scans, scan_work_table, validate_scans
    dset = _set([3000, 64], 950, cls=[0, 1])
    batcher, metrics = ValBatcher(dset, 2048), SegMetrics(17, DEV)
    batch = batcher.batch([0, 1])
    good = torch.randn(2, 17, 2048, device=DEV)
    for bad, msg in ((good.cpu(), "CPU not supported"), (good[:, :16].contiguous(), "fp32 logits"), (good.half(), "fp32 logits"),
                     (good[:1].contiguous(), "logits rows"), (good[:, :, :2000].contiguous(), "must agree"), (good[0], "fp32 logits")):
        with pytest.raises(RuntimeError, match=msg):
            metrics.update_from_scans(bad, batch)
        if bad.dim() != 3 or bad.shape[1] == 17:              # predict_scans takes the class count from the logits
            with pytest.raises(RuntimeError, match=msg.replace("fp32 logits", "logits")):
                predict_scans(bad, batch)
    for key, bad in (("scan_ids", batch["scan_ids"].to(torch.int32)), ("pos", batch["pos"].cpu()), ("scale", batch["scale"].double()),
                     ("center", batch["center"].cpu().numpy())):
        with pytest.raises(RuntimeError, match="must be|CPU"):
            metrics.update_from_scans(good, dict(batch, **{key: bad}))
    assert metrics.scans == 0 and int(metrics.counts.abs().sum()) == 0
    for idx in ([2], [-1], [0, 5], []):
        with pytest.raises(RuntimeError, match="idx must lie|at least one scan"):
            batcher.batch(idx)
    with pytest.raises(IndexError, match="outside the scan"):
        batcher.batch([1], sel=np.full((1, 2048), 64, dtype=np.int64), check=True)
    # the C entry point: bad b / c / n are refused before any launch
    prob = torch.softmax(good, dim=1).contiguous()
    known = torch.zeros(2, 2048, 3, device=DEV)
    work = torch.from_numpy(scan_work_table(dset.sizes)).to(DEV)
    counts = torch.zeros((2, 17 * 18 + 1), dtype=torch.int64, device=DEV)
    ws = torch.empty(int(_lib.load().geot_scan_predict_ws_bytes(2, 2048)), dtype=torch.uint8, device=DEV)

    def launch(b=2, c=17, n=2048, n_scans=2, total=3064, pts=dset.points, cnt=counts, wsp=ws, nbytes=None, table=work, lab=dset.labels):
        call("geot_scan_predict", DEV, b, c, n, n_scans, total, ptr(pts), ptr(lab), ptr(dset.offsets), ptr(batch["scan_ids"]),
             ptr(known), ptr(prob), int(work.shape[0]), ptr(table), None, None, ptr(cnt), ptr(wsp), ws.numel() if nbytes is None else nbytes)
    for kw in (dict(b=-1), dict(b=65536), dict(c=0), dict(c=33), dict(n=0), dict(n=-5), dict(n_scans=0), dict(total=0), dict(pts=None),
               dict(cnt=None), dict(lab=None), dict(wsp=None), dict(nbytes=16), dict(table=None)):
        with pytest.raises(RuntimeError, match="hipError 1"):
            launch(**kw)
    launch(b=0)
    torch.cuda.synchronize()
    assert int(counts.abs().sum()) == 0
    launch()
    torch.cuda.synchronize()
    assert int(counts.sum()) == 3064
    # an empty index list: nothing is counted, the model is never called

    class Never:
        def eval(self):
            return self

        def __call__(self, data):
            raise AssertionError("called")
    cfg = type("Cfg", (), {"num_classes": 17, "num_points": 2048, "epoch": 0, "epochs": 1})()
    with quiet():
        out = validate_scans(Never(), dset, cfg, indices=[])
    assert all(np.isnan(float(v)) for v in out)
    with pytest.raises(RuntimeError, match="num_points"):
        validate_scans(Never(), dset, type("Cfg", (), {"num_classes": 17})())
