"""islands= through the label-returning calls, the validators and fit() (geot_amd/validation.py, geot_amd/fit.py), on the tiny
384-wide model and the two scans of the decode model tests (tests/_scan_decode_ref.py): with islands=None every call makes
the launches and returns the bits of a call without the keyword; with islands on, the labels are clean_scans of the labels
without it, and the validators' three values and the ToothScores rows are the ones computed from those labels; refine= runs
first; fit() records the cleaned validation.  And the synthetic property: small clusters of a wrong tooth label strictly
inside other teeth are handed back exactly (tests/_scan_islands_ref.py property_case)."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scan_decode_ref as dref  # noqa: E402
import _scan_islands_ref as iref  # noqa: E402
import _seg_metrics_ref as sref  # noqa: E402
from _seg_metrics_ref import quiet  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N = dref.N_SAMPLE
IDS = [0, 1]
KINDS = ["interp", "voted", "covered", "decoded"]
ISLANDS = {"min_size": 6, "k": 6}                    # not the defaults: the dict reaches clean_scans
_cache = {}


def _world():
    if "world" not in _cache:
        from geot_amd.openpoints.dataset import DeviceScanSet
        from geot_amd.openpoints.models.segmentation import WholePartSeg
        scans = dref.tiny_scans()
        dset = DeviceScanSet([p for p, _ in scans], [l for _, l in scans], cls=[0, 1], device=DEV)
        model = WholePartSeg(segmentor_args=dref.tiny_model().to(DEV)).eval()
        cfg = type("Cfg", (), {"num_classes": 17, "num_points": N, "epoch": 1, "epochs": 2})()
        _cache["world"] = dict(dset=dset, model=model, cfg=cfg)
    return _cache["world"]


def _seed():
    np.random.seed(2)
    random.seed(2)
    torch.manual_seed(2)


def _batcher(kind):
    from geot_amd.openpoints.dataset import ValBatcher, VoteBatcher
    from geot_amd.openpoints.dataset.sample_draw import DeviceDraws
    return (VoteBatcher if kind == "voted" else ValBatcher)(_world()["dset"], N, draws=DeviceDraws(5))      # the same counter: the same batches


def _validator(kind, **kw):
    from geot_amd import validation as V
    w = _world()
    _seed()
    with quiet():
        if kind == "interp":
            return V.validate_scans(w["model"], _batcher(kind), w["cfg"], **kw)
        if kind == "voted":
            return V.validate_scans_voted(w["model"], _batcher(kind), w["cfg"], num_votes=2, **kw)
        if kind == "covered":
            return V.validate_scans_covered(w["model"], _batcher(kind), w["cfg"], **kw)
        return V.validate_scans_decoded(w["model"], _batcher(kind), w["cfg"], chunk=100, **kw)


def _labels(kind, **kw):
    """The labels of the matching public call under the same seeds."""
    from geot_amd import validation as V
    w = _world()
    _seed()
    with torch.no_grad():
        if kind == "interp":
            data = _batcher(kind).batch(IDS)
            return V.predict_scans(w["model"](data)[0], data, **kw)
        if kind == "voted":
            return V.vote_scans(w["model"], _batcher(kind), IDS, 2, **kw)
        if kind == "covered":
            return V.cover_scans(w["model"], _batcher(kind), IDS, **kw)
        return V.decode_scans(w["model"], _batcher(kind), IDS, chunk=100, **kw)


def _traced(fn):
    from geot_amd.ext import _common
    seen = []
    _common.trace = lambda launch, name: (seen.append(name), launch())[1]
    try:
        out = fn()
    finally:
        _common.trace = None
    return seen, out


def _same_triple(a, b):
    return len(a) == len(b) == 3 and all(np.asarray(x).dtype == np.asarray(y).dtype and sref.same_value(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", KINDS)
def test_islands_off_is_the_call_without_the_keyword(kind):
    _validator(kind)                                                    # warm
    base_launches, base = _traced(lambda: _validator(kind))
    label_launches, labels = _traced(lambda: _labels(kind))
    assert "geot_scan_islands" not in base_launches + label_launches
    for off in (None, False):
        launches, got = _traced(lambda: _validator(kind, islands=off))
        assert launches == base_launches and _same_triple(got, base)
        launches, got = _traced(lambda: _labels(kind, islands=off))
        assert launches == label_launches and all(torch.equal(g, l) for g, l in zip(got, labels))


def _by_hand(preds, kind):
    """validate()'s three values and the ToothScores rows of given labels."""
    from geot_amd import validation as V
    w = _world()
    batch = _batcher(kind).batch(IDS)
    metrics = V.SegMetrics(17, DEV)
    metrics.update(preds, V._scan_labels(batch), [0 if m else 1 for m in batch["mandible"]])
    out = metrics.read()
    teeth = V.ToothScores(17, DEV)
    teeth.update(preds, batch)
    return (out["whole_macc"], out["whole_miou"], out["whole_mdsc"]), teeth, batch


@pytest.mark.parametrize("islands", [True, ISLANDS])
@pytest.mark.parametrize("kind", KINDS)
def test_islands_on_cleans_the_labels_of_the_call_without(kind, islands):
    from geot_amd import validation as V
    kw = {} if islands is True else islands
    plain = _labels(kind)
    want = V.clean_scans([p.clone() for p in plain], _batcher(kind).batch(IDS), num_classes=17, **kw)
    got = _labels(kind, islands=islands)
    assert all(torch.equal(g, w_) and g.dtype == torch.int64 and g.shape == p.shape for g, w_, p in zip(got, want, plain))
    print("%s, islands=%r: %d vertices relabelled" % (kind, islands, sum(int((g != p).sum()) for g, p in zip(got, plain))))
    triple, by_hand, batch = _by_hand(want, kind)
    teeth = V.ToothScores(17, DEV)
    launches, scored = _traced(lambda: _validator(kind, islands=islands, teeth=teeth))
    assert _same_triple(scored, triple)
    at = [launches.index(name) for name in ("geot_scan_islands", "geot_seg_confusion", "geot_tooth_moments")]
    assert launches.count("geot_scan_islands") == 1 and at == sorted(at)
    assert teeth.mandible == by_hand.mandible and torch.equal(teeth.moments[:2], by_hand.moments[:2]) and teeth.moments[:2].any()
    a, b = teeth.read(), by_hand.read()
    assert all(sref.same_value(a[key], b[key]) for key in ("tsa", "tla", "tir", "score"))
    # the restatement on the same labels and the same table
    table = V.scan_neighbours(batch, k=kw.get("k", 8))
    nbrs = [t.cpu().numpy() for t in torch.split(table, batch["sizes"])]
    ref, _, _ = iref.scan_islands([p.cpu().numpy().reshape(-1) for p in plain], nbrs, 17, kw.get("min_size", 10), [0x1fffe] * 2, None)
    assert all(np.array_equal(g.cpu().numpy().reshape(-1), r) for g, r in zip(got, ref))


@pytest.mark.parametrize("kind", KINDS)
def test_refine_runs_before_islands(kind):
    from geot_amd import validation as V
    plain = _labels(kind)
    batch = _batcher(kind).batch(IDS)
    refined = V.refine_scans([p.clone() for p in plain], batch, 10, num_classes=17)
    want = V.clean_scans([p.clone() for p in refined], batch, num_classes=17)
    other = V.refine_scans(V.clean_scans([p.clone() for p in plain], batch, num_classes=17), batch, 10, num_classes=17)
    launches, got = _traced(lambda: _labels(kind, refine=10, islands=True))
    assert all(torch.equal(g, w_) for g, w_ in zip(got, want))
    assert launches.index("geot_scan_refine") < launches.index("geot_scan_islands")
    launches, scored = _traced(lambda: _validator(kind, refine=10, islands=True))
    assert _same_triple(scored, _by_hand(want, kind)[0])
    assert launches.index("geot_scan_refine") < launches.index("geot_scan_islands") < launches.index("geot_seg_confusion")
    print("%s: the two orders differ on %d vertices" % (kind, sum(int((a != b).sum()) for a, b in zip(want, other))))


def test_refine_then_islands_on_noisy_labels_is_not_the_other_order():
    """The untrained model's labels are nearly constant, so the order cannot show on them: random logits give labels on
    which refine-then-clean and clean-then-refine differ, and predict_scans gives the first."""
    from geot_amd import validation as V
    batch = _batcher("interp").batch(IDS)
    logits = torch.randn(2, 17, N, generator=torch.Generator().manual_seed(3)).to(DEV)
    plain = V.predict_scans(logits, batch)
    want = V.clean_scans(V.refine_scans([p.clone() for p in plain], batch, 10, num_classes=17), batch, num_classes=17)
    other = V.refine_scans(V.clean_scans([p.clone() for p in plain], batch, num_classes=17), batch, 10, num_classes=17)
    got = V.predict_scans(logits, batch, refine=10, islands=True)
    assert all(torch.equal(g, w_) for g, w_ in zip(got, want))
    differ = sum(int((a != b).sum()) for a, b in zip(want, other))
    print("the two orders differ on %d of %d vertices" % (differ, sum(batch["sizes"])))
    assert differ > 0


def test_fit_records_the_cleaned_validation_and_refuses_a_bad_value_before_the_first_epoch():
    from geot_amd import train_step as ts
    from geot_amd import validation as V
    from geot_amd.fit import fit
    from geot_amd.openpoints.dataset import SupervisedBatcher, ValBatcher
    from geot_amd.openpoints.dataset.sample_draw import DeviceDraws
    from geot_amd.openpoints.models.segmentation import WholePartSeg
    w = _world()
    base = dict(lr=1e-3, sched="multistep", decay_epochs=[2], decay_rate=0.1, warmup_epochs=0, sched_on_epoch=True, epochs=1,
                val_freq=1, batch_size=2, batch_size_val=2, num_points=N, num_classes=17, num_votes=0, supervised_epochs=0)
    runs = {}
    for islands in (None, ISLANDS):
        torch.manual_seed(5)
        model = WholePartSeg(segmentor_args=dict(NAME="PointTransformer_seg_T", **dref.TINY)).to(DEV)
        step = ts.SupervisedStep(model)
        _seed()
        with quiet():
            launches, out = _traced(lambda: fit(step, SupervisedBatcher(w["dset"], N), dict(base),
                                                val=ValBatcher(w["dset"], N, draws=DeviceDraws(5)), log=lambda rec: None,
                                                generator=torch.Generator().manual_seed(7), islands=islands))
            again = V.validate_scans(model, ValBatcher(w["dset"], N, draws=DeviceDraws(5)), w["cfg"], islands=islands)
        rec = out["records"][-1]
        assert launches.count("geot_scan_islands") == (0 if islands is None else 1)
        assert (rec["val_acc"], rec["val_miou"], rec["val_dsc"]) == tuple(float(v) for v in again)
        runs[islands is None] = ({k: v.detach().clone() for k, v in model.state_dict().items()}, rec)
    (state_off, rec_off), (state_on, rec_on) = runs[True], runs[False]
    bits = lambda t: t.contiguous().reshape(-1).view(torch.uint8)     # noqa: E731
    assert all(torch.equal(bits(state_off[k]), bits(state_on[k])) for k in state_off)       # the training does not see it
    print("val_miou without / with islands: %r / %r" % (rec_off["val_miou"], rec_on["val_miou"]))
    # a bad value: ValueError before anything is trained
    torch.manual_seed(5)
    model = WholePartSeg(segmentor_args=dict(NAME="PointTransformer_seg_T", **dref.TINY)).to(DEV)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for bad in ("yes", 3, {"size": 4}):
        with pytest.raises(ValueError, match="islands"):
            fit(ts.SupervisedStep(model), SupervisedBatcher(w["dset"], N), dict(base), val=w["dset"], log=lambda rec: None, islands=bad)
    assert all(torch.equal(bits(before[k]), bits(v)) for k, v in model.state_dict().items())


def test_injected_clusters_inside_teeth_are_handed_back_exactly():
    """The synthetic property: blob teeth, five clusters of six vertices of a wrong tooth label strictly inside other teeth
    (below min_size = 10).  The kernel equals the restatement, and -- separately -- the restatement equals the uninjected
    labels (which tests/test_scan_islands_cpu.py also checks without a GPU)."""
    from geot_amd import validation as V
    from geot_amd.openpoints.dataset import DeviceScanSet
    case = iref.property_case()
    dset = DeviceScanSet([p for p, _, _, _ in case], [l.astype(np.int32) for _, l, _, _ in case], cls=[0, 1], device=DEV)
    batch = {"scans": dset, "sizes": list(dset.sizes), "scan_ids": torch.tensor([0, 1], dtype=torch.int64, device=DEV),
             "mandible": [True, False], "points": list(torch.split(dset.points, dset.sizes))}
    table = V.scan_neighbours(batch, k=iref.PROPERTY_K)
    assert np.array_equal(table.cpu().numpy(), np.concatenate([nbr for _, _, nbr, _ in case]))      # the table the CPU check used
    noisy = [torch.from_numpy(n).to(DEV).view(1, -1) for _, _, _, n in case]
    got, stats = V.clean_scans(noisy, batch, min_size=iref.PROPERTY_MIN_SIZE, keep_largest=True, num_classes=17, stats=True)
    want, _, want_stats = iref.scan_islands([n for _, _, _, n in case], [nbr for _, _, nbr, _ in case], 17, iref.PROPERTY_MIN_SIZE,
                                            [iref.PROPERTY_KEEP] * 2, None)
    for g, w_, (_, truth, _, _) in zip(got, want, case):
        assert np.array_equal(g.cpu().numpy().reshape(-1), w_)           # the kernel is the restatement
        assert np.array_equal(w_, truth)                                 # the restatement restores the truth
    assert np.array_equal(stats.cpu().numpy(), want_stats) and want_stats.tolist() == [[12, 5, 30, 0]] * 2
    comp = V.scan_components(got, batch, nbr=table, num_classes=17)
    result = V.teeth3ds_result(got[0], comp[0], "lower", patient="synthetic")
    assert sorted(set(result["instances"])) == list(range(7)) and sorted(set(result["labels"])) == [0, 31, 32, 33, 34, 35, 36]
