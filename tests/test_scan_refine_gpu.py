"""geot_scan_refine (csrc/scan_refine.hip) and what is built on it in geot_amd/validation.py -- refine_scans,
part_seg_refinement, the `refine` keyword of predict_scans / vote_scans / validate_scans / validate_scans_voted -- against the
numpy restatement of tests/_scan_refine_ref.py, torch.equal everywhere; the dense form also against the reference-executed
fixture tests/golden/part_seg_refinement_ref.npz.  Shapes: the smallest at which each branch of the kernels can go wrong."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scan_refine_ref as rref  # noqa: E402
import _seg_metrics_ref as ref  # noqa: E402
from _seg_metrics_ref import quiet  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "part_seg_refinement_ref.npz")
LINE = np.array([[float(x), 0.0, 0.0] for x in (0, 1, 2, 3, 10, 11, 12, 13)], np.float32)


def _cloud(m, seed, dup=0):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(m, 3)) * np.array([30.0, 20.0, 10.0]) + np.array([14.0, -37.0, 61.0])).astype(np.float32)
    if dup:
        x[rng.integers(0, m, dup)] = x[rng.integers(0, m, dup)]       # exact duplicates: distance ties decided by index
    return x


def _labels(pts, c, seed, islands=6):
    """Regions along x with islands of 1 .. 12 vertices of other classes: small classes, large classes, neighbours of both."""
    rng = np.random.default_rng(seed)
    m = len(pts)
    pred = (np.argsort(np.argsort(pts[:, 0])) * min(c, 3) // m).astype(np.int64)
    for k in range(islands):
        at = int(rng.integers(m))
        near = np.argsort(((pts - pts[at]) ** 2).sum(1), kind="stable")[:int(rng.integers(1, 13))]
        pred[near] = int(rng.integers(c))
    return pred


def _set(clouds):
    from geot_amd.openpoints.dataset import DeviceScanSet
    return DeviceScanSet(clouds, [np.zeros(len(x), np.int32) for x in clouds], cls=[0] * len(clouds), device=DEV)


def _batch(dset, ids, mandible=None):
    return {"scans": dset, "sizes": [dset.sizes[i] for i in ids], "scan_ids": torch.tensor(ids, dtype=torch.int64, device=DEV),
            "mandible": [True] * len(ids) if mandible is None else mandible}


def _as_views(preds):
    """Per-slot label arrays -> (1, M_i) views of one device buffer, as predict_scans returns them."""
    flat = torch.from_numpy(np.concatenate(preds).astype(np.int64)).to(DEV)
    return [p.view(1, -1) for p in torch.split(flat, [len(p) for p in preds])]


def _check(clouds, ids, preds, c, n, parts=None, mandible=None):
    """refine_scans on slots `ids` of a set of `clouds` with per-slot labels `preds`: labels and every stats column against
    the restatement, in place on the views, the same bits from a second call."""
    from geot_amd.validation import refine_scans
    dset = _set(clouds)
    batch = _batch(dset, ids, mandible)
    jaws = [0 if m else 1 for m in batch["mandible"]]
    want, want_stats = rref.refine_scans(preds, [clouds[i] for i in ids], c, n, None if parts is None else [parts[j] for j in jaws])
    views = _as_views(preds)
    got, stats = refine_scans(views, batch, n, parts, stats=True, num_classes=c)
    again, stats2 = refine_scans(_as_views(preds), batch, n, parts, stats=True, num_classes=c)
    torch.cuda.synchronize()
    print("c=%d n=%d sizes=%s: stats (steps, queries, changed, outside) %s" % (c, n, batch["sizes"], stats.cpu().tolist()))
    assert all(g is v for g, v in zip(got, views))                      # in place: the same views
    for s, (g, a, w) in enumerate(zip(got, again, want)):
        assert g.dtype == torch.int64 and tuple(g.shape) == (1, len(w))
        assert torch.equal(g.cpu().reshape(-1), torch.from_numpy(w)), (s, int((g.cpu().reshape(-1) != torch.from_numpy(w)).sum()))
        assert torch.equal(g, a), s
    assert stats.dtype == torch.int32 and torch.equal(stats.cpu(), torch.from_numpy(want_stats)) and torch.equal(stats, stats2)
    return want_stats


@pytest.mark.parametrize("m", [11, 64, 65, 257, 1000])
def test_sizes_around_the_64_vertex_step(m):
    pts = _cloud(m, m)
    st = _check([pts], [0], [_labels(pts, 17, m + 1)], 17, 10, parts=[[0, 1, 3, 4, 5, 6, 7, 8], [0]])
    assert st[0, 1] >= 1                                                # something was refined


def test_ragged_slots_one_scan_twice_and_another_slot_order():
    clouds = [_cloud(m, 40 + i, dup=m // 20) for i, m in enumerate([65, 300, 11, 1000])]
    ids = [3, 1, 3, 0, 2]
    preds = [_labels(clouds[i], 17, 50 + s) for s, i in enumerate(ids)]
    st = _check(clouds, ids, preds, 17, 10, parts=[[0, 1, 2, 3, 4, 5, 6, 7, 8], [0, 2, 9, 10, 11, 12]],
                mandible=[True, False, False, True, True])
    assert (st[:, 1] > 0).sum() >= 3 and not np.array_equal(st[0], st[2])       # the two slots of scan 3 got their own labels


@pytest.mark.parametrize("n,c", [(1, 2), (10, 1), (63, 17), (10, 32), (1, 32), (63, 2), (5, 17)])
def test_every_n_and_class_count(n, c):
    pts = _cloud(130, 7 * n + c, dup=6)
    pred = _labels(pts, c, n + c, islands=10)
    st = _check([pts], [0], [pred], c, n, parts=[list(range(1, c)) or [0]])      # class 0, a region, is not allowed
    assert c == 1 or st[0, 0] >= 1


def test_one_class_exactly_n_members_and_n_minus_one():
    pts = _cloud(200, 3)
    near = np.argsort(((pts - pts[17]) ** 2).sum(1), kind="stable")
    one = np.full(200, 4, np.int64)                                      # one class, not even allowed: untouched
    exact = np.zeros(200, np.int64)
    exact[near[:10]] = 5                                                 # exactly n = 10 members: kept
    below = np.zeros(200, np.int64)
    below[near[:9]] = 5                                                  # n - 1: refined
    st = _check([pts], [0, 0, 0], [one, exact, below], 17, 10, parts=[[0, 5]])
    assert st[:, :3].tolist() == [[0, 0, 0], [0, 0, 0], [1, 9, 9]]


def test_a_disallowed_class_with_most_of_the_scan_wraps_the_persistent_loop():
    """8700 queries in one slot: more than the search kernel has waves (8192), and the second slot's first query does not start
    at wave 0.  The inner vertices see their own class only: all-zero votes give class 0."""
    pts, small = _cloud(9000, 90), _cloud(300, 91)
    pred = np.full(9000, 3, np.int64)
    pred[np.argsort(pts[:, 1])[:300]] = 1
    other = np.full(300, 3, np.int64)
    other[np.argsort(small[:, 0])[:40]] = 2
    st = _check([pts, small], [0, 1], [pred, other], 17, 10, parts=[[0, 1, 2]])
    assert st[:, :2].tolist() == [[1, 8700], [1, 260]]


def test_hand_checked_cases_through_the_dense_form():
    """The cases of tests/test_scan_refine_cpu.py, whose answers are worked out there: the snapshot rule (a class refined into
    another small class), two small classes that are each other's neighbours in both orders, an equal vote, an all-zero vote."""
    from geot_amd.validation import part_seg_refinement
    swapped = LINE.copy()
    swapped[[1, 2]] = swapped[[2, 1]]
    cases = [  # (labels, points, classes, n, allowed, answer)
        ([0, 1, 2, 0, 0, 0, 0, 0], LINE, 3, 2, None, [0] * 8),
        ([2, 1, 2, 3, 3, 3, 3, 3], LINE, 4, 3, None, [1, 3, 1, 3, 3, 3, 3, 3]),            # not [3, 3, 3, ...]: the aliasing form
        ([1, 2, 1, 3, 3, 3, 3, 3], LINE, 4, 3, None, [2, 3, 2, 3, 3, 3, 3, 3]),
        ([3, 1, 2, 3, 3, 3, 3, 3], LINE, 4, 2, None, [3, 2, 3, 3, 3, 3, 3, 3]),
        ([3, 2, 1, 3, 3, 3, 3, 3], LINE, 4, 2, None, [3, 1, 3, 3, 3, 3, 3, 3]),
        ([3, 2, 1, 3, 3, 3, 3, 3], swapped, 4, 2, None, [3, 1, 3, 3, 3, 3, 3, 3]),
        ([3, 1, 2, 2, 3, 3, 3, 3], LINE, 4, 3, None, [3, 2, 3, 3, 3, 3, 3, 3]),            # v1 -> 2, then v2, v3: (2, 2, 2, 3) -> 3
        ([2, 2, 2, 2, 1, 1, 1, 1], LINE, 3, 3, [0, 1], [0, 0, 0, 0, 1, 1, 1, 1]),
        ([2, 2, 2, 2, 2, 2, 2, 2], LINE, 3, 3, [0, 1], [2] * 8),
        ([1, 1, 1, 0, 0, 0, 0, 0], LINE, 2, 3, None, [1, 1, 1, 0, 0, 0, 0, 0]),
        ([1, 1, 1, 0, 0, 0, 0, 0], LINE, 2, 4, None, [0] * 8),
    ]
    for labels, pts, c, n, allowed, answer in cases:
        want, _ = rref.refine_scan(np.array(labels), pts, c, n, allowed)
        assert want.tolist() == answer, (labels, want.tolist())
        pred = torch.tensor([labels, labels], dtype=torch.int64, device=DEV)
        pos = torch.from_numpy(np.stack([pts, pts])).to(DEV)
        parts = [list(range(c)) if allowed is None else allowed, list(range(c))]
        out = part_seg_refinement(pred, pos, torch.tensor([0, 0]), parts, n=n)
        assert out is pred and pred.cpu().tolist() == [answer, answer], (labels, pred.cpu().tolist())


def test_dense_form_equals_the_reference_fixture():
    from geot_amd.validation import part_seg_refinement
    fx = np.load(FIXTURE)
    pred = torch.from_numpy(fx["pred"].astype(np.int64)).to(DEV)
    pos = torch.from_numpy(fx["pos"]).to(DEV)
    out = part_seg_refinement(pred, pos, torch.from_numpy(fx["cls"]), fx["cls2parts"].tolist(), n=int(fx["n"]))
    assert out is pred
    want = torch.from_numpy(fx["out"].astype(np.int64))
    print("fixture: %d of %d labels changed, %d differ from the reference" %
          (int((want != torch.from_numpy(fx["pred"].astype(np.int64))).sum()), want.numel(), int((pred.cpu() != want).sum())))
    assert torch.equal(pred.cpu(), want)
    assert not torch.equal(pred.cpu(), torch.from_numpy(fx["aliased"].astype(np.int64)))
    # rows of a larger tensor, a non-contiguous pos: the same labels
    wide = torch.from_numpy(fx["pos"]).to(DEV).transpose(0, 1).contiguous().transpose(0, 1)
    again = torch.from_numpy(fx["pred"].astype(np.int64)).to(DEV)
    assert torch.equal(part_seg_refinement(again, wide, fx["cls"].tolist(), fx["cls2parts"].tolist(), n=int(fx["n"])).cpu(), want)


def test_labels_outside_the_classes_are_untouched_and_counted():
    pts = _cloud(300, 11, dup=10)
    pred = _labels(pts, 5, 12, islands=12)
    rng = np.random.default_rng(13)
    out_of = rng.integers(0, 300, 25)
    pred[out_of[:10]] = 5                                                # = c
    pred[out_of[10:20]] = -1
    pred[out_of[20:]] = 1 << 40
    st = _check([pts], [0], [pred], 5, 10, parts=[[0, 1, 2]])
    assert st[0, 3] == len(set(out_of.tolist())) and st[0, 1] > 0


def _raw(dset, ids, preds, c, n, total_out=None, out_offsets=None, stats=True):
    """geot_scan_refine through the C ABI -> (flat labels, stats)."""
    from geot_amd import _lib
    from geot_amd.ext._common import call, ptr
    sizes = [len(p) for p in preds]
    flat = torch.from_numpy(np.concatenate(preds).astype(np.int64)).to(DEV)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]) if out_offsets is None else np.asarray(out_offsets)
    offs = torch.from_numpy(offs.astype(np.int64)).to(DEV)
    ids_dev = torch.tensor(ids, dtype=torch.int64, device=DEV)
    nbytes = int(_lib.load().geot_scan_refine_ws_bytes(len(ids), flat.numel() if total_out is None else total_out, n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    st = torch.full((len(ids), 4), -7, dtype=torch.int32, device=DEV) if stats else None
    call("geot_scan_refine", DEV, len(ids), c, n, len(dset), int(dset.points.shape[0]), ptr(dset.points), ptr(dset.offsets),
         ptr(ids_dev), ptr(offs), None, ptr(flat), ptr(st), ptr(ws), nbytes)
    torch.cuda.synchronize()
    return flat.cpu(), None if st is None else st.cpu()


def test_a_skipped_slot_leaves_its_rows_alone():
    """A scan id outside the set, and a slot the workspace has no room for: nothing of them is read or written, their stats are
    zeros, and the other slots are refined as if alone."""
    clouds = [_cloud(200, 21), _cloud(90, 22)]
    dset = _set(clouds)
    preds = [_labels(clouds[0], 17, 23), _labels(clouds[1], 17, 24), _labels(clouds[0], 17, 25)]
    want, want_stats = rref.refine_scans(preds, [clouds[0], clouds[1], clouds[0]], 17, 10)
    got, st = _raw(dset, [0, 1, 0], preds, 17, 10)
    assert torch.equal(got, torch.from_numpy(np.concatenate(want))) and torch.equal(st, torch.from_numpy(want_stats))
    assert _raw(dset, [0, 1, 0], preds, 17, 10, stats=False)[0].equal(got)              # stats is optional
    for bad in (len(dset), -1):
        got, st = _raw(dset, [0, bad, 0], preds, 17, 10)
        expect = np.concatenate([want[0], preds[1], want[2]])
        assert torch.equal(got, torch.from_numpy(expect)), bad
        assert st[1].tolist() == [0, 0, 0, 0] and torch.equal(st[[0, 2]], torch.from_numpy(want_stats[[0, 2]]))
    # the last slot starts where a workspace for 300 labels ends
    got, st = _raw(dset, [0, 1, 0], preds, 17, 10, total_out=300)
    assert torch.equal(got, torch.from_numpy(np.concatenate([want[0], want[1], preds[2]]))) and st[2].tolist() == [0, 0, 0, 0]


def _noisy_model():
    from test_seg_metrics_gpu import _SeededLogits

    class Noisy(_SeededLogits):
        def __call__(self, data):
            logits, a, b = super().__call__(data)
            g = torch.Generator(device=logits.device).manual_seed(int(logits.shape[2]))
            return logits + 2.5 * torch.randn(logits.shape, device=logits.device, generator=g), a, b
    return Noisy()


PARTS = [[0, 1, 2, 3, 4, 5, 6, 7, 8], [0, 9, 10, 11, 12, 13, 14, 15, 16]]


def _restated(preds, batch, n, parts):
    dset = batch["scans"]
    ids = batch["scan_ids"].cpu().tolist()
    lo = dset.offsets.cpu().tolist()
    clouds = [dset.points[lo[i]:lo[i + 1]].cpu().numpy() for i in ids]
    allowed = None if parts is None else [parts[0 if m else 1] for m in batch["mandible"]]
    return rref.refine_scans([p.cpu().numpy().reshape(-1) for p in preds], clouds, 17, n, allowed)[0]


def test_predict_scans_and_vote_scans_with_refine():
    from geot_amd.openpoints.dataset import ValBatcher, VoteBatcher
    from geot_amd.validation import predict_scans, refine_scans, vote_scans
    from test_val_scans_gpu import _set as scan_set
    dset = scan_set([3000, 777, 1500], 700, cls=[0, 1, 1])
    model = _noisy_model()
    np.random.seed(3)
    batch = ValBatcher(dset, 1024).batch([2, 0, 1])
    logits = model(batch)[0]
    plain = predict_scans(logits, batch)
    # every class allowed: n = 63 makes the classes of the 777-vertex scan small; with the jaws' lists n = 10 has work to do
    for n, parts in ((63, None), (10, PARTS)):
        want = _restated(plain, batch, n, parts)
        got = predict_scans(logits, batch, refine=n, parts=parts)
        two = refine_scans([p.clone() for p in predict_scans(logits, batch)], batch, n, parts, num_classes=17)   # not views: copied
        changed = sum(int((torch.from_numpy(w) != p.cpu().reshape(-1)).sum()) for w, p in zip(want, plain))
        print("predict_scans refine=%d parts=%s: %d labels changed" % (n, parts is not None, changed))
        assert changed > 0
        for g, t, w, p in zip(got, two, want, plain):
            assert g.shape == p.shape and torch.equal(g.cpu().reshape(-1), torch.from_numpy(w)) and torch.equal(g, t)
    assert all(torch.equal(a, b) for a, b in zip(predict_scans(logits, batch, refine=True), predict_scans(logits, batch, refine=10)))
    # votes: the same draws give the same voted labels; refined they equal the restatement of the unrefined ones
    voter = VoteBatcher(dset, 1024)
    np.random.seed(4)
    torch.manual_seed(4)
    voted = vote_scans(model, voter, [1, 2], 3)
    np.random.seed(4)
    torch.manual_seed(4)
    refined = vote_scans(model, voter, [1, 2], 3, refine=10, parts=PARTS)
    want = _restated(voted, _batch(dset, [1, 2], [False, False]), 10, PARTS)
    assert any(not torch.equal(a, b) for a, b in zip(voted, refined))
    assert all(torch.equal(g.cpu().reshape(-1), torch.from_numpy(w)) for g, w in zip(refined, want))


class _Recorder:
    def __init__(self, model):
        self.model, self.seen = model, []

    def eval(self):
        return self

    def __call__(self, data):
        out = self.model(data)
        self.seen.append((data, out[0].clone()))
        return out


def test_validators_with_refine_score_the_refined_labels(caplog):
    from geot_amd.validation import predict_scans, seg_metrics_from_counts, validate_scans, validate_scans_voted
    from test_val_scans_gpu import _set as scan_set
    dset = scan_set([3000, 777, 1500], 720, cls=[0, 1, 1])
    cfg = type("Cfg", (), {"num_classes": 17, "num_points": 1024, "epoch": 3, "epochs": 100, "num_votes": 2, "refine": True})()
    lo = dset.offsets.cpu().tolist()
    for voted in (False, True):
        rec = _Recorder(_noisy_model())
        np.random.seed(8)
        torch.manual_seed(8)
        with quiet():
            if voted:
                got = validate_scans_voted(rec, dset, cfg, batch_size=2, refine=10, parts=PARTS, vote=[])
            else:
                got = validate_scans(rec, dset, cfg, batch_size=2, refine=10, parts=PARTS)
        rows, jaws = [], []
        per_batch = 2 if voted else 1
        for k in range(0, len(rec.seen), per_batch):
            data = rec.seen[k][0]
            if voted:
                from geot_amd.validation import ScanVotes
                votes = ScanVotes(data, 17)
                votes.add(rec.seen[k][1], rec.seen[k][0])
                plain = votes.add(rec.seen[k + 1][1], rec.seen[k + 1][0], last=True, want_pred=True)
            else:
                plain = predict_scans(rec.seen[k][1], data)
            for w, i, m in zip(_restated(plain, data, 10, PARTS), data["scan_ids"].cpu().tolist(), data["mandible"]):
                rows.append(ref.bincount_counts(w, dset.labels[lo[i]:lo[i + 1]].cpu().numpy().astype(np.int64), 17))
                jaws.append(m)
        with quiet():
            want = seg_metrics_from_counts(np.stack(rows), 17, jaws)
        for g, key in zip(got, ("whole_macc", "whole_miou", "whole_mdsc")):
            print("%s refine=10 %s: %r (restated %r)" % ("validate_scans_voted" if voted else "validate_scans", key, g, want[key]))
            assert np.asarray(g).dtype == np.asarray(want[key]).dtype and ref.same_value(g, want[key]) and np.isfinite(float(g))


def test_refine_0_is_todays_path(caplog):
    """Same tensors, same log lines, same launches; a config that carries refine: True changes nothing."""
    from geot_amd.ext import _common
    from geot_amd.openpoints.dataset import ValBatcher, VoteBatcher
    from geot_amd.validation import predict_scans, validate_scans, validate_scans_voted, vote_scans
    from test_val_scans_gpu import _set as scan_set
    dset = scan_set([3000, 777, 1500], 740, cls=[0, 1, 1])
    model = _noisy_model()
    np.random.seed(5)
    batch = ValBatcher(dset, 1024).batch([0, 1])
    logits = model(batch)[0]
    today = predict_scans(logits, batch)
    seen = []
    _common.trace = lambda launch, name: (seen.append(name), launch())[1]
    try:
        off = [predict_scans(logits, batch, refine=r) for r in (0, False, None)]
    finally:
        _common.trace = None
    assert seen == ["geot_scan_predict"] * 3 and all(torch.equal(a, b) for o in off for a, b in zip(o, today))
    voter = VoteBatcher(dset, 1024)
    outs = []
    for kw in ({}, {"refine": 0}):
        np.random.seed(6)
        torch.manual_seed(6)
        outs.append(vote_scans(model, voter, [2, 0], 2, **kw))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    lines = []
    for fn, base in ((validate_scans, {}), (validate_scans_voted, {"vote": []})):
        for cfg_refine, kw in ((False, {}), (True, {}), (True, {"refine": 0}), (True, {"refine": False})):
            cfg = type("Cfg", (), {"num_classes": 17, "num_points": 1024, "epoch": 3, "epochs": 100, "num_votes": 2,
                                   "refine": cfg_refine})()
            np.random.seed(7)
            torch.manual_seed(7)
            caplog.clear()
            seen = []
            _common.trace = lambda launch, name, seen=seen: (seen.append(name), launch())[1]
            try:
                with caplog.at_level(logging.INFO), quiet():
                    out = fn(model, dset, cfg, batch_size=2, **base, **kw)
            finally:
                _common.trace = None
            lines.append((fn.__name__, out, [r.getMessage() for r in caplog.records], [s for s in seen if "refine" in s or "confusion" in s]))
    for name, out, log, extra in lines:
        first = next(l for l in lines if l[0] == name)
        assert len(log) == 3 and log == first[2] and extra == [], (name, log)
        assert all(ref.same_value(a, b) and np.asarray(a).dtype == np.asarray(b).dtype for a, b in zip(out, first[1]))


def test_nothing_synchronises_and_every_refinement_is_one_call():
    from geot_amd.ext import _common
    from geot_amd.openpoints.dataset import ValBatcher
    from geot_amd.validation import SegMetrics, _count_refined, part_seg_refinement, predict_scans, refine_scans
    from test_val_scans_gpu import _set as scan_set
    dset = scan_set([3000, 777, 1500, 64], 760, cls=[0, 1, 1, 0])
    batcher, metrics = ValBatcher(dset, 1024), SegMetrics(17, DEV)
    logits4 = _noisy_model()({"pos": torch.randn(4, 1024, 3, device=DEV)})[0].contiguous()
    dense, pos = torch.randint(0, 17, (3, 500), device=DEV), torch.randn(3, 500, 3, device=DEV)
    warm = batcher.batch([0, 1, 2, 3])
    refine_scans(predict_scans(logits4, warm), warm, 10, PARTS, stats=True)
    _count_refined(metrics, predict_scans(logits4, warm), warm, 10, PARTS)
    part_seg_refinement(dense.clone(), pos, [0, 1, 0], PARTS)
    torch.cuda.synchronize()
    names = {}
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError, match="synchroniz"):
            logits4.sum().item()
        for ids in ([2], [0, 1, 2, 3], [3, 1]):
            batch = batcher.batch(ids)
            logits = logits4[:len(ids)].contiguous()
            seen = []
            _common.trace = lambda launch, name, seen=seen: (seen.append(name), launch())[1]
            try:
                predict_scans(logits, batch, refine=10, parts=PARTS)
                refine_scans(predict_scans(logits, batch), batch, 5, stats=True)
                _count_refined(metrics, predict_scans(logits, batch), batch, 10, PARTS)
                part_seg_refinement(dense.clone(), pos, [0, 1, 0], PARTS)
            finally:
                _common.trace = None
            names[len(ids)] = seen
    finally:
        _common.trace = None
        torch.cuda.set_sync_debug_mode(0)
    expect = ["geot_scan_predict", "geot_scan_refine"] * 3 + ["geot_seg_confusion", "geot_scan_refine"]
    assert names[1] == names[2] == names[4] == expect, names
    assert metrics.read()["scans"] == 4 + 1 + 4 + 2
