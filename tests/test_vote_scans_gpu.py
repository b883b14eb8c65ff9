"""Voting end to end (geot_amd/validation.py ScanVotes, vote_scans, validate_scans_voted): one vote with an empty vote list
is validate_scans (exact), three votes of the stand-in model against the torch composite made of get_pred_whole's statements
(three_interpolate summed over the passes, then arg-max) and against the fp64 reference, outside the margin rule of
tests/_scan_vote_ref.py; nothing synchronises with the host."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scan_vote_ref as vref  # noqa: E402
import _seg_metrics_ref as ref  # noqa: E402
from _seg_metrics_ref import quiet  # noqa: E402
from test_scan_vote_gpu import _reference  # noqa: E402
from test_seg_metrics_gpu import _SeededLogits  # noqa: E402
from test_val_scans_gpu import DEV, _set  # noqa: E402

pytestmark = pytest.mark.gpu


class _Recorder:
    """Wraps a model; keeps every batch it saw and the logits it returned, in call order."""

    def __init__(self, model):
        self.model, self.seen = model, []

    def eval(self):
        self.model.eval()
        return self

    def __call__(self, data):
        out = self.model(data)
        self.seen.append((data, out[0].clone()))
        return out


def test_one_vote_with_an_empty_list_is_validate_scans():
    from geot_amd.validation import validate_scans, validate_scans_voted
    dset = _set([30011, 20000, 1500, 25000, 9000], 800, cls=[0, 1, 1, 1, 0])      # mixed jaws, 1500 < num_points, a short last batch
    cfg = type("Cfg", (), {"num_classes": 17, "num_points": 8000, "epoch": 3, "epochs": 100, "num_votes": 1,
                           "datatransforms": {"vote": [], "kwargs": {"gravity_dim": 1, "scale": [0.9, 1.1]}}})()
    with quiet():
        np.random.seed(99)
        want = validate_scans(_SeededLogits(), dset, cfg, batch_size=2)
        np.random.seed(99)
        got = validate_scans_voted(_SeededLogits(), dset, cfg, batch_size=2)          # num_votes and vote from cfg
        np.random.seed(99)
        side = validate_scans_voted(_SeededLogits(), dset, cfg, num_votes=1, vote=[], batch_size=2, stream=torch.cuda.Stream(DEV))
        np.random.seed(99)
        shard = validate_scans_voted(_SeededLogits(), dset, cfg, batch_size=2, indices=[4, 2, 1])
        np.random.seed(99)
        shard_want = validate_scans(_SeededLogits(), dset, cfg, batch_size=2, indices=[4, 2, 1])
    for g, s, w, k in zip(got, side, want, ("whole_macc", "whole_miou", "whole_mdsc")):
        print("validate_scans_voted %s: %r (validate_scans %r, side stream %r)" % (k, g, w, s))
        assert np.asarray(g).dtype == np.asarray(w).dtype == np.asarray(s).dtype, k
        assert ref.same_value(g, w) and ref.same_value(s, w) and np.isfinite(float(g)), (k, g, s, w)
    assert all(ref.same_value(a, b) for a, b in zip(shard, shard_want))


def test_votes_change_the_passes_and_the_configured_defaults_apply():
    """cfg.num_votes passes per batch, each on another sample under another scale; the scores stay those of a sensible model."""
    from geot_amd.validation import validate_scans_voted
    dset = _set([30011, 20000, 9000], 830, cls=[0, 1, 0])
    cfg = type("Cfg", (), {"num_classes": 17, "num_points": 4096, "epoch": 0, "epochs": 1, "num_votes": 3})()
    rec = _Recorder(_SeededLogits())
    np.random.seed(5)
    torch.manual_seed(5)
    with quiet():
        out = validate_scans_voted(rec, dset, cfg, batch_size=2)
    assert len(rec.seen) == 2 * 3 and all(np.isfinite(float(v)) for v in out)
    first, second, third = (rec.seen[k][0] for k in range(3))
    assert torch.equal(first["scan_ids"], second["scan_ids"]) and torch.equal(first["scan_ids"], third["scan_ids"])
    assert not torch.equal(first["pos_search"], second["pos_search"]) and not torch.equal(first["pos"], first["pos_search"])
    assert rec.seen[3][0]["sizes"] == [9000] and rec.seen[5][0]["sizes"] == [9000]


def test_vote_scans_equals_the_torch_composite_and_the_fp64_reference():
    from geot_amd.openpoints.dataset import VoteBatcher
    from geot_amd.pointnet2 import pointnet2_utils as pt_utils
    from geot_amd.validation import vote_scans
    sizes, idx, votes, n = [30011, 777, 20000], [2, 0, 1], 3, 4096
    dset = _set(sizes, 860, cls=[0, 1, 1])
    batcher = VoteBatcher(dset, n, stream=torch.cuda.Stream(DEV))
    rec = _Recorder(_SeededLogits())
    np.random.seed(17)
    torch.manual_seed(17)
    preds = vote_scans(rec, batcher, idx, votes)
    torch.cuda.synchronize()
    assert len(rec.seen) == votes and len(preds) == 3
    assert [tuple(p.shape) for p in preds] == [(1, sizes[i]) for i in idx] and all(p.dtype == torch.int64 for p in preds)
    # the composite: get_pred_whole's statements per pass, three_interpolate's outputs summed, one arg-max
    sums = [None] * len(idx)
    knowns, probs = [], []
    for data, logits in rec.seen:
        prob = torch.softmax(logits, dim=1)
        known = []
        for s in range(len(idx)):
            logit = prob[s].unsqueeze(0).contiguous()
            point = data["pos_search"][s].unsqueeze(0).contiguous()
            sc, ce = data["scale"][s].unsqueeze(0).contiguous(), data["center"][s].unsqueeze(0).contiguous()
            point = (point * sc + ce).contiguous()
            dist, nn = pt_utils.three_nn(data["points"][s].unsqueeze(0).float(), point.float())
            dist_recip = 1.0 / (dist + 1e-8)
            weight = dist_recip / torch.sum(dist_recip, dim=2, keepdim=True)
            whole = pt_utils.three_interpolate(logit, nn, weight)
            sums[s] = whole if sums[s] is None else sums[s] + whole
            known.append(point[0])
        knowns.append(torch.stack(known))
        probs.append(prob.contiguous())
    want64 = _reference(dset, idx, knowns, probs)
    decided = vref.decided(want64, votes)
    excluded = int((~decided).sum())
    print("excluded by the margin rule: %d of %d vertices" % (excluded, len(decided)))
    assert excluded <= 0.001 * len(decided)
    got = torch.cat([p.reshape(-1) for p in preds]).cpu().numpy()
    composite = torch.cat([s.argmax(dim=1).reshape(-1) for s in sums]).cpu().numpy()
    print("vote_scans differs from the composite at %d vertices, %d of them decided" %
          (int((got != composite).sum()), int((got != composite)[decided].sum())))
    assert np.array_equal(got[decided], composite[decided])
    assert np.array_equal(got[decided], vref.argmax(want64)[decided])


def test_scan_votes_probabilities_and_refusals():
    from geot_amd.openpoints.dataset import ValBatcher, VoteBatcher
    from geot_amd.validation import ScanVotes, predict_scans
    dset = _set([3000, 64], 950, cls=[0, 1])
    batcher = VoteBatcher(dset, 2048)
    np.random.seed(2)
    torch.manual_seed(2)
    one, two = batcher.batch([0, 1]), batcher.batch([0, 1])
    logits = torch.randn(2, 17, 2048, device=DEV)
    votes = ScanVotes(one, 17)
    with pytest.raises(RuntimeError, match="no vote yet"):
        votes.probabilities()
    with pytest.raises(RuntimeError, match="last vote"):
        votes.add(logits, one, want_pred=True)
    assert votes.add(logits, one) is None
    p1 = [p.clone() for p in votes.probabilities()]
    preds = votes.add(logits, two, last=True, want_pred=True)
    p2 = votes.probabilities()
    torch.cuda.synchronize()
    assert [tuple(p.shape) for p in p2] == [(3000, 17), (64, 17)] and votes.votes == 2
    assert all(float((p.sum(1) - 1).abs().max()) <= 1e-5 for p in p1 + p2)
    assert all(torch.equal(pr.reshape(-1), p.argmax(1)) for pr, p in zip(preds, torch.split(votes.acc, [3000, 64])))
    with pytest.raises(RuntimeError, match="last vote has been added"):
        votes.add(logits, one)
    # a plain ValBatcher batch votes too: pos is what is searched; one vote of it is predict_scans
    plain = ValBatcher(dset, 2048).batch([0, 1])
    single = ScanVotes(plain, 17).add(logits, plain, last=True, want_pred=True)
    assert all(torch.equal(a, b) for a, b in zip(single, predict_scans(logits, plain)))
    for bad, msg in ((logits.cpu(), "CPU not supported"), (logits[:, :16].contiguous(), "fp32 logits"), (logits[:1].contiguous(), "logits rows")):
        with pytest.raises(RuntimeError, match=msg):
            ScanVotes(one, 17).add(bad, one)
    with pytest.raises(RuntimeError, match="same scans"):
        ScanVotes(one, 17).add(logits[:1].contiguous(), batcher.batch([1]))
    with pytest.raises(RuntimeError, match="1..32 classes"):
        ScanVotes(one, 33)


def test_nothing_synchronises_and_every_vote_is_one_call():
    from geot_amd.ext import _common
    from geot_amd.openpoints.dataset import DeviceDraws, VoteBatcher
    from geot_amd.validation import ScanVotes, SegMetrics, vote_scans
    dset = _set([20000, 9999, 3000, 64], 900, cls=[0, 1, 0, 1])
    batcher = VoteBatcher(dset, 4096)
    drawn = VoteBatcher(dset, 4096, stream=torch.cuda.Stream(DEV), draws=DeviceDraws(3, views=True))
    metrics = SegMetrics(17, DEV)
    logits4 = torch.randn(4, 17, 4096, device=DEV)
    model = _SeededLogits()
    for b in (batcher, drawn):                                  # warm: kernels, layouts, workspace, pinned pool
        warm = b.batch([0, 1, 2, 3])
        b.join(warm)
        votes = ScanVotes(warm, 17)
        votes.add(logits4, warm)
        votes.add(logits4, warm, last=True, counts=metrics._rows(4), want_pred=True)
        votes.probabilities()
        vote_scans(model, b, [1, 3], 2)
        b.batch([2])                                            # (a batch shape's draw layout is copied to the device once)
    torch.cuda.synchronize()
    names = {}
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError, match="synchroniz"):
            logits4.sum().item()
        for b in (batcher, drawn):
            for ids in ([2], [0, 1, 2, 3], [3, 1]):
                logits = logits4[:len(ids)].contiguous()
                seen = []
                _common.trace = lambda launch, name, seen=seen: (seen.append(name), launch())[1]
                try:
                    first = b.batch(ids)
                    del seen[:]
                    b.join(first)
                    votes = ScanVotes(first, 17)
                    votes.add(logits, first)
                    votes.add(logits, first, last=True, counts=metrics._rows(len(ids)), want_pred=True)
                finally:
                    _common.trace = None
                names.setdefault(len(ids), seen)
                votes.probabilities()
                vote_scans(model, b, ids, 3)
    finally:
        _common.trace = None
        torch.cuda.set_sync_debug_mode(0)
    assert names[1] == names[4] == ["geot_scan_vote", "geot_scan_vote"], names


def _logged(cls, events, *args, **kwargs):
    """A ValBatcher / VoteBatcher that writes its batch() and join() calls into `events`, then does what it always does."""
    class Logged(cls):
        def batch(self, idx, *a, **kw):
            events.append(("batch", [int(i) for i in idx]))
            out = super().batch(idx, *a, **kw)
            out["_ids"] = [int(i) for i in idx]
            return out

        def join(self, data):
            events.append(("join", data["_ids"]))
            return super().join(data)
    return Logged(*args, **kwargs)


class _LoggedRecorder(_Recorder):
    def __init__(self, model, events):
        super().__init__(model)
        self.events = events

    def __call__(self, data):
        self.events.append(("model", data["_ids"]))
        return super().__call__(data)


def test_the_look_ahead_order_of_every_public_pass_loop():
    """join, queue the next batch, run the model: the same sequence from validate_scans, validate_scans_voted and vote_scans,
    with and without refine; the voted triple equals a replay of the recorded passes through ScanVotes and
    SegMetrics.update_from_votes."""
    from geot_amd.openpoints.dataset import ValBatcher, VoteBatcher
    from geot_amd.validation import ScanVotes, SegMetrics, validate_scans, validate_scans_voted, vote_scans
    from test_scan_refine_gpu import PARTS
    from test_val_passes_cpu import look_ahead_events
    dset = _set([3000, 777, 1500], 880, cls=[0, 1, 1])
    cfg = type("Cfg", (), {"num_classes": 17, "num_points": 1024, "epoch": 3, "epochs": 100})()
    groups = [[0, 1], [2]]

    def run(kind, fn):
        events = []
        batcher = _logged(ValBatcher if kind == "val" else VoteBatcher, events, dset, 1024)
        rec = _LoggedRecorder(_SeededLogits(), events)
        np.random.seed(21)
        torch.manual_seed(21)
        with quiet():
            out = fn(rec, batcher)
        return events, out, rec

    for refine in ({}, {"refine": 10, "parts": PARTS}):
        events, out, _ = run("val", lambda rec, b: validate_scans(rec, b, cfg, batch_size=2, **refine))
        assert events == look_ahead_events(groups, 1), (refine, events)
        assert all(np.isfinite(float(v)) for v in out)
        events, out, rec = run("vote", lambda rec, b: validate_scans_voted(rec, b, cfg, num_votes=2, batch_size=2, **refine))
        assert events == look_ahead_events(groups, 2), (refine, events)
        assert events[:6] == [("batch", [0, 1]), ("join", [0, 1]), ("batch", [0, 1]), ("model", [0, 1]), ("join", [0, 1]), ("batch", [2])]
        assert all(np.isfinite(float(v)) for v in out)
        if not refine:
            voted, seen = out, rec.seen
    events, preds, _ = run("vote", lambda rec, b: vote_scans(rec, b, [1, 2], 3))
    assert events == look_ahead_events([[1, 2]], 3), events
    assert [tuple(p.shape) for p in preds] == [(1, 777), (1, 1500)]
    # the voted scores, replayed from the passes the model saw
    metrics = SegMetrics(17, DEV)
    assert len(seen) == 4
    for k in (0, 2):
        votes = ScanVotes(seen[k][0], 17)
        votes.add(seen[k][1], seen[k][0])
        metrics.update_from_votes(votes, seen[k + 1][1], seen[k + 1][0])
    assert metrics.scans == 3 and metrics.mandible == [True, False, False]
    with quiet():
        want = metrics.read()
    for g, key in zip(voted, ("whole_macc", "whole_miou", "whole_mdsc")):
        print("validate_scans_voted %s: %r (replayed %r)" % (key, g, want[key]))
        assert np.asarray(g).dtype == np.asarray(want[key]).dtype and ref.same_value(g, want[key]), (key, g, want[key])
