"""geot_scan_vote through the C ABI (csrc/scan_predict.hip, include/geot_hip.h): one SET | FINISH call against
geot_scan_predict (exact), the accumulator against the fp64 restatement of tests/_scan_vote_ref.py on the neighbours
geot_three_nn_ws chose (tolerance (16 V + V^2) 2^-24, derived there), the predictions against torch.argmax of the returned
accumulator (exact) and against the fp64 arg-max outside the margin, the counts against torch.bincount, reproducibility,
skipped slots, NaNs and the refusals -- for both forms of the accumulator access (GEOT_VOTE_IMPL=row|tile).  The scans are the
synthetic ones of tests/test_val_scans_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scan_vote_ref as vref  # noqa: E402
import _seg_metrics_ref as ref  # noqa: E402
from test_val_scans_gpu import DEV, _kernel, _known_and_logits, _offsets, _ragged_set, _set  # noqa: E402

pytestmark = pytest.mark.gpu
SET, FINISH = 1, 2
FORMS = ("row", "tile")


def _vote(dset, ids, known, prob, c, acc, mode, counts=None, pred=None, with_labels=True, ids_dev=None, work=None, offs=None,
          ws_bytes=None, acc_given=True, offs_given=True):
    """One geot_scan_vote call through the C ABI."""
    from geot_amd import _lib
    from geot_amd.ext._common import call, ptr
    from geot_amd.validation import scan_work_table
    b, n = known.shape[0], known.shape[1]
    sizes = [dset.sizes[i] for i in ids]
    ids_dev = torch.tensor(ids, dtype=torch.int64, device=DEV) if ids_dev is None else ids_dev
    work = torch.from_numpy(scan_work_table(sizes)).to(DEV) if work is None else work
    offs = _offsets(sizes) if offs is None else offs
    nbytes = int(_lib.load().geot_scan_predict_ws_bytes(b, n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    call("geot_scan_vote", DEV, b, c, n, len(dset), int(dset.points.shape[0]), ptr(dset.points),
         ptr(dset.labels) if with_labels else None, ptr(dset.offsets), ptr(ids_dev), ptr(known), ptr(prob), int(work.shape[0]),
         ptr(work), ptr(offs) if offs_given else None, ptr(acc) if acc_given else None, mode, ptr(pred), ptr(counts), ptr(ws),
         nbytes if ws_bytes is None else ws_bytes)
    torch.cuda.synchronize()


def _neighbours(dset, ids, known):
    """geot_three_nn_ws per slot -> (d2 (total, 3) fp32, idx (total, 3)) as numpy, slot after slot."""
    from geot_amd.ext._common import call, knn_workspace, ptr
    n = known.shape[1]
    sizes = [dset.sizes[i] for i in ids]
    starts = np.concatenate([[0], np.cumsum(dset.sizes)])
    idx = torch.empty((sum(sizes), 3), dtype=torch.int32, device=DEV)
    dist2 = torch.empty((sum(sizes), 3), dtype=torch.float32, device=DEV)
    at = 0
    for s, i in enumerate(ids):
        lo, m = int(starts[i]), sizes[s]
        unknown = dset.points[lo:lo + m].contiguous()
        wp, wb, _keep = knn_workspace(DEV, 1, m, n, 3)
        call("geot_three_nn_ws", DEV, 1, m, n, ptr(unknown), ptr(known[s]), ptr(dist2) + 12 * at, ptr(idx) + 12 * at, wp, wb)
        at += m
    torch.cuda.synchronize()
    return dist2.cpu().numpy(), idx.cpu().numpy()


def _reference(dset, ids, knowns, probs):
    """The fp64 sum of the votes for every vertex of every slot: (total, C)."""
    sizes = [dset.sizes[i] for i in ids]
    ends = np.cumsum(sizes)
    parts = [[] for _ in ids]
    for known, prob in zip(knowns, probs):
        d2, idx = _neighbours(dset, ids, known)
        prob = prob.cpu().numpy()
        for s in range(len(ids)):
            rows = slice(int(ends[s]) - sizes[s], int(ends[s]))
            parts[s].append((prob[s], d2[rows], idx[rows]))
    return np.concatenate([vref.vote_sum(p) for p in parts])


def _labels(dset, ids):
    starts = np.concatenate([[0], np.cumsum(dset.sizes)])
    return torch.cat([dset.labels[int(starts[i]):int(starts[i]) + dset.sizes[i]] for i in ids]).to(torch.int64)


def _bincount(dset, ids, pred, c):
    slots, sizes = c * (c + 1) + 1, [dset.sizes[i] for i in ids]
    return torch.stack([torch.bincount(ref.torch_keys(p, lab, c), minlength=slots)
                        for p, lab in zip(torch.split(pred, sizes), torch.split(_labels(dset, ids), sizes))])


# (C, n, slots, V).  The scans of tests/test_val_scans_gpu.py RAGGED = [1, 63, 64, 65, 100003, 5000, 777] vertices: every C of
# {1, 2, 5, 17, 32}, every n of {1, 2, 3, 8, 2047, 2048} (fewer than three neighbours, both sides of the grid switch), V = 1..4,
# one scan in two slots, scan ids not ascending, and the full-size case last
CASES = [(1, 1, [0], 1), (2, 2, [3, 1], 2), (5, 3, [2, 0, 5], 4), (32, 8, [6, 1, 6, 0], 3), (17, 2047, [5, 3, 2], 2),
         (17, 2048, [5, 0, 1, 5], 3), (32, 2048, [6, 2], 4), (2, 2048, [5], 3), (5, 8, [3], 1), (17, 16000, [4], 2)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("c,n,ids,votes", CASES)
def test_votes(c, n, ids, votes, form, monkeypatch):
    monkeypatch.setenv("GEOT_VOTE_IMPL", form)                # the library reads the variable at every call
    dset = _ragged_set()
    b, slots = len(ids), c * (c + 1) + 1
    sizes = [dset.sizes[i] for i in ids]
    total = sum(sizes)
    knowns, probs = [], []
    for v in range(votes):
        known, logits = _known_and_logits(b, n, c, 77 * c + n + 1000 * v)
        knowns.append(known)
        probs.append(torch.softmax(logits, dim=1).contiguous())

    # 1. one SET | FINISH call is geot_scan_predict: counts only, pred only, both
    want_counts = torch.zeros((b, slots), dtype=torch.int64, device=DEV)
    want_pred = torch.cat(_kernel(dset, ids, knowns[0], probs[0], c, counts=want_counts, want_pred=True))
    for with_counts, with_pred in ((True, False), (False, True), (True, True)):
        acc = torch.full((total, c), float("nan"), device=DEV)          # SET: what is there does not matter
        counts = torch.zeros_like(want_counts) if with_counts else None
        pred = torch.full((total,), -1, dtype=torch.int64, device=DEV) if with_pred else None
        _vote(dset, ids, knowns[0], probs[0], c, acc, SET | FINISH, counts=counts, pred=pred, with_labels=with_counts)
        assert counts is None or torch.equal(counts, want_counts), int((counts - want_counts).abs().sum())
        assert pred is None or torch.equal(pred, want_pred), int((pred != want_pred).sum())
    first = acc.clone()

    # 2. V votes, the last with FINISH; again; and the same votes without FINISH
    def run(finish):
        acc = torch.empty((total, c), device=DEV)
        counts = torch.zeros_like(want_counts) if finish else None
        pred = torch.full((total,), -1, dtype=torch.int64, device=DEV) if finish else None
        for v in range(votes):
            last = finish and v + 1 == votes
            _vote(dset, ids, knowns[v], probs[v], c, acc, (SET if v == 0 else 0) | (FINISH if last else 0),
                  counts=counts if last else None, pred=pred if last else None)
        return acc, pred, counts
    acc, pred, counts = run(True)
    again = run(True)
    plain = run(False)[0]
    assert torch.equal(acc, again[0]) and torch.equal(pred, again[1]) and torch.equal(counts, again[2])
    assert torch.equal(acc, plain)
    assert votes > 1 or torch.equal(acc, first)

    # 3. the accumulator against fp64
    want = _reference(dset, ids, knowns, probs)
    tol = vref.tolerance(votes)
    got = acc.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    err = float(np.nanmax(np.abs(got - want))) if not np.isnan(want).all() else 0.0
    print("C=%d n=%d ids=%s V=%d %s: |acc - fp64| = %.3e (tolerance %.3e)" % (c, n, ids, votes, form, err, tol))
    assert err <= tol, (err, tol)

    # 4. predictions: torch.argmax of the kernel's own sums, exactly; the fp64 arg-max wherever its margin decides
    assert torch.equal(pred, torch.argmax(plain, dim=1))
    decided = vref.decided(want, votes)
    excluded = int((~decided).sum())
    print("  excluded by the margin rule: %d of %d vertices; smallest margin %.3e" %
          (excluded, total, float(np.nanmin(vref.margin(want))) if c > 1 else float("inf")))
    assert excluded <= 0.001 * total, (excluded, total)
    assert np.array_equal(pred.cpu().numpy()[decided], vref.argmax(want)[decided])

    # 5. counts: torch.bincount of (label, pred), every row the scan's vertex count
    assert torch.equal(counts, _bincount(dset, ids, pred, c))
    assert torch.equal(counts.sum(1), torch.tensor(sizes, device=DEV))


@pytest.mark.parametrize("form", FORMS)
def test_a_bad_slot_or_work_entry_is_skipped_and_the_others_are_right(form, monkeypatch):
    """A scan id outside the set and work entries outside their scan: their accumulator rows, predictions and counts stay
    as they were."""
    from geot_amd.validation import scan_work_table
    monkeypatch.setenv("GEOT_VOTE_IMPL", form)
    dset = _ragged_set()
    c, n, ids = 5, 8, [1, 2]
    sizes = [dset.sizes[i] for i in ids]
    known, logits = _known_and_logits(2, n, c, 5)
    prob = torch.softmax(logits, dim=1).contiguous()

    def fresh():
        return (torch.full((sum(sizes), c), -7.0, device=DEV), torch.full((sum(sizes),), -1, dtype=torch.int64, device=DEV),
                torch.zeros((2, c * (c + 1) + 1), dtype=torch.int64, device=DEV))
    acc0, pred0, counts0 = fresh()
    _vote(dset, ids, known, prob, c, acc0, SET | FINISH, counts=counts0, pred=pred0)
    assert int((pred0 < 0).sum()) == 0 and int(counts0.sum()) == sum(sizes)
    table = scan_work_table(sizes)
    extra = np.array([[2, 0, 5, 0], [-1, 0, 5, 0], [0, 63, 5, 0], [0, -1, 5, 0], [1, 0, 0, 0]], dtype=np.int32)   # all unusable
    for bad_ids, tab in (([1, len(dset)], table), ([1, -1], table), (ids, np.concatenate([table, extra]))):
        acc, pred, counts = fresh()
        _vote(dset, ids, known, prob, c, acc, SET | FINISH, counts=counts, pred=pred,
              ids_dev=torch.tensor(bad_ids, dtype=torch.int64, device=DEV), work=torch.from_numpy(np.ascontiguousarray(tab)).to(DEV))
        if bad_ids == ids:
            assert torch.equal(acc, acc0) and torch.equal(pred, pred0) and torch.equal(counts, counts0)
        else:
            m = sizes[0]
            assert torch.equal(acc[:m], acc0[:m]) and torch.equal(pred[:m], pred0[:m]) and torch.equal(counts[0], counts0[0])
            assert bool((acc[m:] == -7.0).all()) and bool((pred[m:] == -1).all()) and int(counts[1].sum()) == 0


@pytest.mark.parametrize("form", FORMS)
def test_nan_probabilities_and_a_nan_vertex_follow_the_first_nan_rule_through_the_sum(form, monkeypatch):
    from test_val_scans_gpu import _scan
    from geot_amd.openpoints.dataset import DeviceScanSet
    monkeypatch.setenv("GEOT_VOTE_IMPL", form)
    c, n, votes = 5, 8, 3
    pts, lab = _scan(777, 41, c)
    pts[100] = np.array([np.nan, 1.0, 2.0], np.float32)
    dset = DeviceScanSet([pts, _scan(65, 42, c)[0]], [lab, _scan(65, 42, c)[1]], device=DEV)
    ids, sizes = [0, 1], [777, 65]
    knowns, probs = [], []
    for v in range(votes):
        known, logits = _known_and_logits(2, n, c, 900 + v)
        prob = torch.softmax(logits, dim=1).contiguous()
        if v == 1:                                     # the middle vote: NaN in class 3 at two sampled points, class 1 at one
            prob[0, 3, 2] = prob[0, 3, 5] = prob[0, 1, 5] = float("nan")
        knowns.append(known)
        probs.append(prob)
    acc = torch.empty((sum(sizes), c), device=DEV)
    pred = torch.full((sum(sizes),), -1, dtype=torch.int64, device=DEV)
    counts = torch.zeros((2, c * (c + 1) + 1), dtype=torch.int64, device=DEV)
    for v in range(votes):
        last = v + 1 == votes
        _vote(dset, ids, knowns[v], probs[v], c, acc, (SET if v == 0 else 0) | (FINISH if last else 0),
              counts=counts if last else None, pred=pred if last else None)
    want = _reference(dset, ids, knowns, probs)
    got = acc.cpu().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert nan[100].all() and int(pred[100]) == 0                     # the NaN vertex: 0 / 0 weights, class 0 is the first NaN
    assert nan[:777, 3].sum() > 1 and nan[:777, 1].sum() >= 1 and not nan[777:].any() and not nan[:, [0, 2, 4]][np.arange(len(nan)) != 100].any()
    rows = nan.any(1)
    assert np.array_equal(pred.cpu().numpy()[rows], nan[rows].argmax(1))     # the first NaN wins, whatever the other sums
    assert torch.equal(pred, torch.argmax(acc, dim=1))
    assert float(np.nanmax(np.abs(got.astype(np.float64) - want))) <= vref.tolerance(votes)
    assert torch.equal(counts, _bincount(dset, ids, pred, c))


def test_refusals():
    from geot_amd.validation import scan_work_table
    dset = _set([3000, 64], 950, cls=[0, 1])
    c, n, ids = 17, 2048, [0, 1]
    known, logits = _known_and_logits(2, n, c, 3)
    prob = torch.softmax(logits, dim=1).contiguous()
    acc = torch.full((3064, c), -7.0, device=DEV)
    pred = torch.full((3064,), -1, dtype=torch.int64, device=DEV)
    counts = torch.zeros((2, c * (c + 1) + 1), dtype=torch.int64, device=DEV)
    for kw in (dict(mode=SET, pred=pred), dict(mode=0, counts=counts), dict(mode=SET, pred=pred, counts=counts),     # no FINISH
               dict(mode=SET | FINISH, counts=counts, with_labels=False), dict(mode=SET, acc_given=False),
               dict(mode=SET | FINISH, pred=pred, offs_given=False), dict(mode=SET, offs_given=False), dict(mode=SET, ws_bytes=16),
               dict(mode=4), dict(mode=SET | FINISH | 8, pred=pred)):
        mode = kw.pop("mode")
        with pytest.raises(RuntimeError, match="hipError 1"):
            _vote(dset, ids, known, prob, c, acc, mode, **kw)
    torch.cuda.synchronize()
    assert bool((acc == -7.0).all()) and bool((pred == -1).all()) and int(counts.sum()) == 0
    _vote(dset, ids, known, prob, c, acc, SET | FINISH)               # FINISH with nobody reading the arg-max: the sums alone
    _vote(dset, ids, known, prob, c, acc, FINISH, pred=pred, counts=counts)
    assert int(counts.sum()) == 3064 and torch.equal(pred, torch.argmax(acc, dim=1))
    work = torch.from_numpy(scan_work_table(dset.sizes)).to(DEV)
    _vote(dset, ids, known, prob, c, acc, SET, work=work[:0])         # no work: nothing to do
