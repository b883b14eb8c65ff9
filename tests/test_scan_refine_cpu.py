"""Refining whole-scan predictions, the part that needs no GPU: the ABI and the binding of geot_scan_refine, the refusals that
come before any device call, and the numpy restatement the GPU tests compare against (tests/_scan_refine_ref.py) against the
reference-executed fixture (tests/golden/part_seg_refinement_ref.npz, every vertex), a plain loop and hand-checked cases."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scan_refine_ref as rref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "part_seg_refinement_ref.npz")
EXACT_MEMBERS = [1, 3, 7, 9, 10, 12]      # scan 0 of the fixture, classes 4, 5, 6, 7, 8, 12: below n, n - 1, exactly n = 10, not allowed


def test_abi_version_and_signature():
    import ctypes
    from geot_amd import _lib, build, validation
    build.build()
    hdr = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    assert int(re.search(r"GEOT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 22
    lib = _lib.load()
    assert lib.geot_abi_version() == _lib.ABI_VERSION
    decl = re.search(r"int geot_scan_refine\(([^;]*)\);", hdr).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args[:5] == ["int b", "int c", "int n", "int n_scans", "long long total"] and args[-1] == "void *stream"
    assert args[9:12] == ["const unsigned *allowed", "long long *pred", "int *stats"] and len(args) == 15
    proto = _lib.PROTOTYPES["geot_scan_refine"]
    assert len(proto) == len(args)
    for a, t in zip(args, proto):
        want = ctypes.c_void_p if "*" in a else ctypes.c_longlong if a.startswith("long long") else ctypes.c_int
        assert t is want, (a, t)
    assert lib.geot_scan_refine.argtypes == proto
    assert re.search(r"long long geot_scan_refine_ws_bytes\(int b, long long total_out, int n\);", hdr)
    assert _lib.PLAIN["geot_scan_refine_ws_bytes"] == ([ctypes.c_int, ctypes.c_longlong, ctypes.c_int], ctypes.c_longlong)
    for name in ("refine_scans", "part_seg_refinement", "validate_scans_voted"):
        assert callable(getattr(validation, name))
    assert validation.REFINE_MAX_N == 63


def test_workspace_size_and_entry_point_refusals_need_no_device():
    from geot_amd import _lib
    lib = _lib.load()
    ws = lib.geot_scan_refine_ws_bytes
    head = ws(2, 0, 10)
    assert head > 0 and head % 16 == 0
    assert ws(2, 1000, 10) - head == 1000 * 4 * 12                     # a query list and n + 1 neighbours per vertex
    assert ws(0, 0, 1) == 0 and ws(65535, 10, 63) > 0
    for b, total, n in ((-1, 10, 10), (65536, 10, 10), (2, -1, 10), (2, 10, 0), (2, 10, 64)):
        assert ws(b, total, n) == -1, (b, total, n)
    # hipErrorInvalidValue (1) before any launch: the pointers are never followed
    fake = 1 << 20
    good = dict(b=2, c=17, n=10, n_scans=3, total=100, points=fake, offsets=fake, scan_ids=fake, out_offsets=fake, allowed=None,
                pred=fake, stats=None, ws=fake, ws_bytes=head)
    for change in (dict(c=0), dict(c=33), dict(n=0), dict(n=64), dict(b=-1), dict(b=65536), dict(n_scans=0), dict(total=0),
                   dict(points=None), dict(offsets=None), dict(scan_ids=None), dict(out_offsets=None), dict(pred=None),
                   dict(ws=None), dict(ws=fake + 4), dict(ws_bytes=head - 16)):
        a = dict(good, **change)
        assert lib.geot_scan_refine(*a.values(), None) == 1, change
    assert lib.geot_scan_refine(*dict(good, b=0, ws_bytes=0).values(), None) == 0      # nothing to do


def test_python_refusals_come_before_any_device_call():
    import torch
    from geot_amd.validation import part_seg_refinement, predict_scans, refine_scans, validate_scans, vote_scans
    batch = {"scans": None, "sizes": [20, 30], "scan_ids": None, "mandible": [True, False]}
    preds = [torch.zeros(1, 20, dtype=torch.int64), torch.zeros(1, 30, dtype=torch.int64)]
    for n in (0, 64, -1, 2.5, True):
        with pytest.raises(RuntimeError, match="n must be an int in 1..63"):
            refine_scans(preds, batch, n)
    with pytest.raises(RuntimeError, match="no 21 nearest vertices"):
        refine_scans(preds, batch, 20)
    with pytest.raises(RuntimeError, match="int64"):
        refine_scans([p.int() for p in preds], batch, 5)
    with pytest.raises(RuntimeError, match="one prediction tensor per scan"):
        refine_scans(preds[:1], batch, 5)
    with pytest.raises(RuntimeError, match="30 predictions for a scan of 20"):
        refine_scans(preds[::-1], batch, 5)
    with pytest.raises(RuntimeError, match="1..32 classes"):
        refine_scans(preds, batch, 5, parts=[[0, 1], [0, 40]])
    with pytest.raises(RuntimeError, match=r"labels in \[0, 4\)"):
        refine_scans(preds, batch, 5, parts=[[0, 7], [0, 3]])

    class OnGpu:
        device = torch.device("cuda", 0)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        refine_scans(preds, dict(batch, scans=OnGpu()), 5)
    pred, pos = torch.zeros(2, 12, dtype=torch.int64), torch.zeros(2, 12, 3)
    parts = [[0, 1], [0, 2, 3]]
    for n in (0, 64):
        with pytest.raises(RuntimeError, match="n must be an int in 1..63"):
            part_seg_refinement(pred, pos, [0, 1], parts, n)
    with pytest.raises(RuntimeError, match="no 13 nearest points"):
        part_seg_refinement(pred, pos, [0, 1], parts, 12)
    with pytest.raises(RuntimeError, match=r"\(B, N\) int64"):
        part_seg_refinement(pred.int(), pos, [0, 1], parts, 5)
    with pytest.raises(RuntimeError, match=r"\(B, N, 3\) fp32"):
        part_seg_refinement(pred, pos.double(), [0, 1], parts, 5)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        part_seg_refinement(pred, pos, [0, 1], parts, 5)

    class Never:
        def eval(self):
            raise AssertionError("called")
    for bad in (64, -1, "yes", 2.0):
        with pytest.raises(RuntimeError, match="refine"):
            predict_scans(None, None, refine=bad)
        with pytest.raises(RuntimeError, match="refine"):
            vote_scans(Never(), None, [0], 3, refine=bad)
        with pytest.raises(RuntimeError, match="refine"):
            validate_scans(Never(), None, {}, refine=bad)


def test_the_restatement_equals_the_reference_fixture_on_every_vertex():
    fx = np.load(FIXTURE)
    meta = str(fx["meta"])
    assert "cpu() returns a clone" in meta and "no query excluded" in meta and "seed %d" % int(fx["seed"]) in meta
    assert float(fx["min_gap_ulp"]) >= 32.0
    pos, pred, out, n = fx["pos"], fx["pred"].astype(np.int64), fx["out"].astype(np.int64), int(fx["n"])
    parts, cls = fx["cls2parts"].tolist(), fx["cls"].tolist()
    c = parts[-1][-1] + 1
    assert pos.dtype == np.float32 and float(np.sqrt((pos.astype(np.float64) ** 2).sum(-1)).max()) <= 1.01
    got, stats = rref.refine_scans(list(pred), list(pos), c, n, [parts[j] for j in cls])
    assert np.array_equal(np.stack(got), out)
    assert np.array_equal(stats, fx["stats"]) and int(stats[:, 1].sum()) >= 100 and int(stats[:, 2].sum()) == int((out != pred).sum())
    # what the inputs hold: classes of 1, 3, 7, 9 and 10 members, a disallowed class, two classes, one class
    members = {int(l): int((pred[0] == l).sum()) for l in np.unique(pred[0])}
    print("scan 0 members per class:", members)
    assert [members[l] for l in (4, 5, 6, 7, 8, 12)] == EXACT_MEMBERS
    assert (out[0] == 8).sum() >= 1 and not (out[0] == 12).any()        # exactly n members: kept; not allowed: gone
    assert len(np.unique(pred[2])) == 2 and len(np.unique(pred[3])) == 1 and np.array_equal(out[3], pred[3])
    assert not (out[1][pred[1] == 3] == 3).any() and (out[1] == 0).any()    # the big disallowed class: inner vertices vote all-zero
    # the aliasing form (a plain CPU tensor) gives other labels, and the restatement knows both
    alias = [rref.refine_scan(p, x, c, n, parts[j], alias=True)[0] for p, x, j in zip(pred, pos, cls)]
    assert np.array_equal(np.stack(alias), fx["aliased"].astype(np.int64)) and not np.array_equal(fx["aliased"], fx["out"])


def _loop(pred, pts, c, n, allowed):
    """The rules one statement at a time, python lists and fp32 scalars."""
    m = len(pred)
    snap, cur = [int(p) for p in pred], [int(p) for p in pred]
    order = []
    for v in range(m):
        if 0 <= snap[v] < c and snap[v] not in order:
            order.append(snap[v])
    if len(order) < 2:
        return cur
    for i in order:
        if not (snap.count(i) < n or (allowed is not None and i not in allowed)):
            continue
        staged = {}
        for v in range(m):
            if snap[v] != i:
                continue
            cand = []
            for j in range(m):
                dx, dy, dz = (np.float32(pts[v][a]) - np.float32(pts[j][a]) for a in range(3))
                d2 = np.float32(np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(dz * dz))
                if d2 < np.inf:
                    cand.append((d2, j))
            votes = [0] * c
            for _, j in sorted(cand)[:n + 1]:
                if 0 <= cur[j] < c:
                    votes[cur[j]] += 1
            votes[i] = 0
            staged[v] = votes.index(max(votes))
        for v, new in staged.items():
            cur[v] = new
    return cur


@pytest.mark.parametrize("seed,m,c,n", [(0, 40, 5, 3), (1, 64, 17, 10), (2, 30, 3, 1), (3, 50, 8, 6)])
def test_the_restatement_equals_a_plain_loop(seed, m, c, n):
    rng = np.random.default_rng(seed)
    pts = rng.normal(size=(m, 3)).astype(np.float32)
    pts[7] = pts[3]                                                     # an exact tie, decided by index
    pts[11] = pts[3]
    pred = rng.integers(0, c, m)
    pred[rng.integers(0, m, 3)] = c + 2                                 # outside [0, c): untouched, never votes
    pred[5] = -1
    allowed = sorted(set(range(c)) - {int(pred[0])})
    for ok in (None, allowed):
        got, stats = rref.refine_scan(pred, pts, c, n, ok)
        want = _loop(pred, pts, c, n, ok)
        assert got.tolist() == want
        assert stats[3] == int(((pred < 0) | (pred >= c)).sum()) and stats[2] == int((got != pred).sum())
        assert np.array_equal(got[(pred < 0) | (pred >= c)], pred[(pred < 0) | (pred >= c)])


LINE = np.array([[float(x), 0.0, 0.0] for x in (0, 1, 2, 3, 10, 11, 12, 13)], np.float32)


def test_snapshot_rule_differs_from_the_aliasing_form():
    # n = 2, three nearest.  Class 1 = {v1}, class 2 = {v2}, both small, 1 first.  Step 1: v1 sees (v1, v0, v2) = labels
    # (1, 0, 2) -> class 1 zeroed, tie 0 / 2 -> 0.  Step 2, snapshot: v2 sees (v2, v1, v3) = (2, 0 now, 0) -> 0.
    pred = np.array([0, 1, 2, 0, 0, 0, 0, 0])
    got, stats = rref.refine_scan(pred, LINE, 3, 2)
    assert got.tolist() == [0] * 8 and stats == [2, 2, 2, 0]
    # Class 2 = {v1}, class 1 = {v2, v5}: v1 -> (2, 0, 1): tie 0 / 1 -> 0.  With class 1 first instead (below) the same.  The
    # aliasing form differs when a step relabels INTO a later small class: 1 = {v1}, 2 = {v2}, 0 absent near them.
    pred = np.array([2, 1, 2, 3, 3, 3, 3, 3])                           # counts: 2 -> 2 (< 3), 1 -> 1, 3 -> 5
    snap, _ = rref.refine_scan(pred, LINE, 4, 3)
    alias, _ = rref.refine_scan(pred, LINE, 4, 3, alias=True)
    # snapshot.  order 2, 1 (3 is large).  Step 2: queries v0, v2 (four nearest).  v0: (v0, v1, v2, v3) = (2, 1, 2, 3) -> 2 zeroed,
    # 1 and 3 tie -> 1.  v2: (v2, v1, v3, v0) = (2, 1, 3, 2) -> 1.  Step 1: the only query is v1 (snap): (v1, v0, v2, v3) = (1, 1, 1, 3)
    # now -> 1 zeroed -> 3.
    assert snap.tolist() == [1, 3, 1, 3, 3, 3, 3, 3]
    # aliasing: step 1's queries are everything labelled 1 NOW: v0, v1, v2 -> all see (1, 1, 1, 3) -> 3.
    assert alias.tolist() == [3, 3, 3, 3, 3, 3, 3, 3]


def test_first_occurrence_order_changes_the_result():
    # classes 1 = {v1} and 2 = {v2}, n = 2 (three nearest), the rest 0 / 3.  v1 sees (v1, v0, v2), v2 sees (v2, v1, v3).
    a = np.array([3, 1, 2, 3, 3, 3, 3, 3])          # order 3, 1, 2: v1 -> (1, 3, 2): 2 and 3 tie -> 2; then v2 -> (2, 2, 3): zeroed -> 3
    b = np.array([3, 2, 1, 3, 3, 3, 3, 3])          # order 3, 2, 1: v1 -> (2, 3, 1): 1 and 3 tie -> 1; then v2 -> (1, 1, 3): zeroed -> 3
    assert rref.refine_scan(a, LINE, 4, 2)[0].tolist() == [3, 2, 3, 3, 3, 3, 3, 3]
    assert rref.refine_scan(b, LINE, 4, 2)[0].tolist() == [3, 1, 3, 3, 3, 3, 3, 3]
    # the same labels with the other class first in the scan: vertex 0 decides the order, not the class id
    c = np.array([2, 1, 2, 3, 3, 3, 3, 3])          # order 2, 1 -- worked in the snapshot test: [1, 3, 1, ...]
    d = np.array([1, 2, 1, 3, 3, 3, 3, 3])          # order 1, 2 by symmetry: [2, 3, 2, ...]
    assert rref.refine_scan(c, LINE, 4, 3)[0].tolist() == [1, 3, 1, 3, 3, 3, 3, 3]
    assert rref.refine_scan(d, LINE, 4, 3)[0].tolist() == [2, 3, 2, 3, 3, 3, 3, 3]
    # the same scan with vertices 1 and 2 stored in the other order (coordinates and labels swapped together): the geometry and
    # every vertex's label are unchanged, only class 2 now occurs first.  Step 2: the vertex at x = 2 sees (2, 1, 3): 1 and 3 tie
    # -> 1; step 1: the vertex at x = 1 sees (1, 3, 1 now): zeroed -> 3.  In storage order a gave x = 1 -> 2, x = 2 -> 3.
    pts = LINE.copy()
    pts[[1, 2]] = pts[[2, 1]]
    f = np.array([3, 2, 1, 3, 3, 3, 3, 3])          # vertex 1 lies at x = 2 (class 2), vertex 2 at x = 1 (class 1)
    assert rref.refine_scan(f, pts, 4, 2)[0].tolist() == [3, 1, 3, 3, 3, 3, 3, 3]      # x = 2 -> 1, x = 1 -> 3


def test_an_equal_vote_goes_to_the_lower_class_and_an_all_zero_vote_gives_0():
    pred = np.array([3, 1, 2, 2, 3, 3, 3, 3])       # n = 3 (four nearest): v1 sees (v1, v0, v2, v3) = (1, 3, 2, 2) -> 2
    assert rref.refine_scan(pred, LINE, 4, 3)[0][1] == 2
    pred = np.array([3, 1, 2, 3, 3, 3, 3, 3])       # n = 2: v1 sees (1, 3, 2): 2 and 3 have one vote each -> the lower, 2
    assert rref.refine_scan(pred, LINE, 4, 2)[0][1] == 2
    # all zero: class 2 is not allowed and fills the left group, whose four nearest are all class 2 -> zeroed -> class 0,
    # although no vertex of the scan is labelled 0
    pred = np.array([2, 2, 2, 2, 1, 1, 1, 1])
    got, stats = rref.refine_scan(pred, LINE, 3, 3, allowed=[0, 1])
    assert got.tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and stats == [1, 4, 4, 0]
    # one class present: untouched even when it is not allowed
    assert rref.refine_scan(np.full(8, 2), LINE, 3, 3, allowed=[0, 1])[0].tolist() == [2] * 8
    # exactly n members: kept; n - 1: refined
    pred = np.array([1, 1, 1, 0, 0, 0, 0, 0])
    assert rref.refine_scan(pred, LINE, 2, 3)[0].tolist() == pred.tolist()
    assert rref.refine_scan(pred, LINE, 2, 4)[0].tolist() == [0] * 8
