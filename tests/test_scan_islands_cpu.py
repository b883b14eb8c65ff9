"""Connected pieces of whole-scan labels, the part that needs no GPU: the ABI and the binding of geot_scan_islands, its
workspace sizes, the refusals that come before any device call (C and Python), teeth3ds_result on hand-made arrays of both
jaws, and the numpy restatement the GPU tests compare against (tests/_scan_islands_ref.py) on graphs checked by hand."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scan_islands_ref as iref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_version_signature_and_exports():
    import geot_amd
    from geot_amd import _lib, build, validation
    build.build()
    hdr = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    assert int(re.search(r"GEOT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 34
    lib = _lib.load()
    assert lib.geot_abi_version() == _lib.ABI_VERSION
    decl = re.search(r"int geot_scan_islands\(([^;]*)\);", hdr).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["int b", "int c", "int k", "int min_size", "int n_scans", "long long total", "const long long *offsets",
                    "const long long *scan_ids", "const long long *out_offsets", "const int *nbr", "const unsigned *keep",
                    "const unsigned *allowed", "long long *pred", "int *comp", "int *stats", "void *ws", "long long ws_bytes",
                    "void *stream"]
    proto = _lib.PROTOTYPES["geot_scan_islands"]
    assert len(proto) == len(args)
    for a, t in zip(args, proto):
        want = ctypes.c_void_p if "*" in a else ctypes.c_longlong if a.startswith("long long") else ctypes.c_int
        assert t is want, (a, t)
    assert lib.geot_scan_islands.argtypes == proto and lib.geot_scan_islands.restype is ctypes.c_int
    assert re.search(r"long long geot_scan_islands_ws_bytes\(int b, long long total_out, int c\);", hdr)
    assert _lib.PLAIN["geot_scan_islands_ws_bytes"] == ([ctypes.c_int, ctypes.c_longlong, ctypes.c_int], ctypes.c_longlong)
    for name in ("clean_scans", "scan_components", "scan_neighbours", "teeth3ds_result"):
        assert callable(getattr(validation, name)) and getattr(geot_amd, name) is getattr(validation, name)
    assert validation.ISLANDS_MAX_K == 32


def test_workspace_size_and_entry_point_refusals_need_no_device():
    from geot_amd import _lib
    lib = _lib.load()
    ws = lib.geot_scan_islands_ws_bytes
    head = ws(2, 0, 17)
    assert head == 2 * 17 * 8 and head % 16 == 0                        # per slot and class the packed largest piece
    assert ws(3, 0, 17) == 416 and ws(3, 0, 17) % 16 == 0               # 408 rounded up
    assert ws(2, 1000, 17) - head == 1000 * 4 * (17 + 2)                # per vertex a parent, a size and c vote counts
    assert ws(0, 0, 1) == 0 and ws(65535, 10, 32) > 0 and ws(1, 1 << 40, 32) > 0
    for b, total, c in ((-1, 10, 17), (65536, 10, 17), (2, -1, 17), (2, 10, 0), (2, 10, 33), (2, (1 << 40) + 1, 17)):
        assert ws(b, total, c) == -1, (b, total, c)
    # hipErrorInvalidValue (1) before any launch: the pointers are never followed
    fake = 1 << 20
    good = dict(b=2, c=17, k=9, min_size=10, n_scans=3, total=100, offsets=fake, scan_ids=fake, out_offsets=fake, nbr=fake,
                keep=None, allowed=None, pred=fake, comp=None, stats=None, ws=fake, ws_bytes=head)
    for change in (dict(c=0), dict(c=33), dict(k=0), dict(k=33), dict(min_size=-1), dict(b=-1), dict(b=65536), dict(n_scans=0),
                   dict(total=0), dict(offsets=None), dict(scan_ids=None), dict(out_offsets=None), dict(nbr=None), dict(pred=None),
                   dict(ws=None), dict(ws=fake + 4), dict(ws=fake + 8), dict(ws_bytes=head - 16), dict(ws_bytes=-1)):
        a = dict(good, **change)
        assert lib.geot_scan_islands(*a.values(), None) == 1, change
    assert lib.geot_scan_islands(*dict(good, b=0, ws_bytes=0).values(), None) == 0      # nothing to do


def test_python_refusals_come_before_any_device_call():
    import torch
    from geot_amd import validation as V
    from geot_amd.fit import fit
    batch = {"scans": None, "sizes": [20, 30], "scan_ids": None, "mandible": [True, False]}
    preds = [torch.zeros(1, 20, dtype=torch.int64), torch.zeros(1, 30, dtype=torch.int64)]
    for bad in (-1, 2.5, True, "3"):
        with pytest.raises(RuntimeError, match="min_size must be an int >= 0"):
            V.clean_scans(preds, batch, min_size=bad)
    for bad in (0, 32, 2.0, True):
        with pytest.raises(RuntimeError, match="k must be an int in 1..31"):
            V.clean_scans(preds, batch, k=bad)
    for bad in (3, "ab", [1, 40], [True]):
        with pytest.raises(RuntimeError, match="keep_largest"):
            V.clean_scans(preds, batch, keep_largest=bad)
    with pytest.raises(RuntimeError, match="int64"):
        V.clean_scans([p.int() for p in preds], batch)
    with pytest.raises(RuntimeError, match="one prediction tensor per scan"):
        V.clean_scans(preds[:1], batch)
    with pytest.raises(RuntimeError, match="30 predictions for a scan of 20"):
        V.scan_components(preds[::-1], batch)

    class OnGpu:
        device = torch.device("cuda", 0)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        V.clean_scans(preds, dict(batch, scans=OnGpu()))

    class Never:
        def eval(self):
            raise AssertionError("called")
    for bad in (3, "yes", 2.0, [1], {"size": 3}, {"min_size": -1}, {"k": 0}, {"keep_largest": 7}, {"stats": True}):
        with pytest.raises(ValueError, match="islands"):
            V.predict_scans(None, None, islands=bad)
        with pytest.raises(ValueError, match="islands"):
            V.vote_scans(Never(), None, [0], 2, islands=bad)
        with pytest.raises(ValueError, match="islands"):
            V.cover_scans(Never(), None, [0], islands=bad)
        with pytest.raises(ValueError, match="islands"):
            V.decode_scans(Never(), None, [0], islands=bad)
        for name in ("validate_scans", "validate_scans_voted", "validate_scans_covered", "validate_scans_decoded"):
            with pytest.raises(ValueError, match="islands"):
                getattr(V, name)(Never(), None, {"num_votes": 2}, islands=bad)
        with pytest.raises(ValueError, match="islands"):
            fit(None, None, {"epochs": 1}, islands=bad)
    assert V._islands_kw(None, "t") is None and V._islands_kw(False, "t") is None and V._islands_kw(True, "t") == {}
    assert V._islands_kw({"min_size": 4, "keep_largest": [1, 2], "k": 5}, "t") == {"min_size": 4, "keep_largest": [1, 2], "k": 5}


def test_scan_neighbours_refuses_a_scan_shorter_than_its_rows():
    import torch
    from geot_amd.validation import scan_neighbours

    class Scans:
        device = torch.device("cpu")
    batch = {"scans": Scans(), "sizes": [8, 30], "scan_ids": torch.zeros(2, dtype=torch.int64)}
    with pytest.raises(ValueError, match="a scan of 8 vertices has no 9 nearest vertices"):
        scan_neighbours(batch, k=8)


def test_teeth3ds_result_on_both_jaws():
    import torch
    from geot_amd.validation import teeth3ds_result
    labels = np.array([0, 1, 1, 8, 9, 16, 0, 1, 3, 3], dtype=np.int64)
    comp = np.array([0, 1, 1, 3, 4, 5, 0, 7, 8, 8], dtype=np.int32)        # class 1 lies in two pieces: roots 1 and 7
    low = teeth3ds_result(labels, comp, "lower", patient="0EAKT1CU")
    assert low == {"id_patient": "0EAKT1CU", "jaw": "lower", "labels": [0, 31, 31, 38, 41, 48, 0, 31, 33, 33],
                   "instances": [0, 1, 1, 2, 3, 4, 0, 5, 6, 6]}
    up = teeth3ds_result(torch.from_numpy(labels).view(1, -1), torch.from_numpy(comp).view(1, -1), "upper")
    assert up["labels"] == [0, 11, 11, 18, 21, 28, 0, 11, 13, 13] and up["instances"] == low["instances"] and up["id_patient"] is None
    assert all(type(v) is int for v in up["labels"] + up["instances"])
    # every class of both jaws: the inverse of the dataset's label2id
    every = np.arange(17)
    assert teeth3ds_result(every, every, "lower")["labels"] == [0] + list(range(31, 39)) + list(range(41, 49))
    assert teeth3ds_result(every, every, "upper")["labels"] == [0] + list(range(11, 19)) + list(range(21, 29))
    assert teeth3ds_result(every, every, "upper")["instances"] == list(range(17))
    empty = teeth3ds_result(np.zeros(0, np.int64), np.zeros(0, np.int32), "lower")
    assert empty["labels"] == [] and empty["instances"] == []
    with pytest.raises(ValueError, match="jaw"):
        teeth3ds_result(labels, comp, "mandible")
    with pytest.raises(RuntimeError, match="0 .. 16"):
        teeth3ds_result(labels + 10, comp, "lower")
    with pytest.raises(RuntimeError, match="10 labels and 9 components"):
        teeth3ds_result(labels, comp[:9], "lower")


# ---- the oracle on graphs small enough to check by hand -----------------------------------------------------------------------------
def _path(m):
    return np.array([[v + 1 if v + 1 < m else -1] for v in range(m)])


def test_oracle_components_by_hand():
    # 0-1-2 | 3-4 by labels on a path; the table is directed, the edge is not
    labels = [2, 2, 2, 5, 5]
    assert iref.components(labels, _path(5), 8).tolist() == [0, 0, 0, 3, 3]
    back = np.array([[-1], [0], [1], [2], [3]])                          # only the backward entries
    assert iref.components(labels, back, 8).tolist() == [0, 0, 0, 3, 3]
    # entries that do not exist: negative, >= m, the vertex itself; a duplicate is harmless
    rows = np.array([[0, -1, 9, 5], [1, 1, -7, 5], [3, 3, 3, 2], [-1, -1, -1, -1], [4, -1, 6, 4], [0, 0, 0, 0]])
    assert iref.existing(rows, 6).tolist() == [[False, False, False, True], [False, False, False, True], [True, True, True, False],
                                               [False] * 4, [False] * 4, [True] * 4]
    assert iref.components([1, 1, 1, 1, 1, 1], rows, 2).tolist() == [0, 0, 2, 2, 4, 0]
    # a label outside [0, c) is its own component and joins nobody
    assert iref.components([1, 9, 1, -1, -1], _path(5), 2).tolist() == [0, 1, 2, 3, 4]


def test_oracle_islands_by_hand():
    # a path 0..9: class 1 on 0-3, a piece of class 2 on 4-5, class 1 again on 6-9; both directions in the table
    m = 10
    nbr = np.array([[v - 1, v + 1 if v + 1 < m else -1] for v in range(m)])
    labels = np.array([1, 1, 1, 1, 2, 2, 1, 1, 1, 1])
    # min_size at size, size + 1: the piece of two vertices survives 2 and falls to 3; its votes are 3 -> class 1, 6 -> class 1
    out, comp, st = iref.scan_islands_slot(labels, nbr, 4, 2)
    assert out.tolist() == labels.tolist() and comp.tolist() == [0, 0, 0, 0, 4, 4, 6, 6, 6, 6] and st == [3, 0, 0, 0]
    out, comp, st = iref.scan_islands_slot(labels, nbr, 4, 3)
    assert out.tolist() == [1] * 10 and comp.tolist() == [0, 0, 0, 0, 4, 4, 6, 6, 6, 6] and st == [3, 1, 2, 0]
    # keep class 1 to its largest piece: two pieces of four, the lower root stays; the other takes class 2's label
    out, _, st = iref.scan_islands_slot(labels, nbr, 4, 0, keep=1 << 1)
    assert out.tolist() == [1, 1, 1, 1, 2, 2, 2, 2, 2, 2] and st == [3, 1, 4, 0]
    # ... and with the small piece an island too, the second piece of class 1 has no neighbour left to vote: stranded
    out, _, st = iref.scan_islands_slot(labels, nbr, 4, 3, keep=1 << 1)
    assert out.tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1] and st == [3, 2, 2, 4]
    # allowed without class 2: the piece goes whatever its size; a tie of votes (one for 1 from each side ... and one for 3)
    labels = np.array([1, 1, 1, 1, 2, 2, 3, 3, 3, 3])
    out, _, st = iref.scan_islands_slot(labels, nbr, 4, 0, allowed=0b1011)
    assert out.tolist() == [1, 1, 1, 1, 1, 1, 3, 3, 3, 3] and st == [3, 1, 2, 0]       # votes 1: 1, 3: 1 -> the lower class
    # forward entries only: with the piece's own rows empty nothing votes, though its neighbours name it
    fwd = nbr.copy()
    fwd[4:6] = [[5, -1], [4, -1]]
    out, _, st = iref.scan_islands_slot(labels, fwd, 4, 3)
    assert out.tolist() == labels.tolist() and st == [3, 1, 0, 2]
    # labels outside [0, c): never an island, never a vote, never written, not counted as components
    labels = np.array([1, 1, 1, 1, 7, -2, 1, 1, 1, 1])
    out, comp, st = iref.scan_islands_slot(labels, nbr, 4, 5)
    assert out.tolist() == labels.tolist() and comp.tolist() == [0, 0, 0, 0, 4, 5, 6, 6, 6, 6] and st == [2, 2, 0, 8]
    # the batch form: a skipped slot keeps its labels and has zero stats
    outs, comps, stats = iref.scan_islands([labels, labels], [nbr, nbr], 4, 5, usable=[True, False])
    assert comps[1] is None and outs[1].tolist() == labels.tolist() and stats.tolist() == [[2, 2, 0, 8], [0, 0, 0, 0]]


def test_oracle_knn_table_orders_by_distance_then_index():
    pts = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [3, 0, 0], [-1, 0, 0]], np.float32)
    assert iref.knn_table(pts, 3).tolist() == [[0, 1, 2], [1, 2, 0], [1, 2, 0], [3, 1, 2], [4, 0, 1]]


def test_the_restatement_alone_restores_the_property_case():
    """What tests/test_scan_islands_val_gpu.py relies on: for the placements of iref.property_case the oracle hands every
    injected cluster back to the tooth around it, touches nothing else, and leaves the uninjected labels alone."""
    for pts, truth, nbr, noisy in iref.property_case():
        assert (noisy != truth).sum() == 30 and (truth[noisy != truth] > 0).all() and (noisy[noisy != truth] > 0).all()
        out, _, st = iref.scan_islands_slot(noisy, nbr, 17, iref.PROPERTY_MIN_SIZE, keep=iref.PROPERTY_KEEP)
        assert np.array_equal(out, truth) and st == [12, 5, 30, 0]
        same, _, st = iref.scan_islands_slot(truth, nbr, 17, iref.PROPERTY_MIN_SIZE, keep=iref.PROPERTY_KEEP)
        assert np.array_equal(same, truth) and st == [7, 0, 0, 0]
