"""geot_scan_islands (csrc/scan_islands.hip) and what is built on it in geot_amd/validation.py -- scan_neighbours,
scan_components, clean_scans -- against the numpy restatement (tests/_scan_islands_ref.py): array_equal for pred, comp and
stats in every case, the same bits from a second call and from the plain form (GEOT_SCAN_ISLANDS_IMPL=basic).  Hand-built
tables that need no geometry (paths, a ring, a star, one directed entry, rows of junk), every rule on either side of its
threshold, ragged batches with skipped slots and gaps, clouds whose table comes from scan_neighbours, and one capture."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scan_islands_ref as iref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PRED_FILL, COMP_FILL, STAT_FILL = -77, -9, -5        # what the buffers hold where the call must not write


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


def _raw(set_sizes, ids, preds, nbrs, c, min_size, keep=None, allowed=None, out_offsets=None, total_out=None, offsets=None,
         want_comp=True, want_stats=True, told=None):
    """geot_scan_islands through the C ABI on slots `ids` of a set of scans of set_sizes vertices; preds / nbrs: per slot the
    labels and the (M, k) table -> (pred, comp, stats) as numpy, the whole buffers.  out_offsets: where the slots lie in the
    buffers (default: packed); told: what the call is told instead."""
    from geot_amd import _lib
    from geot_amd.ext._common import call, ptr
    k = next(np.asarray(t).reshape(len(p), -1).shape[1] for p, t in zip(preds, nbrs) if p is not None)
    lens = [0 if p is None else len(p) for p in preds]
    if out_offsets is None:
        out_offsets = np.concatenate([[0], np.cumsum(lens)[:-1]])
    if total_out is None:
        total_out = int(sum(lens))
    pred = np.full(total_out, PRED_FILL, dtype=np.int64)
    table = np.full((total_out, k), 0x7fffffff, dtype=np.int32)
    for p, t, o in zip(preds, nbrs, out_offsets):
        if p is not None:
            pred[o:o + len(p)] = p
            table[o:o + len(p)] = np.asarray(t).reshape(len(p), k)
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum(set_sizes)])
    b = len(ids)
    d_pred, d_nbr = _dev(pred, np.int64), _dev(table, np.int32)
    d_off, d_ids, d_out = _dev(offsets, np.int64), _dev(ids, np.int64), _dev(out_offsets if told is None else told, np.int64)
    d_keep = None if keep is None else _dev(np.asarray(keep, dtype=np.uint32).view(np.int32), np.int32)
    d_allowed = None if allowed is None else _dev(np.asarray(allowed, dtype=np.uint32).view(np.int32), np.int32)
    comp = torch.full((total_out,), COMP_FILL, dtype=torch.int32, device=DEV) if want_comp else None
    stats = torch.full((b, 4), STAT_FILL, dtype=torch.int32, device=DEV) if want_stats else None
    nbytes = int(_lib.load().geot_scan_islands_ws_bytes(b, total_out, c))
    ws = torch.randint(0, 255, (nbytes,), dtype=torch.uint8, device=DEV)           # the contents are irrelevant on entry
    call("geot_scan_islands", DEV, b, c, k, min_size, len(set_sizes), int(sum(set_sizes)), ptr(d_off), ptr(d_ids), ptr(d_out),
         ptr(d_nbr), ptr(d_keep), ptr(d_allowed), ptr(d_pred), ptr(comp), ptr(stats), ptr(ws), nbytes)
    torch.cuda.synchronize()
    return (d_pred.cpu().numpy(), None if comp is None else comp.cpu().numpy(), None if stats is None else stats.cpu().numpy())


def _check(preds, nbrs, c, min_size, keep=None, allowed=None, usable=None, monkeypatch=None, **raw):
    """One batch of slots, slot s on scan s of a set sized by the slots (unless raw says otherwise): pred, comp and stats
    against the restatement over the WHOLE buffers, a second call, and -- with monkeypatch -- the plain form."""
    b = len(preds)
    lens = [0 if p is None else len(p) for p in preds]
    set_sizes = raw.pop("set_sizes", [max(n, 1) for n in lens])
    ids = raw.pop("ids", list(range(b)))
    out_offsets = raw.get("out_offsets")
    if out_offsets is None:
        out_offsets = np.concatenate([[0], np.cumsum(lens)[:-1]])
    total_out = raw.get("total_out") or int(sum(lens))
    usable = [p is not None for p in preds] if usable is None else usable
    want, want_comp, want_stats = iref.scan_islands([np.zeros(0) if p is None else p for p in preds],
                                                    [np.zeros((0, 1)) if t is None else t for t in nbrs], c, min_size, keep, allowed,
                                                    usable)
    e_pred = np.full(total_out, PRED_FILL, dtype=np.int64)
    e_comp = np.full(total_out, COMP_FILL, dtype=np.int32)
    for s, (p, o) in enumerate(zip(preds, out_offsets)):
        if p is not None:
            e_pred[o:o + len(p)] = want[s]
            if usable[s]:
                e_comp[o:o + len(p)] = want_comp[s]
    got = _raw(set_sizes, ids, preds, nbrs, c, min_size, keep, allowed, **raw)
    print("c=%d min_size=%d sizes=%s: stats (components, islands, changed, stranded) %s" % (c, min_size, lens, got[2].tolist()))
    assert np.array_equal(got[2], want_stats), (got[2].tolist(), want_stats.tolist())
    assert np.array_equal(got[1], e_comp), int((got[1] != e_comp).sum())
    assert np.array_equal(got[0], e_pred), int((got[0] != e_pred).sum())
    again = _raw(set_sizes, ids, preds, nbrs, c, min_size, keep, allowed, **raw)
    assert all(np.array_equal(a, g) for a, g in zip(again, got))
    if monkeypatch is not None:
        monkeypatch.setenv("GEOT_SCAN_ISLANDS_IMPL", "basic")
        plain = _raw(set_sizes, ids, preds, nbrs, c, min_size, keep, allowed, **raw)
        monkeypatch.delenv("GEOT_SCAN_ISLANDS_IMPL")
        assert all(np.array_equal(a, g) for a, g in zip(plain, got))
    return got


# ---- hand-built tables ----------------------------------------------------------------------------------------------------------------
M_PATH = 4096


def _path_tables():
    rng = np.random.default_rng(11)
    fwd = np.arange(1, M_PATH + 1).reshape(-1, 1)
    fwd[-1] = -1
    back = np.arange(-1, M_PATH - 1).reshape(-1, 1)
    perm = rng.permutation(M_PATH)                       # the path visits perm[0], perm[1], ...: deep trees, long CAS chains
    shuffled = np.full((M_PATH, 1), -1)
    shuffled[perm[:-1], 0] = perm[1:]
    ring = ((np.arange(M_PATH) + 1) % M_PATH).reshape(-1, 1)
    star = np.full((M_PATH, 1), M_PATH - 1)              # every leaf names the hub, the hub (the highest index) names itself
    return [fwd, back, shuffled, ring, star]


def test_paths_ring_and_star_of_one_label(monkeypatch):
    tables = _path_tables()
    preds = [np.ones(M_PATH, dtype=np.int64) for _ in tables]
    got = _check(preds, tables, 2, 0, monkeypatch=monkeypatch)                  # components only
    assert (got[1] == 0).all() and got[2][:, 0].tolist() == [1] * 5
    assert (got[1].reshape(5, -1) == 0).all()


def test_paths_ring_and_star_cut_into_pieces(monkeypatch):
    """The same tables under labels that cut them: runs of 1 .. 40 vertices of three classes along the index; pieces below
    min_size are relabelled by what their rows name."""
    rng = np.random.default_rng(12)
    tables = _path_tables()
    preds = []
    for _ in tables:
        runs = rng.integers(1, 41, size=M_PATH)
        preds.append(np.repeat(rng.integers(0, 3, size=M_PATH), runs)[:M_PATH].astype(np.int64))
    _check(preds, tables, 3, 8, keep=[0b110] * 5, monkeypatch=monkeypatch)


@pytest.mark.parametrize("forward", [True, False])
def test_one_directed_entry_joins_two_components(forward):
    m = 20
    nbr = np.array([[v + 1 if v + 1 < m and v != 9 else -1, -1] for v in range(m)])       # 0-9 and 10-19
    sep = _check([np.ones(m, dtype=np.int64)], [nbr], 2, 0)
    assert sep[1].tolist() == [0] * 10 + [10] * 10 and sep[2][0, 0] == 2
    if forward:
        nbr[9, 1] = 10
    else:
        nbr[10, 1] = 9
    got = _check([np.ones(m, dtype=np.int64)], [nbr], 2, 0)
    assert (got[1] == 0).all() and got[2][0, 0] == 1


def test_rows_of_junk_join_nothing():
    m = 70
    rng = np.random.default_rng(13)
    nbr = np.empty((m, 6), dtype=np.int64)
    nbr[:, 0] = -1
    nbr[:, 1] = np.arange(m)                                 # itself
    nbr[:, 2] = rng.choice([m, m + 1, 2 ** 31 - 1, -2 ** 31, -5], size=m)
    nbr[:, 3] = nbr[:, 1]
    nbr[:, 4] = nbr[:, 2]
    nbr[:, 5] = -1
    got = _check([np.ones(m, dtype=np.int64)], [nbr], 2, 3, keep=[0b10])
    assert got[1].tolist() == list(range(m)) and got[2].tolist() == [[m, m, 0, m]]         # every vertex a stranded island
    nbr[:, 5] = (np.arange(m) // 7) * 7                      # one real entry, duplicated: groups of seven around their first
    nbr[:, 0] = nbr[:, 5]
    got = _check([np.ones(m, dtype=np.int64)], [nbr], 2, 0)
    assert got[1].tolist() == [v // 7 * 7 for v in range(m)]


# ---- the rules --------------------------------------------------------------------------------------------------------------------------
def _grid(w, h):
    """The 4-neighbour table of a w x h grid, vertex y * w + x."""
    nbr = np.full((w * h, 4), -1)
    for y in range(h):
        for x in range(w):
            v = y * w + x
            nbr[v] = [v - 1 if x else -1, v + 1 if x + 1 < w else -1, v - w if y else -1, v + w if y + 1 < h else -1]
    return nbr


def test_min_size_on_either_side_of_a_piece():
    w = h = 16
    nbr = _grid(w, h)
    labels = np.ones(w * h, dtype=np.int64)
    piece = [5 * w + 5, 5 * w + 6, 5 * w + 7, 6 * w + 5, 6 * w + 6, 7 * w + 6]       # six vertices of class 2
    labels[piece] = 2
    for min_size, gone in ((5, False), (6, False), (7, True)):
        got = _check([labels], [nbr], 3, min_size)
        assert (got[0][piece] == (1 if gone else 2)).all() and got[2][0].tolist() == [2, int(gone), 6 * gone, 0]


def test_equal_pieces_vote_ties_and_stranded_islands(monkeypatch):
    w, h = 12, 9
    nbr = _grid(w, h)
    labels = np.zeros(w * h, dtype=np.int64)
    labels[[1 * w + 1, 1 * w + 2]] = 3                       # two pieces of class 3 of equal size: the lower root stays
    labels[[4 * w + 6, 4 * w + 7]] = 3
    got = _check([labels], [nbr], 4, 0, keep=[1 << 3], monkeypatch=monkeypatch)
    assert (got[0][[1 * w + 1, 1 * w + 2]] == 3).all() and (got[0][[4 * w + 6, 4 * w + 7]] == 0).all()
    # a vote tie: a single vertex of class 3 between two of class 1 and two of class 2 -> the lower class
    labels = np.zeros(w * h, dtype=np.int64)
    v = 4 * w + 4
    labels[[v - 1, v + 1]] = 2
    labels[[v - w, v + w]] = 1
    labels[v] = 3
    got = _check([labels], [nbr], 4, 0, allowed=[0b0111])
    assert got[0][v] == 1 and got[2][0].tolist()[1:] == [1, 1, 0]
    # stranded: an island whose neighbours are all islands (a checkerboard of single vertices, min_size 2) ...
    board = ((np.arange(w * h) // w + np.arange(w * h) % w) % 2).astype(np.int64)
    got = _check([board], [nbr], 2, 2)
    assert np.array_equal(got[0], board) and got[2][0].tolist() == [w * h, w * h, 0, w * h]
    # ... and one with no entries at all, beside one that is relabelled
    labels = np.ones(w * h, dtype=np.int64)
    labels[[2 * w + 2, 6 * w + 6]] = 2
    cut = nbr.copy()
    cut[2 * w + 2] = -1
    got = _check([labels], [cut], 3, 2)
    assert got[0][2 * w + 2] == 2 and got[0][6 * w + 6] == 1 and got[2][0].tolist() == [3, 2, 1, 1]


def test_keep_and_allowed_bits_per_slot_and_labels_out_of_range(monkeypatch):
    w, h = 10, 10
    nbr = _grid(w, h)
    rng = np.random.default_rng(14)
    labels = (np.arange(w * h) % w // 4).astype(np.int64)                # three vertical bands: classes 0, 1, 2
    labels[rng.choice(w * h, 12, replace=False)] = rng.integers(0, 3, 12)
    labels[[33, 34, 77]] = [5, -1, 3]                                    # outside [0, 3): own pieces, never written, never vote
    preds = [labels] * 6
    keep = [0, 0b111, 0b010, 0, 0b100, 0xffffffff]
    allowed = [0xffffffff, 0xffffffff, 0b011, 0b101, 0b110, 0]
    got = _check(preds, [nbr] * 6, 3, 0, keep=keep, allowed=allowed, monkeypatch=monkeypatch)
    flat = got[0].reshape(6, -1)
    assert np.array_equal(flat[0], labels) and (flat[:, [33, 34, 77]] == [5, -1, 3]).all()
    assert np.array_equal(flat[5], labels) and got[2][5, 3] == 97         # nothing allowed: every piece a stranded island
    _check(preds[:2], [nbr] * 2, 3, 3, keep=None, allowed=allowed[3:5])
    _check(preds[:2], [nbr] * 2, 3, 3, keep=keep[1:3], allowed=None)


def _random_case(m, k, c, seed):
    """Labels in runs along the index with noise and values outside [0, c); a table of nearby indices with junk entries."""
    rng = np.random.default_rng(seed)
    runs = rng.integers(1, 30, size=m)
    labels = np.repeat(rng.integers(0, c, size=m), runs)[:m].astype(np.int64)
    noise = rng.choice(m, m // 10, replace=False)
    labels[noise] = rng.integers(-1, c + 1, size=noise.size)
    nbr = np.arange(m)[:, None] + rng.integers(-6, 7, size=(m, k))
    nbr[rng.random((m, k)) < 0.15] = -1
    far = rng.random((m, k)) < 0.02
    nbr[far] = rng.integers(0, m, size=int(far.sum()))
    return labels, nbr


@pytest.mark.parametrize("k", [1, 9, 32])
@pytest.mark.parametrize("c", [1, 2, 17, 32])
def test_class_counts_and_table_widths(c, k, monkeypatch):
    rng = np.random.default_rng(100 * c + k)
    sizes = [700, 257]
    cases = [_random_case(m, k, c, 1000 * c + 10 * k + s) for s, m in enumerate(sizes)]
    keep = rng.integers(0, 1 << c, size=2, dtype=np.uint64).astype(np.uint32)
    allowed = (rng.integers(0, 1 << c, size=2, dtype=np.uint64) | rng.integers(0, 1 << c, size=2, dtype=np.uint64)).astype(np.uint32)
    for min_size, kw in ((0, dict()), (4, dict(keep=keep)), (10, dict(keep=keep, allowed=allowed))):
        _check([p for p, _ in cases], [t for _, t in cases], c, min_size, monkeypatch=monkeypatch if min_size == 4 else None, **kw)


# ---- batches ----------------------------------------------------------------------------------------------------------------------------
def test_skipped_slots_gaps_and_optional_outputs():
    sizes = [300, 120, 64, 200]
    cases = [_random_case(m, 5, 4, 50 + s) for s, m in enumerate(sizes)]
    preds, nbrs = [p for p, _ in cases], [t for _, t in cases]
    keep = [0b1110] * 4
    # out_offsets with gaps: the words between the slots keep what they held
    gaps = np.array([7, 7 + 300 + 13, 7 + 300 + 13 + 120, 7 + 300 + 13 + 120 + 64 + 1])
    _check(preds, nbrs, 4, 5, keep=keep, out_offsets=gaps, total_out=int(gaps[-1] + 200 + 5))
    # skipped slots -- nothing of the slot is written, its stats are zero.  A scan id outside the set, on either side:
    for ids, usable in (([0, -1, 2, 3], [1, 0, 1, 1]), ([0, 1, 4, 3], [1, 1, 0, 1]), ([1 << 40, 1, 2, -(1 << 40)], [0, 1, 1, 0])):
        _check(preds, nbrs, 4, 5, keep=keep, ids=ids, usable=[bool(u) for u in usable], set_sizes=sizes)
    # an offsets pair that is empty, reversed, ends past `total` or starts below zero.  The slots sit on scans 0, 2, 4, 6 of a
    # set with a spare scan behind each, so one scan's end moves without any other slot's pair changing
    spaced = [300, 10, 120, 10, 64, 10, 200, 10]
    ends = np.concatenate([[0], np.cumsum(spaced)])
    for at, value, slot in ((3, ends[2], 1), (3, ends[2] - 5, 1), (7, ends[-1] + 1, 3), (0, -1, 0)):
        offs = ends.copy()
        offs[at] = value
        _check(preds, nbrs, 4, 5, keep=keep, ids=[0, 2, 4, 6], set_sizes=spaced, offsets=offs, usable=[s != slot for s in range(4)])
    # an out_offsets entry that is negative or leaves no room for the slot in the workspace
    packed = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    for slot, o in ((0, -1), (2, sum(sizes) - 63), (3, sum(sizes)), (1, 1 << 50)):
        told = packed.copy()
        told[slot] = o
        _check(preds, nbrs, 4, 5, keep=keep, told=told, usable=[s != slot for s in range(4)])
    # comp NULL, stats NULL, both
    full = _raw(sizes, [0, 1, 2, 3], preds, nbrs, 4, 5, keep=keep)
    assert full[2].all(axis=1).any()
    for kw in (dict(want_comp=False), dict(want_stats=False), dict(want_comp=False, want_stats=False)):
        part = _raw(sizes, [0, 1, 2, 3], preds, nbrs, 4, 5, keep=keep, **kw)
        assert np.array_equal(part[0], full[0])
        assert (part[1] is None) == (not kw.get("want_comp", True)) and (part[2] is None) == (not kw.get("want_stats", True))
        assert part[1] is None or np.array_equal(part[1], full[1])
        assert part[2] is None or np.array_equal(part[2], full[2])


def test_components_only_form_leaves_every_bit_of_pred():
    labels, nbr = _random_case(900, 7, 5, 77)
    labels[::50] = np.array([1 << 40, -(1 << 50), 5, -1] * 5)[:len(labels[::50])]       # whatever the words hold
    for min_size in (0, 1):
        got = _check([labels], [nbr], 5, min_size)
        assert np.array_equal(got[0], labels) and got[2][0, 1:].tolist() == [0, 0, 0]


# ---- geometry: the table from scan_neighbours ---------------------------------------------------------------------------------------------
RAGGED = [1, 63, 64, 65, 257, 20011]
_world = {}


def _ragged():
    if not _world:
        from geot_amd.openpoints.dataset import DeviceScanSet
        clouds = [iref.surface_scan(m, 20 + s, teeth=6) for s, m in enumerate(RAGGED)]
        dset = DeviceScanSet([p for p, _ in clouds], [l.astype(np.int32) for _, l in clouds], cls=[s % 2 for s in range(len(RAGGED))],
                             device=DEV)
        _world.update(clouds=clouds, dset=dset)
    return _world


def _batch(dset, ids, views=True):
    batch = {"scans": dset, "sizes": [dset.sizes[i] for i in ids], "scan_ids": torch.tensor(ids, dtype=torch.int64, device=DEV),
             "mandible": [i % 2 == 0 for i in ids]}             # the set's cls is i % 2, and 0 is the mandible
    if views:
        pts = torch.split(dset.points, dset.sizes)
        batch["points"] = [pts[i] for i in ids]
    return batch


def test_scan_neighbours_is_the_sorted_search_of_each_scan():
    from geot_amd.knn_cuda import knn_sorted
    from geot_amd.validation import scan_neighbours
    w = _ragged()
    ids = [5, 4, 3]                                      # not in the set's order
    for views in (True, False):                          # the batcher's views read in place / gathered by scan id
        table = scan_neighbours(_batch(w["dset"], ids, views), k=8)
        assert table.dtype == torch.int32 and tuple(table.shape) == (sum(RAGGED[i] for i in ids), 9)
        at = 0
        for i in ids:
            p = torch.from_numpy(w["clouds"][i][0]).to(DEV).view(1, -1, 3)
            _, idx = knn_sorted(p, p, 9)
            assert torch.equal(table[at:at + RAGGED[i]], idx[0])
            at += RAGGED[i]
    small = scan_neighbours(_batch(w["dset"], [4]), k=8).cpu().numpy()
    assert np.array_equal(small, iref.knn_table(w["clouds"][4][0], 9))
    with pytest.raises(ValueError, match="a scan of 1 vertices has no 3 nearest"):
        scan_neighbours(_batch(w["dset"], [4, 0]), k=2)


def _noisy(labels, pts, seed, c):
    """Blob labels plus injected noise: clusters of 1 .. 30 nearby vertices of random classes, and single stray vertices."""
    rng = np.random.default_rng(seed)
    out = labels.copy()
    for _ in range(max(1, len(labels) // 400)):
        at = int(rng.integers(len(labels)))
        lo, hi = max(0, at - 200), min(len(labels), at + 200)       # the order is coherent along x: look nearby only
        near = lo + np.argsort(((pts[lo:hi] - pts[at]) ** 2).sum(1), kind="stable")[:int(rng.integers(1, 31))]
        out[near] = int(rng.integers(c))
    stray = rng.choice(len(labels), max(1, len(labels) // 100), replace=False)
    out[stray] = rng.integers(0, c, size=stray.size)
    return out


def test_ragged_batch_of_clouds_through_the_python_calls(monkeypatch):
    """Slots of 63, 64, 65, 257 and about 20 000 vertices in one clean_scans / scan_components call on scan_neighbours' table,
    with parts and keep_largest; then all six slots, the one-vertex scan among them (no search gives it a row: its row names
    itself and nothing), through the C ABI."""
    from geot_amd.validation import clean_scans, scan_components, scan_neighbours
    w = _ragged()
    c = 7
    ids = [1, 2, 3, 4, 5]
    batch = _batch(w["dset"], ids)
    table = scan_neighbours(batch, k=8)
    nbrs = [t.cpu().numpy() for t in torch.split(table, batch["sizes"])]
    preds = [_noisy(w["clouds"][i][1], w["clouds"][i][0], 30 + i, c) for i in ids]
    parts = [[0, 1, 2, 3, 4], [0, 3, 4, 5, 6]]               # jaw 0 (the mandible: the even scans of this set) and jaw 1
    jaws = [0 if m else 1 for m in batch["mandible"]]
    allowed = [sum(1 << l for l in parts[j]) for j in jaws]
    want, want_comp, want_stats = iref.scan_islands(preds, nbrs, c, 10, [0b1111110] * 5, allowed)
    flat = torch.from_numpy(np.concatenate(preds)).to(DEV)
    views = [p.view(1, -1) for p in torch.split(flat, batch["sizes"])]
    before = scan_components(views, batch, nbr=table, num_classes=c)
    assert torch.equal(flat.cpu(), torch.from_numpy(np.concatenate(preds)))              # the labels are untouched
    got, stats = clean_scans(views, batch, min_size=10, keep_largest=True, parts=parts, nbr=table, stats=True)
    assert all(g is v for g, v in zip(got, views))                                      # in place: the same views
    print("stats (components, islands, changed, stranded)", stats.cpu().tolist())
    assert np.array_equal(stats.cpu().numpy(), want_stats)
    for s in range(5):
        assert before[s].dtype == torch.int32 and tuple(before[s].shape) == (1, RAGGED[ids[s]])
        assert np.array_equal(before[s].cpu().numpy().reshape(-1), want_comp[s]), s
        assert np.array_equal(got[s].cpu().numpy().reshape(-1), want[s]), s
    assert want_stats[:, 1].min() > 0 and want_stats[4, 2] > 100                        # the case is not empty
    # the default table (scan_neighbours inside), a list that is no view of one buffer, the plain form: the same labels
    monkeypatch.setenv("GEOT_SCAN_ISLANDS_IMPL", "basic")
    loose = clean_scans([torch.from_numpy(p).to(DEV) for p in preds], batch, parts=parts)
    monkeypatch.delenv("GEOT_SCAN_ISLANDS_IMPL")
    assert all(np.array_equal(l.cpu().numpy(), wnt) for l, wnt in zip(loose, want))
    # all six slots, the one-vertex scan among them, through the C ABI with k = 9 (its row: itself and junk)
    all_preds = [np.array([3], dtype=np.int64)] + preds
    all_nbrs = [np.array([[0] + [-1] * 8])] + nbrs
    _check(all_preds, all_nbrs, c, 10, keep=[0b1111110] * 6, allowed=[0x7f] + allowed, set_sizes=RAGGED, monkeypatch=monkeypatch)


def test_class_zero_may_lie_in_pieces_and_keep_largest_takes_classes():
    from geot_amd.validation import clean_scans
    w = _ragged()
    batch = _batch(w["dset"], [4])
    pts, labels = w["clouds"][4]
    nbr = iref.knn_table(pts, 9)
    # a wall of class 1 along the middle cuts the gingiva in two large pieces; a second, smaller piece of class 1 far away
    x = pts[:, 0]
    labels = np.zeros(len(pts), dtype=np.int64)
    labels[(x > 14) & (x < 26)] = 1
    labels[np.argsort(x, kind="stable")[:12]] = 1
    comp = iref.components(labels, nbr, 17)
    assert len(np.unique(comp[labels == 0])) >= 2 and len(np.unique(comp[labels == 1])) >= 2
    for keep_largest, mask in ((True, 0x1fffe), (False, 0), ([0], 1), ([0, 1], 3), ((1,), 2)):
        want, _, want_stats = iref.scan_islands([labels], [nbr], 17, 0, [mask], None)
        views = [torch.from_numpy(labels).to(DEV).view(1, -1)]
        got, stats = clean_scans(views, batch, min_size=0, keep_largest=keep_largest, num_classes=17, stats=True)
        assert np.array_equal(got[0].cpu().numpy().reshape(-1), want[0]) and np.array_equal(stats.cpu().numpy(), want_stats)
        if not mask & 1:                                     # the gingiva is never kept to one piece unless it is named
            assert (want[0][labels == 0] == 0).all()
        else:
            assert (want[0] == 0).sum() < (labels == 0).sum()


def test_one_capture_holds_kernel_nodes_only_and_replays_to_the_eager_bits():
    from geot_amd import streams
    from geot_amd.validation import clean_scans, scan_neighbours
    w = _ragged()
    ids = [4, 5]
    batch = _batch(w["dset"], ids)
    table = scan_neighbours(batch, k=8)
    noisy = torch.from_numpy(np.concatenate([_noisy(w["clouds"][i][1], w["clouds"][i][0], 60 + i, 7) for i in ids])).to(DEV)
    sizes = batch["sizes"]
    eager = noisy.clone()
    _, eager_stats = clean_scans([p.view(1, -1) for p in torch.split(eager, sizes)], batch, nbr=table, num_classes=7, stats=True)
    assert not torch.equal(eager, noisy)
    static = noisy.clone()
    from geot_amd import _lib
    from geot_amd.ext._common import call, ptr
    nbytes = int(_lib.load().geot_scan_islands_ws_bytes(2, static.numel(), 7))
    held = {"ws": torch.empty(nbytes, dtype=torch.uint8, device=DEV), "stats": torch.empty((2, 4), dtype=torch.int32, device=DEV),
            "out": torch.tensor([0, sizes[0]], dtype=torch.int64).to(DEV), "keep": torch.tensor([0x7e, 0x7e], dtype=torch.int32).to(DEV)}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with streams.capture(graph, DEV):
        call("geot_scan_islands", DEV, 2, 7, 9, 10, len(w["dset"]), int(w["dset"].points.shape[0]), ptr(w["dset"].offsets),
             ptr(batch["scan_ids"]), ptr(held["out"]), ptr(table), ptr(held["keep"]), None, ptr(static), None, ptr(held["stats"]),
             ptr(held["ws"]), nbytes)
    kinds = streams.node_types(graph)
    assert set(kinds) == {"kernel"} and kinds["kernel"] == 6, kinds
    for _ in range(2):
        static.copy_(noisy)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, eager) and torch.equal(held["stats"], eager_stats)
