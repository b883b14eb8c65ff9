"""geot_mesh_neighbours (csrc/mesh_neighbours.hip) through the C ABI against the numpy restatement (tests/_mesh_ref.py):
array_equal for the table and the stats over the WHOLE buffers, in guarded arenas -- nbr, stats, the faces and the workspace lie
between guard elements that are compared afterwards; the workspace arrives full of noise.  The smallest shapes at which each
branch can go wrong: a grid just past one scan block (4 225 vertices) said in three ways, widths on either side of the valence,
fans on either side of the lane / wave threshold, ragged and skipped slots, faces with indices outside the scan, the plain form
(GEOT_MESH_NEIGHBOURS_IMPL=basic), and one capture.

A skipped slot: its rows are untouched and its stats row is written with zeros, as include/geot_hip.h says (and as
geot_scan_islands does)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_ref as mref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NBR_FILL, STAT_FILL, GUARD_FILL = -77, -5, 0x5a5a5a5a        # what the buffers hold where the call must not write
GUARD = 64                                                   # guard elements on either side of every arena


class Arena:
    """n elements between two guards; `inner` is what the call is given."""

    def __init__(self, values, dtype, fill=GUARD_FILL):
        values = np.ascontiguousarray(np.asarray(values).astype(dtype)).reshape(-1)
        host = np.full(values.size + 2 * GUARD, fill, dtype=dtype)
        host[GUARD:GUARD + values.size] = values
        self.fill, self.n = host[0], values.size
        self.whole = torch.from_numpy(host).to(DEV)
        self.inner = self.whole[GUARD:GUARD + self.n]

    def ptr(self):
        return self.inner.data_ptr()

    def intact(self):
        host = self.whole.cpu().numpy()
        return bool((host[:GUARD] == self.fill).all() and (host[GUARD + self.n:] == self.fill).all())


def _raw(set_sizes, set_faces, ids, k, offsets=None, face_offsets=None, total_faces=None, out_offsets=None, total_out=None,
         told_out=None, told_face_out=None, want_stats=True, null_faces=False):
    """geot_mesh_neighbours on slots `ids` of a set of scans of set_sizes vertices and set_faces faces -> (nbr (total_out, k),
    stats (b, 4) or None) as numpy, the whole buffers; the guards of every arena are checked.  out_offsets: where the slots'
    rows lie (default: packed); told_out / told_face_out / offsets / face_offsets / total_faces: what the call is told instead
    of the truth."""
    from geot_amd import _lib
    from geot_amd.ext._common import call
    b = len(ids)
    inside = [i if 0 <= i < len(set_sizes) else None for i in ids]
    lens = [0 if i is None else set_sizes[i] for i in inside]
    counts = [0 if i is None else len(set_faces[i]) for i in inside]
    if out_offsets is None:
        out_offsets = np.concatenate([[0], np.cumsum(lens)[:-1]])
    if total_out is None:
        total_out = int(sum(lens))
    face_out = np.concatenate([[0], np.cumsum(counts)])
    batch_faces = int(face_out[-1])
    all_faces = np.concatenate([np.asarray(f, dtype=np.int64).reshape(-1, 3) for f in set_faces])
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum(set_sizes)])
    if face_offsets is None:
        face_offsets = np.concatenate([[0], np.cumsum([len(f) for f in set_faces])])
    nbytes = int(_lib.load().geot_mesh_neighbours_ws_bytes(b, total_out, batch_faces))
    assert nbytes > 0 and nbytes % 16 == 0
    rng = np.random.default_rng(nbytes)
    a_faces = Arena(all_faces, np.int32)
    a_nbr = Arena(np.full(total_out * k, NBR_FILL), np.int32)
    a_stats = Arena(np.full(b * 4, STAT_FILL), np.int32)
    a_ws = Arena(rng.integers(0, 256, size=nbytes), np.uint8, fill=0xa5)         # the contents are irrelevant on entry
    assert a_ws.ptr() % 16 == 0
    d = [torch.from_numpy(np.asarray(x, dtype=np.int64)).to(DEV) for x in
         (offsets, face_offsets, ids, out_offsets if told_out is None else told_out, face_out if told_face_out is None else told_face_out)]
    call("geot_mesh_neighbours", DEV, b, k, len(set_sizes), int(sum(set_sizes)), len(all_faces) if total_faces is None else total_faces,
         None if null_faces else a_faces.ptr(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
         batch_faces, a_nbr.ptr(), a_stats.ptr() if want_stats else None, a_ws.ptr(), nbytes)
    torch.cuda.synchronize()
    assert a_faces.intact() and a_nbr.intact() and a_stats.intact() and a_ws.intact(), "a guard element was written"
    stats = a_stats.inner.cpu().numpy().reshape(b, 4)
    if not want_stats:
        assert (stats == STAT_FILL).all()
    return a_nbr.inner.cpu().numpy().reshape(total_out, k), stats if want_stats else None


def _check(set_sizes, set_faces, ids, k, usable=None, monkeypatch=None, **raw):
    """One call against the restatement over the whole buffers; a second call; with monkeypatch the plain form.  usable[s]
    False: the slot must be skipped (rows untouched, stats zero)."""
    b = len(ids)
    usable = [True] * b if usable is None else usable
    inside = [i if 0 <= i < len(set_sizes) else None for i in ids]
    lens = [0 if i is None else set_sizes[i] for i in inside]
    out_offsets = raw.get("out_offsets")
    if out_offsets is None:
        out_offsets = np.concatenate([[0], np.cumsum(lens)[:-1]])
    total_out = raw.get("total_out") or int(sum(lens))
    e_nbr = np.full((total_out, k), NBR_FILL, dtype=np.int32)
    e_stats = np.zeros((b, 4), dtype=np.int32)
    for s, (i, o) in enumerate(zip(inside, out_offsets)):
        if usable[s]:
            e_nbr[o:o + lens[s]], e_stats[s] = mref.mesh_table(set_faces[i], set_sizes[i], k)
    got = _raw(set_sizes, set_faces, ids, k, **raw)
    print("k=%d sizes=%s: stats (usable, ignored, truncated, longest) %s" % (k, lens, got[1].tolist()))
    assert np.array_equal(got[1], e_stats), (got[1].tolist(), e_stats.tolist())
    assert np.array_equal(got[0], e_nbr), int((got[0] != e_nbr).sum())
    again = _raw(set_sizes, set_faces, ids, k, **raw)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
    if monkeypatch is not None:
        monkeypatch.setenv("GEOT_MESH_NEIGHBOURS_IMPL", "basic")
        plain = _raw(set_sizes, set_faces, ids, k, **raw)
        monkeypatch.delenv("GEOT_MESH_NEIGHBOURS_IMPL")
        assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1])
    return got


R = 65                                  # 65 x 65 vertices: 4 225, just past one scan block and one wave multiple; 8 192 faces
M_GRID = R * R
_kept = {}


def _grid():
    if "grid" not in _kept:
        _kept["grid"] = mref.grid(R, R)
    return _kept["grid"]


def fans(rims):
    """Closed fans side by side in one scan -> (vertex count, faces); fan j's centre is the first vertex of its block."""
    at, out = 0, []
    for rim in rims:
        out.append(mref.fan(rim).astype(np.int64) + at)
        at += rim + 1
    return at, np.concatenate(out).astype(np.int32)


def test_the_grid_said_in_three_ways_gives_the_same_bits(monkeypatch):
    faces = _grid()
    assert faces.shape == (8192, 3)
    plain = _check([M_GRID], [faces], [0], 16, monkeypatch=monkeypatch)
    assert plain[1].tolist() == [[8192, 0, 0, 6]]
    shuffled = _check([M_GRID], [mref.shuffled(faces, 1)], [0], 16)
    turned = _check([M_GRID], [mref.shuffled(faces, 2, corners=True, duplicate=0.1)], [0], 16, monkeypatch=monkeypatch)
    assert np.array_equal(shuffled[0], plain[0]) and np.array_equal(turned[0], plain[0])
    assert shuffled[1].tolist() == plain[1].tolist() and turned[1].tolist() == [[8192 + 819, 0, 0, 6]]


@pytest.mark.parametrize("k", [1, 5, 6, 7, 32])
def test_widths_on_either_side_of_the_valence(k, monkeypatch):
    got = _check([M_GRID], [mref.shuffled(_grid(), 3, corners=True)], [0], k, monkeypatch=monkeypatch)
    interior = (R - 2) * (R - 2)                        # valence 6; an edge vertex has 4, two corners 3 and two 2
    truncated = {1: M_GRID, 5: interior}.get(k, 0)
    assert got[1].tolist() == [[8192, 0, truncated, min(k, 6)]]


@pytest.mark.parametrize("k", [32, 16])
def test_a_fan_whose_centre_is_truncated(k, monkeypatch):
    got = _check([41], [mref.shuffled(mref.fan(40), 4, corners=True)], [0], k, monkeypatch=monkeypatch)
    assert got[1].tolist() == [[40, 0, 1, k]] and got[0][0].tolist() == list(range(1, k + 1))


def test_raw_rows_on_either_side_of_the_lane_wave_threshold(monkeypatch):
    """A fan's centre has two raw entries per face: 32 faces are GEOT_MESH_NEIGHBOURS_LANE_ROW entries (one lane), one face more
    goes to the wave.  Then rows of several wave steps, and several long rows inside one wave."""
    from geot_amd import _lib
    at = _lib.MESH_NEIGHBOURS_LANE_ROW // 2
    assert at == 32
    sizes, faces = [at + 1, at + 2], [mref.shuffled(mref.fan(at), 5, corners=True), mref.shuffled(mref.fan(at + 1), 6, corners=True)]
    got = _check(sizes, faces, [0, 1], 32, monkeypatch=monkeypatch)
    assert got[1].tolist() == [[at, 0, 0, 32], [at + 1, 0, 1, 32]]
    _check(sizes, faces, [1, 0], 7, monkeypatch=monkeypatch)
    # the faces at the threshold said twice: 128 raw entries for the same 32 neighbours -- the wave, and not truncated
    twice = np.concatenate([faces[0], faces[0][::-1, ::-1]])
    got = _check([at + 1], [twice], [0], 32, monkeypatch=monkeypatch)
    assert got[1].tolist() == [[2 * at, 0, 0, 32]]
    # 400 raw entries (seven wave steps); the centres are vertices 0, 41, 74, 108 and 309 -- two long rows inside the second
    # wave, short ones around them
    m, many = fans([40, 32, 33, 200, 3])
    for k, truncated in ((32, 3), (6, 4)):
        got = _check([m], [mref.shuffled(many, 7, corners=True, duplicate=0.1)], [0], k, monkeypatch=monkeypatch)
        assert got[1][0, 2] == truncated


def test_ragged_slots(monkeypatch):
    """A scan of 3 vertices and 1 face beside the grid, a scan with a mesh of no faces, scans used in two slots; then a set
    with no faces at all and a NULL faces pointer."""
    tri = np.array([[2, 0, 1]], dtype=np.int32)
    none = np.zeros((0, 3), dtype=np.int32)
    sizes, faces = [M_GRID, 3, 10], [mref.shuffled(_grid(), 8), tri, none]
    got = _check(sizes, faces, [1, 0, 2, 0, 1], 9, monkeypatch=monkeypatch)
    assert got[1].tolist() == [[1, 0, 0, 2], [8192, 0, 0, 6], [0, 0, 0, 0], [8192, 0, 0, 6], [1, 0, 0, 2]]
    assert (got[0][3 + M_GRID:3 + M_GRID + 10] == -1).all()                          # the scan without faces: rows of -1
    # gaps between the slots' rows keep what they held; stats NULL
    gaps = np.array([5, 5 + 3 + 11, 5 + 3 + 11 + M_GRID])
    _check(sizes, faces, [1, 0, 2], 9, out_offsets=gaps, total_out=int(gaps[-1] + 10 + 7))
    full = _raw(sizes, faces, [1, 0, 2], 9)
    assert np.array_equal(_raw(sizes, faces, [1, 0, 2], 9, want_stats=False)[0], full[0])
    got = _check([4, 6], [none, none], [0, 1, 0], 3, null_faces=True)
    assert (got[0] == -1).all() and (got[1] == 0).all()


def test_skipped_slots_are_neither_read_nor_written():
    grid = mref.shuffled(_grid(), 9)
    m_f, f_f = fans([40, 5])
    tri = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int32)
    sizes, faces, ids = [M_GRID, m_f, 4], [grid, f_f, tri], [0, 1, 2]
    others = lambda slot: [s != slot for s in range(3)]          # noqa: E731
    # a scan id outside the set, on either side
    for bad, usable in (([0, -1, 2], others(1)), ([0, 1, 3], others(2)), ([1 << 40, 1, -(1 << 40)], [False, True, False])):
        _check(sizes, faces, bad, 8, usable=usable)
    # The slots on scans 0, 2, 4 of a set with a spare scan behind each, so one scan's end moves without any other slot's
    # pair changing.  A vertex range that is empty, reversed, ends past `total` or starts below zero:
    spare = np.array([[0, 1, 2]], dtype=np.int32)
    s_sizes, s_faces, s_ids = [M_GRID, 5, m_f, 5, 4, 5], [grid, spare, f_f, spare, tri, spare], [0, 2, 4]
    ends = np.concatenate([[0], np.cumsum(s_sizes)])
    for at, value, slot in ((3, ends[2], 1), (3, ends[2] - 5, 1), (5, ends[-1] + 1, 2), (0, -1, 0)):
        offs = ends.copy()
        offs[at] = value
        _check(s_sizes, s_faces, s_ids, 8, usable=others(slot), offsets=offs)
    # a face range that is reversed or starts below zero (the slot's face_out_offsets pair then disagrees as well) ...
    f_ends = np.concatenate([[0], np.cumsum([len(f) for f in s_faces])])
    for at, value, slot in ((3, f_ends[2] - 1, 1), (0, -1, 0)):
        offs = f_ends.copy()
        offs[at] = value
        _check(s_sizes, s_faces, s_ids, 8, usable=others(slot), face_offsets=offs)
    # ... and one that agrees with its pair and fails this rule alone: it ends past total_faces (slot 2 on the set's LAST scan);
    # it starts below zero with the pair saying one face more (which moves the last pair past batch_faces: slot 2 goes too)
    _check(sizes, faces, ids, 8, usable=others(2), total_faces=int(sum(len(f) for f in faces)) - 1)
    true_out = np.concatenate([[0], np.cumsum([len(f) for f in faces])])
    low = true_out.copy()
    low[0] = -1
    _check(sizes, faces, ids, 8, usable=[False, True, False], face_offsets=low, told_face_out=true_out + np.array([0, 1, 1, 1]))
    # a face_out_offsets pair that disagrees with the slot's face range: an entry in the middle spoils both its pairs; the last
    # one past batch_faces; the first one negative; a pair in the wrong order
    for at, value, usable in ((1, true_out[1] + 1, [False, False, True]), (3, true_out[3] + 1, others(2)), (0, -1, others(0)),
                              (2, true_out[1] - 1, [True, False, False])):
        told = true_out.copy()
        told[at] = value
        _check(sizes, faces, ids, 8, usable=usable, told_face_out=told)
    # an out_offsets entry that is negative or leaves no room for the slot's rows: one row too far is enough
    packed = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    for slot, o in ((0, -1), (2, sum(sizes) - 3), (1, sum(sizes) - m_f + 1), (1, 1 << 50)):
        told = packed.copy()
        told[slot] = o
        _check(sizes, faces, ids, 8, usable=others(slot), told_out=told)


def test_faces_with_indices_outside_the_scan_are_ignored_and_counted(monkeypatch):
    """Indices -1, M, 2^31 - 1 and -2^31 at every corner, and repeated indices along edges the grid has: the table is the
    grid's own, the stats count what was ignored.  The kernel checks the bounds before any use."""
    rng = np.random.default_rng(10)
    grid = _grid()
    junk = []
    for value in (-1, M_GRID, 2 ** 31 - 1, -2 ** 31, M_GRID + 1, -7):
        for corner in range(3):
            for _ in range(20):
                face = rng.integers(0, M_GRID, size=3)
                face[corner] = value
                junk.append(face)
    junk.append(np.array([2 ** 31 - 1] * 3))
    junk.append(np.array([-1, M_GRID, -1]))
    v = rng.integers(0, M_GRID - 1, size=50)
    v = v[v % R != R - 1]                                    # v and v + 1 are joined by the grid
    repeated = np.concatenate([np.stack([v, v, v + 1], 1), np.stack([v + 1, v, v + 1], 1), np.stack([v, v, v], 1)])
    faces = mref.shuffled(np.concatenate([grid, np.asarray(junk), repeated]), 11, corners=True)
    clean = _check([M_GRID], [grid], [0], 8)
    got = _check([M_GRID, 3], [faces, faces[:40]], [0, 1], 8, monkeypatch=monkeypatch)
    assert np.array_equal(got[0][:M_GRID], clean[0]) and got[1][0].tolist() == [8192 + len(repeated), len(junk), 0, 6]
    assert got[1][1, 0] + got[1][1, 1] == 40 and got[1][1, 1] > 30          # the same faces on a scan of 3 vertices: most are outside


def test_one_capture_holds_kernel_nodes_only_and_replays_to_the_eager_bits():
    from geot_amd import _lib, streams
    from geot_amd.ext._common import call, ptr
    m_f, f_f = fans([40, 33, 5])
    sizes, faces, k = [M_GRID, m_f], [mref.shuffled(_grid(), 12, corners=True), f_f], 16
    eager = _raw(sizes, faces, [1, 0], k)
    counts = [len(faces[1]), len(faces[0])]
    total_out, batch_faces = m_f + M_GRID, sum(counts)
    nbytes = int(_lib.load().geot_mesh_neighbours_ws_bytes(2, total_out, batch_faces))
    to = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)      # noqa: E731
    held = {"faces": to(np.concatenate(faces), np.int32), "offsets": to([0, M_GRID, M_GRID + m_f], np.int64),
            "face_offsets": to([0, counts[1], counts[1] + counts[0]], np.int64), "ids": to([1, 0], np.int64),
            "out": to([0, m_f], np.int64), "face_out": to([0, counts[0], batch_faces], np.int64),
            "nbr": torch.full((total_out, k), NBR_FILL, dtype=torch.int32, device=DEV),
            "stats": torch.full((2, 4), STAT_FILL, dtype=torch.int32, device=DEV),
            "ws": torch.empty(nbytes, dtype=torch.uint8, device=DEV)}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with streams.capture(graph, DEV):
        call("geot_mesh_neighbours", DEV, 2, k, 2, M_GRID + m_f, batch_faces, ptr(held["faces"]), ptr(held["offsets"]),
             ptr(held["face_offsets"]), ptr(held["ids"]), ptr(held["out"]), ptr(held["face_out"]), batch_faces, ptr(held["nbr"]),
             ptr(held["stats"]), ptr(held["ws"]), nbytes)
    kinds = streams.node_types(graph)
    assert set(kinds) == {"kernel"} and kinds["kernel"] == 7, kinds
    for _ in range(2):
        held["nbr"].fill_(NBR_FILL)
        held["stats"].fill_(STAT_FILL)
        held["ws"].random_(0, 256)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(held["nbr"].cpu().numpy(), eager[0]) and np.array_equal(held["stats"].cpu().numpy(), eager[1])
