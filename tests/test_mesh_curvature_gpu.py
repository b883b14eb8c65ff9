"""The mesh-curvature entry points (csrc/mesh_curvature.hip) through the C ABI against the numpy restatement
(tests/_curvature_ref.py): array_equal over the WHOLE buffers, in guarded arenas -- every output, the inputs and the workspace
lie between guard elements that are compared afterwards; the workspace arrives full of noise.  Defects: the octahedron, a 65 x 65
height field (more than one workgroup of faces) said in three ways, 200 atomics on one word, ragged and skipped slots, junk and
repeated indices, a zero-length edge and a NaN vertex, the stats of all of them, every call made twice.  Ball sums of hand-made
64-bit values: the closed ball at d2 == r2 on a lattice, a radius below the spacing and one covering the scan, fine and coarse
grids, M in {1, 63, 65, 4225}, values of both signs near 2^40, both forms.  The range keys and the sample launch.  The curvature
of the height field against an independent float64 computation.  One capture."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _curvature_ref as cref  # noqa: E402
import _mesh_ref as mref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DQ_FILL, STAT_FILL, OUT_FILL, KEY_FILL, GUARD_FILL = -(7 << 40) - 5, -5, -777.5, 0x12345678, 0x5a
GUARD = 64                                                   # guard elements on either side of every arena


class Arena:
    """n elements between two guards; `inner` is what the call is given."""

    def __init__(self, values, dtype, fill=GUARD_FILL):
        values = np.ascontiguousarray(np.asarray(values).astype(dtype)).reshape(-1)
        host = np.full(values.size + 2 * GUARD, fill, dtype=dtype)
        host[GUARD:GUARD + values.size] = values
        self.n, self.before = values.size, host.copy()
        self.whole = torch.from_numpy(host).to(DEV)
        self.inner = self.whole[GUARD:GUARD + self.n]

    def ptr(self):
        return self.inner.data_ptr()

    def intact(self, whole=False):
        """The guards are as they were (whole=True: the inner elements too: an input)."""
        host = self.whole.cpu().numpy()
        same = lambda a, b: a.tobytes() == b.tobytes()              # noqa: E731  (NaN inputs compare by their bytes)
        if whole:
            return same(host, self.before)
        return same(host[:GUARD], self.before[:GUARD]) and same(host[GUARD + self.n:], self.before[GUARD + self.n:])

    def host(self):
        return self.inner.cpu().numpy()


def _noise(nbytes, seed):
    return Arena(np.random.default_rng(seed).integers(0, 256, size=nbytes), np.uint8, fill=0xa5)


# ---- defects ---------------------------------------------------------------------------------------------------------------------
def _defects_raw(set_points, set_faces, ids, out_offsets, total_out, want_stats=True):
    """geot_mesh_angle_defects on slots `ids` of a set -> (defect_q (total_out,) int64, stats (b, 4) or None), the whole buffers."""
    from geot_amd import _lib
    from geot_amd.ext._common import call
    b, n = len(ids), len(set_points)
    sizes = [len(p) for p in set_points]
    counts = [len(set_faces[i]) if 0 <= i < n else 0 for i in ids]
    face_out = np.concatenate([[0], np.cumsum(counts)])
    a_points = Arena(np.concatenate(set_points), np.float32)
    a_faces = Arena(np.concatenate([np.asarray(f, dtype=np.int64).reshape(-1, 3) for f in set_faces]), np.int32)
    a_dq = Arena(np.full(total_out, DQ_FILL), np.int64)
    a_stats = Arena(np.full(b * 4, STAT_FILL), np.int32)
    nbytes = int(_lib.load().geot_mesh_angle_defects_ws_bytes(total_out))
    a_ws = _noise(nbytes, nbytes)
    assert nbytes > 0 and a_ws.ptr() % 16 == 0
    d = [torch.from_numpy(np.asarray(x, dtype=np.int64)).to(DEV) for x in
         (np.concatenate([[0], np.cumsum(sizes)]), np.concatenate([[0], np.cumsum([len(f) for f in set_faces])]), ids, out_offsets, face_out)]
    call("geot_mesh_angle_defects", DEV, b, n, int(sum(sizes)), a_faces.n // 3, a_points.ptr(), a_faces.ptr(), d[0].data_ptr(),
         d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), int(face_out[-1]), total_out, a_dq.ptr(),
         a_stats.ptr() if want_stats else None, a_ws.ptr(), nbytes)
    torch.cuda.synchronize()
    assert a_points.intact(True) and a_faces.intact(True) and a_dq.intact() and a_stats.intact(not want_stats) and a_ws.intact(), \
        "a guard element or an input was written"
    return a_dq.host(), a_stats.host().reshape(b, 4) if want_stats else None


def _defects(set_points, set_faces, ids=None, out_offsets=None, total_out=None, usable=None):
    """One call against the restatement over the whole buffers, and a second call: the same bits.  usable[s] False: the slot
    must be skipped (rows untouched, stats zero)."""
    n = len(set_points)
    ids = list(range(n)) if ids is None else ids
    usable = [True] * len(ids) if usable is None else usable
    lens = [len(set_points[i]) if 0 <= i < n else 0 for i in ids]
    if out_offsets is None:
        out_offsets = np.concatenate([[0], np.cumsum(lens)[:-1]])
    total_out = int(sum(lens)) if total_out is None else total_out
    e_dq, e_stats = np.full(total_out, DQ_FILL, dtype=np.int64), np.zeros((len(ids), 4), dtype=np.int32)
    for s, (i, o) in enumerate(zip(ids, out_offsets)):
        if usable[s]:
            e_dq[o:o + lens[s]], e_stats[s] = cref.defects_q(set_points[i], set_faces[i])
    got = _defects_raw(set_points, set_faces, ids, out_offsets, total_out)
    print("sizes %s: stats (usable, ignored, degenerate, lonely) %s" % (lens, got[1].tolist()))
    assert np.array_equal(got[1], e_stats), (got[1].tolist(), e_stats.tolist())
    assert np.array_equal(got[0], e_dq), int((got[0] != e_dq).sum())
    again = _defects_raw(set_points, set_faces, ids, out_offsets, total_out)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
    bare = _defects_raw(set_points, set_faces, ids, out_offsets, total_out, want_stats=False)
    assert np.array_equal(bare[0], got[0]) and bare[1] is None
    return got


R = 65                                  # 65 x 65 vertices: 4 225; 8 192 faces: 32 workgroups of faces
SEED, RADIUS = 1, 1.3                   # no pair of vertices within a relative 2^-18 of the radius (asserted below)
_kept = {}


def _field():
    if "field" not in _kept:
        _kept["field"] = (cref.height_field(R, R, SEED), mref.grid(R, R))
    return _kept["field"]


def _fan(rim, lift=0.3):
    ang = 2 * np.pi * np.arange(rim) / rim
    pts = np.concatenate([[[0, 0, lift]], np.stack([np.cos(ang), np.sin(ang), np.zeros(rim)], 1)]).astype(np.float32)
    return pts, mref.fan(rim)


def test_the_octahedron():
    v, f = cref.octahedron()
    got = _defects([v], [f])
    assert got[1].tolist() == [[8, 0, 0, 0]]
    assert abs(got[0].sum() / cref.Q - 4 * np.pi) <= 24 * cref.ANGLE_BOUND + 24 * 2.0 ** -33


def test_the_height_field_said_in_three_ways_gives_the_same_bits():
    pts, faces = _field()
    assert faces.shape == (8192, 3) and len(pts) == 4225
    plain = _defects([pts], [faces])
    shuffled = _defects([pts], [mref.shuffled(faces, 1)])
    turned = _defects([pts], [mref.shuffled(faces, 2, corners=True)])
    assert plain[1].tolist() == [[8192, 0, 0, 0]]
    assert np.array_equal(shuffled[0], plain[0]) and np.array_equal(turned[0], plain[0])
    assert np.array_equal(shuffled[1], plain[1]) and np.array_equal(turned[1], plain[1])
    # duplicates count twice: another result, and again the restatement's
    twice = _defects([pts], [mref.shuffled(faces, 3, corners=True, duplicate=0.1)])
    assert twice[1].tolist() == [[8192 + 819, 0, 0, 0]] and not np.array_equal(twice[0], plain[0])


def test_two_hundred_atomics_on_one_word():
    pts, faces = _fan(200)
    got = _defects([pts], [mref.shuffled(faces, 4, corners=True)])
    assert got[1].tolist() == [[200, 0, 0, 0]]
    assert got[0][0] < 0.5 * cref.Q2PI and (got[0][1:] > 0).all()         # 200 angles summed at the centre


def test_ragged_slots_and_a_skipped_one():
    o_v, o_f = cref.octahedron()
    h_v, h_f = cref.height_field(9, 7, 3), mref.grid(9, 7)
    f_v, f_f = _fan(40)
    pts, faces = [o_v, h_v, f_v], [o_f, h_f, f_f]
    # slots in another order than the set, with gaps between their rows; scan 7 is outside the set: skipped
    _defects(pts, faces, ids=[2, 7, 0, 1], out_offsets=[70, 0, 3, 120], total_out=200, usable=[True, False, True, True])
    # a slot that does not fit total_out, and one before row 0: skipped, nothing of them is written
    _defects(pts, faces, ids=[1, 0, 2], out_offsets=[0, 195, -1], total_out=200, usable=[True, False, False])
    # the same scan in two slots
    _defects(pts, faces, ids=[0, 0], out_offsets=[10, 0], total_out=16)


def test_junk_and_repeated_indices_a_zero_length_edge_and_a_nan_vertex():
    pts, faces = cref.height_field(9, 9, 5), mref.grid(9, 9)
    clean = _defects([pts], [faces])
    junk = np.array([[0, 1, 81], [-1, 2, 3], [5, 5, 6], [7, 8, 7], [2 ** 31 - 1, 0, 1], [-2 ** 31, 4, 5], [9, 9, 9]])
    mixed = np.concatenate([faces[:30], junk, faces[30:]])
    got = _defects([pts], [mixed])
    assert got[1].tolist() == [[128, 7, 0, 0]] and np.array_equal(got[0], clean[0])
    broken = pts.copy()
    broken[40] = broken[41]                     # a zero-length edge in every face that holds both
    broken[10, 1] = np.nan
    broken[70, 2] = np.inf
    got = _defects([broken], [mixed])
    assert got[1][0, 2] > 10 and got[1][0, :2].tolist() == [128, 7]
    assert (got[0][[10, 70]] == cref.Q2PI).all()        # every face at a non-finite vertex is degenerate: no angle at all
    # a scan whose only faces are ignored ones: every vertex is in no usable face
    got = _defects([pts], [junk])
    assert got[1].tolist() == [[0, 7, 0, 81]] and (got[0] == cref.Q2PI).all()


# ---- ball sum --------------------------------------------------------------------------------------------------------------------
def _ball_raw(points, value, radius):
    from geot_amd import _lib
    from geot_amd.ext._common import call
    m = len(points)
    a_points, a_value = Arena(points, np.float32), Arena(value, np.int64)
    a_out, a_keys = Arena(np.full(m, OUT_FILL), np.float32), Arena(np.full(2, KEY_FILL), np.uint32)
    nbytes = int(_lib.load().geot_scan_ball_sum_ws_bytes(m))
    a_ws = _noise(nbytes, m)
    assert nbytes > 0 and a_ws.ptr() % 16 == 0
    call("geot_scan_ball_sum", DEV, m, float(radius), a_points.ptr(), a_value.ptr(), a_out.ptr(), a_keys.ptr(), a_ws.ptr(), nbytes)
    torch.cuda.synchronize()
    assert a_points.intact(True) and a_value.intact(True) and a_out.intact() and a_keys.intact() and a_ws.intact(), \
        "a guard element or an input was written"
    return a_out.host(), a_keys.host()


def _ball(points, value, radius, monkeypatch, inside=None):
    """Both forms, each twice, against the restatement: out bit for bit and the two range keys."""
    e_out, sums, e_rng = cref.ball_sum(points, value, radius, inside)
    got = _ball_raw(points, value, radius)
    assert np.array_equal(got[0], e_out), int((got[0] != e_out).sum())
    assert got[1].tolist() == cref.ord_keys(e_rng).tolist()
    again = _ball_raw(points, value, radius)
    monkeypatch.setenv("GEOT_BALL_SUM_IMPL", "basic")
    plain = _ball_raw(points, value, radius)
    monkeypatch.delenv("GEOT_BALL_SUM_IMPL")
    for other in (again, plain):
        assert np.array_equal(other[0], got[0]) and np.array_equal(other[1], got[1])
    return got[0], sums


def _values(m, seed):
    """Values of both signs near 2^40, no two alike."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-2 ** 40, 2 ** 40, size=m) | 1) * np.where(np.arange(m) % 2 == 0, 1, -1)


def test_the_closed_ball_on_a_lattice(monkeypatch):
    """Pitch 0.125, radius 0.125: d2 == r2 exactly for the four neighbours, which are inside; the grid's z-dimension is 1."""
    g = 9
    pts = mref.grid_points(g, g) * np.float32(0.125)
    ones = np.full(g * g, 1 << 32, dtype=np.int64)
    out, _ = _ball(pts, ones, 0.125, monkeypatch)
    count = out.reshape(g, g)
    assert (count[1:-1, 1:-1] == 5).all() and count[0, 0] == count[0, -1] == count[-1, 0] == count[-1, -1] == 3
    assert (count[0, 1:-1] == 4).all() and (count[1:-1, 0] == 4).all()
    _ball(pts, _values(g * g, 1), 0.125, monkeypatch)
    # a radius below the smallest spacing: the vertex's own value, bit for bit
    value = _values(g * g, 2)
    out, _ = _ball(pts, value, 0.1, monkeypatch)
    assert np.array_equal(out, (value.astype(np.float64) / cref.Q).astype(np.float32))
    # a radius covering the scan: a single cell, every vertex the total
    out, sums = _ball(pts, value, 4.0, monkeypatch)
    assert (sums == value.sum()).all() and (out == out[0]).all()


@pytest.mark.parametrize("m", [1, 63, 65, 4225])
def test_fine_and_coarse_grids_at_every_size(m, monkeypatch):
    rng = np.random.default_rng(m)
    pts = (rng.random((m, 3)) * 10).astype(np.float32)
    value = _values(m, m + 1)
    # extent / radius below 32: the cell edge is just above the radius; members in all 26 outer cells of some block
    radius = 1.0
    inside = cref.members(pts, radius)
    if m == 4225:
        ext = (pts.max(0) - pts.min(0)).max()
        cells = int(ext / (radius * 1.0001))
        assert 1 < cells < 32
        cell = np.minimum(((pts - pts.min(0)) * (cells / ext)).astype(np.int64), cells - 1)
        v, u = np.nonzero(inside)
        assert len({tuple(d) for d in (cell[u] - cell[v])}) == 27             # the centre cell and all 26 around it
    _ball(pts, value, radius, monkeypatch, inside)
    # extent / radius above 32: coarse cells of extent / 32, many candidates for a handful of members -- the workload's regime
    radius = 0.2
    assert (pts.max(0) - pts.min(0)).max() / radius > 32 or m == 1
    _ball(pts, value, radius, monkeypatch)
    # a flat scan, vertices that coincide and a non-finite one: in nobody's ball, its own included
    if m >= 63:
        flat = pts.copy()
        flat[:, 2] = 0
        flat[5], flat[7, 0], flat[9, 1] = flat[6], np.nan, np.inf
        out, sums = _ball(flat, value, 0.7, monkeypatch)
        assert sums[7] == 0 and sums[9] == 0 and out[7] == 0 and sums[5] == sums[6]


# ---- range and sample ------------------------------------------------------------------------------------------------------------
def _sample_raw(cur, keys, sizes, ids, sel):
    from geot_amd.ext._common import call
    s, m = sel.shape
    a_cur, a_keys, a_sel = Arena(cur, np.float32), Arena(keys, np.uint32), Arena(sel, np.int64)
    a_out, a_bad = Arena(np.full(s * m, OUT_FILL), np.float32), Arena(np.full(s, STAT_FILL), np.int32)
    d = [torch.from_numpy(np.asarray(x, dtype=np.int64)).to(DEV) for x in (np.concatenate([[0], np.cumsum(sizes)]), ids)]
    call("geot_curvature_sample", DEV, s, m, len(sizes), int(sum(sizes)), a_cur.ptr(), a_keys.ptr(), d[0].data_ptr(), d[1].data_ptr(),
         a_sel.ptr(), a_out.ptr(), a_bad.ptr())
    torch.cuda.synchronize()
    assert a_cur.intact(True) and a_keys.intact(True) and a_sel.intact(True) and a_out.intact() and a_bad.intact()
    return a_out.host().reshape(s, m), a_bad.host()


def test_the_range_keys_and_the_sample_launch():
    rng = np.random.default_rng(8)
    sizes = [50, 1, 2100, 30]
    curs = [rng.normal(size=n).astype(np.float32) * 5 for n in sizes]
    curs[3][:] = -2.5                                   # a constant scan: 0 everywhere, not NaN
    ranges = [np.array([np.abs(c).min(), np.abs(c).max()], dtype=np.float32) for c in curs]
    keys = np.concatenate([cref.ord_keys(r) for r in ranges])
    m = 1500                                            # more than one pass of the workgroup
    ids = [2, 0, 3, 1, 2, 9, -1]
    sel = np.stack([rng.integers(0, sizes[i] if 0 <= i < 4 else 5, size=m) for i in ids])
    sel[0, :6] = [0, 0, 2099, 2099, 7, 7]               # first, last, repeated
    sel[0, 6:8] = [np.abs(curs[2]).argmax(), np.abs(curs[2]).argmin()]
    sel[1, :4] = [-1, 50, 2 ** 40, 49]                  # outside the scan: 0, flagged, never an address
    sel[4, -1] = 2100
    got, bad = _sample_raw(np.concatenate(curs), keys, sizes, ids, sel)
    assert bad.tolist() == [0, 1, 0, 0, 1, 2, 2]
    for slot, i in enumerate(ids):
        if not 0 <= i < 4:
            assert (got[slot] == 0).all()
            continue
        ok = (sel[slot] >= 0) & (sel[slot] < sizes[i])
        want = np.zeros(m, dtype=np.float32)
        want[ok] = cref.normalise(curs[i], ranges[i], sel[slot][ok])
        assert np.array_equal(got[slot], want), slot
    assert (got[2] == 0).all() and (got[3] == 0).all() and got[0].max() == 1 and got[0].min() == 0
    again, bad2 = _sample_raw(np.concatenate(curs), keys, sizes, ids, sel)
    assert np.array_equal(again, got) and np.array_equal(bad2, bad)


# ---- the whole definition, through the scan set --------------------------------------------------------------------------------
def _set():
    if "set" not in _kept:
        from geot_amd.openpoints.dataset import DeviceScanSet
        pts, faces = _field()
        o_v, o_f = cref.octahedron()
        scans = [pts, o_v * np.float32(3), cref.height_field(9, 7, 3)]
        labels = [np.zeros(len(p), dtype=np.int32) for p in scans]
        _kept["scans"], _kept["meshes"] = scans, [mref.shuffled(faces, 6, corners=True), o_f, None]
        _kept["set"] = DeviceScanSet(scans, labels, device=DEV, faces=_kept["meshes"])
        _kept["inside"] = cref.members(pts, RADIUS)
    return _kept["set"]


def test_compute_curvature_is_the_restatement_and_within_its_bound_of_float64():
    from geot_amd.openpoints.dataset import mesh_curvature
    from geot_amd.openpoints.dataset import DeviceScanSet
    dset = _set()
    pts, faces = _field()
    fresh = DeviceScanSet(_kept["scans"][1:2], [np.zeros(6, dtype=np.int32)], device=DEV, faces=_kept["meshes"][1:2])
    assert fresh.curvature is None and fresh.curvature_range is None and fresh.defects is None and fresh.curvature_radius is None
    st = dset.compute_curvature(RADIUS, stats=True)
    assert st.cpu().tolist() == [[8192, 0, 0, 0], [8, 0, 0, 0]] and dset.curvature_radius == RADIUS
    cur, rng, dq, _ = cref.curvature(pts, _kept["meshes"][0], RADIUS, _kept["inside"])
    o_cur, o_rng, o_dq, _ = cref.curvature(_kept["scans"][1], _kept["meshes"][1], RADIUS)
    got = dset.curvature.cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got[:4225], cur) and np.array_equal(got[4225:4231], o_cur)
    assert (got[4231:] == 0).all() and (dset.defects.cpu().numpy()[4231:] == 0).all()              # the scan without a mesh
    assert np.array_equal(dset.defects.cpu().numpy()[:4231], np.concatenate([dq, o_dq]))
    assert np.array_equal(dset.curvature_range.cpu().numpy(), np.stack([rng, o_rng, [0, 0]]).astype(np.float32))
    assert o_rng[0] == o_rng[1]                                          # a radius below the octahedron's edge: all alike
    views = mesh_curvature(dset, RADIUS)
    assert [tuple(v.shape) for v in views] == [(4225,), (6,), (63,)] and views[0].data_ptr() == dset.curvature.data_ptr()
    assert dset.compute_curvature(RADIUS) is dset and np.array_equal(dset.curvature.cpu().numpy(), got)      # the same bits
    # against the independent float64 computation: no pair of vertices so close to the radius that membership could differ
    assert cref.near_the_radius(pts, RADIUS) == 0
    want, members, load = cref.curvature_f64(pts, faces, RADIUS)
    assert np.array_equal(members, _kept["inside"].sum(1))
    valence = np.bincount(faces.reshape(-1), minlength=4225)
    tol = members * valence.max() * cref.ANGLE_BOUND
    diff = np.abs(cur.astype(np.float64) - want)
    print("curvature %.4g .. %.4g, members %d .. %d: max |gpu - f64| = %.3g, smallest tolerance %.3g"
          % (want.min(), want.max(), members.min(), members.max(), diff.max(), tol.min()))
    assert (diff <= tol).all()
    # another radius recomputes
    dset.compute_curvature(0.5)
    assert dset.curvature_radius == 0.5 and not np.array_equal(dset.curvature.cpu().numpy()[:4225], cur)
    assert np.array_equal(dset.curvature.cpu().numpy()[:4225], cref.curvature(pts, faces, 0.5)[0])
    dset.compute_curvature(RADIUS)


def test_merged_sets_carry_the_curvature_only_with_one_radius():
    from geot_amd.openpoints.dataset import DeviceScanSet
    dset = _set()
    dset.compute_curvature(RADIUS)
    other = DeviceScanSet(_kept["scans"][1:2], [np.zeros(6, dtype=np.int32)], device=DEV, faces=_kept["meshes"][1:2])
    assert DeviceScanSet._merged(dset, other).curvature is None                      # one side has none
    other.compute_curvature(0.5)
    assert DeviceScanSet._merged(dset, other).curvature is None                      # two radii
    other.compute_curvature(RADIUS)
    both = DeviceScanSet._merged(dset, other)
    assert both.curvature_radius == RADIUS and torch.equal(both.curvature, torch.cat([dset.curvature, other.curvature]))
    assert torch.equal(both.curvature_range, torch.cat([dset.curvature_range, other.curvature_range]))
    assert torch.equal(both.defects, torch.cat([dset.defects, other.defects])) and both._curvature_keys.shape == (4, 2)


def test_one_capture_holds_kernel_nodes_only_and_replays_to_the_eager_bits():
    """compute_curvature (its slot tables are on the device after the first call) and the launch a batch adds."""
    from geot_amd import streams
    from geot_amd.openpoints.dataset.scan_set import curvature_sample
    dset = _set()
    dset.compute_curvature(RADIUS)
    ids = torch.tensor([1, 0, 0], dtype=torch.int64, device=DEV)
    sel = torch.from_numpy(np.random.default_rng(3).integers(0, 6, size=(3, 500))).to(DEV)
    eager_cur = dset.curvature.clone()
    eager, eager_bad = curvature_sample(dset, ids, sel)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with streams.capture(graph, DEV):
        dset.compute_curvature(RADIUS)
        out, bad = curvature_sample(dset, ids, sel)
    kinds = streams.node_types(graph)
    assert set(kinds) == {"kernel"} and kinds["kernel"] >= 3 + 2 * 7 + 1, kinds
    for _ in range(2):
        dset.curvature.fill_(-1)
        out.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dset.curvature, eager_cur) and torch.equal(out, eager) and torch.equal(bad, eager_bad)
