"""Mesh curvature, the part that needs no GPU: the numpy restatement the GPU tests compare against (tests/_curvature_ref.py) held
against an independent float64 computation and against closed meshes whose total defect is known (4 pi for genus 0, 0 for a
torus, pi / 2 at every corner of a cube); its invariance under reordering; the ABI and the binding of the three entry points and
their refusals before any launch; the Python refusals that come before any device call."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _curvature_ref as cref  # noqa: E402
import _mesh_ref as mref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_PI_Q = 2.0 * np.pi * cref.Q


def _rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)


def test_the_float32_angle_stays_within_its_bound_of_float64_whatever_the_conditioning():
    """Edge lengths 1e-2 .. 1e1, coordinates up to 1e2, angles 1e-3 .. pi - 1e-3, any orientation: the restated angle against
    np.arctan2 in float64 on the SAME float32 coordinates, within ANGLE_BOUND (absolute; derived in _curvature_ref by operation
    count before any difference was looked at)."""
    rng = np.random.default_rng(11)
    n = 300000
    l1, l2 = (10.0 ** rng.uniform(-2, 1, size=n) for _ in range(2))
    theta = np.exp(rng.uniform(np.log(1e-3), np.log(np.pi / 2), size=n))
    theta = np.where(rng.random(n) < 0.5, theta, np.pi - theta)                     # both ends of (0, pi) alike
    theta[:4] = [1e-3, np.pi - 1e-3, np.pi / 2, np.pi / 4]
    rot = _rotations(rng, n)
    e1 = np.einsum("nij,nj->ni", rot, np.stack([l1, np.zeros(n), np.zeros(n)], 1))
    e2 = np.einsum("nij,nj->ni", rot, np.stack([l2 * np.cos(theta), l2 * np.sin(theta), np.zeros(n)], 1))
    a = rng.uniform(-1, 1, size=(n, 3)) * (10.0 ** rng.uniform(-2, 2, size=(n, 1)))
    a = np.clip(a, -89, 89)                                                         # corners stay inside 1e2
    a, b, c = (v.astype(np.float32) for v in (a, a + e1, a + e2))
    assert max(np.abs(v).max() for v in (a, b, c)) <= 100
    for first, others in ((a, (b, c)), (b, (c, a)), (c, (a, b))):                   # every corner: small, large and middling angles
        got = cref.corner_angles_f32(first, *others)
        want = cref.corner_angles_f64(first, *others)
        assert got.dtype == np.float32 and np.isfinite(got).all() and got.min() >= 0 and got.max() <= np.float32(np.pi)
        diff = np.abs(got.astype(np.float64) - want)
        print("angles %.3g .. %.3g rad: max |f32 - f64| = %.3g rad (bound %.3g)" % (want.min(), want.max(), diff.max(), cref.ANGLE_BOUND))
        assert diff.max() <= cref.ANGLE_BOUND
        assert np.array_equal(got, cref.corner_angles_f32(first, *others[::-1]))    # the two others swapped: the same bits
    assert cref.corner_angles_f64(a, b, c).min() < 2e-3 and cref.corner_angles_f64(a, b, c).max() > np.pi - 2e-3


def test_the_atan2_by_hand():
    f = np.float32
    got = cref.atan2_f32(f([0, 0, 1, 1, 1, 0, np.inf, np.nan, 1, 3e38]), f([0, 1, 0, 1, -1, -1, 1, 1, np.inf, -3e38]))
    want = [0, 0, np.pi / 2, np.pi / 4, 3 * np.pi / 4, np.pi, 0, 0, 0, 3 * np.pi / 4]
    assert np.abs(got - np.array(want)).max() <= 4e-7 and got[0] == 0 and got[1] == 0 and got[6] == 0 and got[7] == 0 and got[8] == 0
    assert cref.PI_HI == f(np.pi) and abs(float(cref.PI_HI) + float(cref.PI_LO) - np.pi) < 1e-14
    assert cref.Q2PI == 26986075409 and cref.TAN_PIO8 < np.tan(np.pi / 8) + 1e-7
    # the polynomial's truncation: the first term left out on the reduced range
    assert float(cref.TAN_PIO8) ** 21 / 21 < 4.5e-10


CLOSED = {"octahedron": (cref.octahedron, 4 * np.pi), "icosphere": (lambda: cref.icosphere(2), 4 * np.pi),
          "torus": (lambda: cref.torus(16), 0.0), "cube": (cref.cube, 4 * np.pi)}


@pytest.mark.parametrize("name", sorted(CLOSED))
def test_closed_meshes_have_their_total_defect(name):
    make, total = CLOSED[name]
    v, f = make()
    faces = len(f)
    assert {"octahedron": (6, 8), "icosphere": (162, 320), "torus": (256, 512), "cube": (8, 12)}[name] == (len(v), faces)
    tol = 3 * faces * cref.ANGLE_BOUND + 3 * faces * 2.0 ** -33
    dq, stats = cref.defects_q(v, f)
    assert stats == [faces, 0, 0, 0] and dq.dtype == np.int64
    assert abs(dq.sum() / cref.Q - total) <= tol, (dq.sum() / cref.Q, total, tol)
    if name == "cube":
        assert np.abs(dq / cref.Q - np.pi / 2).max() <= tol
    if name == "octahedron":
        assert np.abs(dq / cref.Q - 2 * np.pi / 3).max() <= tol             # four angles of pi / 3 at every vertex
    assert np.abs(dq / cref.Q - cref.defects_f64(v, f)).max() <= 12 * cref.ANGLE_BOUND + 2.0 ** -30      # valence <= 8 here
    # a radius spanning the mesh: every vertex's curvature is the total
    cur, rng, _, _ = cref.curvature(v, f, 10.0)
    assert np.abs(cur.astype(np.float64) - total).max() <= tol + 2.0 ** -22 and (cur == cur[0]).all()
    assert rng[0] == rng[1] == abs(cur[0]) and (cref.normalise(cur, rng) == 0).all()       # max == min: 0, not NaN
    # a radius below every edge: the vertex's own defect
    own, rng, _, _ = cref.curvature(v, f, 1e-3)
    assert np.array_equal(own, (dq.astype(np.float64) / cref.Q).astype(np.float32))
    if name != "cube" and name != "octahedron":
        norm = cref.normalise(own, rng)
        assert norm.min() == 0 and norm.max() == 1 and norm.dtype == np.float32
    else:
        assert rng[1] - rng[0] <= 1e-5


def test_the_result_depends_on_the_multiset_of_faces_alone():
    v, f = cref.icosphere(1)
    dq, stats = cref.defects_q(v, f)
    for seed in (1, 2):
        other, st = cref.defects_q(v, mref.shuffled(f, seed, corners=True))
        assert np.array_equal(other, dq) and st == stats
    # a duplicated face doubles its angles: the defects of its corners fall by exactly the face's quantised angles
    twice, st = cref.defects_q(v, np.concatenate([f, f[:1]]))
    a, b, c = v[f[0]][:, None, :]
    q = [int(np.rint(float(cref.corner_angles_f32(*order)[0]) * cref.Q)) for order in ((a, b, c), (b, c, a), (c, a, b))]
    want = dq.copy()
    want[f[0]] -= q
    assert np.array_equal(twice, want) and st == [len(f) + 1, 0, 0, 0]
    # all faces twice: every defect is Q2PI - 2 (Q2PI - defect)
    assert np.array_equal(cref.defects_q(v, np.concatenate([f, f[::-1, ::-1]]))[0], cref.Q2PI - 2 * (cref.Q2PI - dq))


def test_the_face_rules_by_hand():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0], [np.nan, 0, 0], [5, 5, 5]], dtype=np.float32)
    # one right triangle; vertices 3, 4, 5 are in no face: 2 pi
    dq, st = cref.defects_q(v, [[0, 1, 2]])
    assert st == [1, 0, 0, 3] and (dq[3:] == cref.Q2PI).all()
    assert np.abs(dq[:3] / cref.Q - (2 * np.pi - np.array([np.pi / 2, np.pi / 4, np.pi / 4]))).max() <= cref.ANGLE_BOUND + 2.0 ** -32
    # junk and repeated indices: ignored as a whole; a zero-length edge (1 and 3 coincide) and a NaN corner: three zero angles
    dq2, st = cref.defects_q(v, [[0, 1, 2], [0, 1, 6], [-1, 1, 2], [0, 0, 2], [2 ** 31 - 1, 0, 1], [0, 1, 3], [0, 4, 2]])
    assert st == [3, 4, 2, 1] and np.array_equal(dq2, dq)
    # the ball: a NaN vertex is in nobody's ball, its own included; coincident vertices are in each other's
    inside = cref.members(v, 0.5)
    assert not inside[4].any() and not inside[:, 4].any() and inside[1, 3] and inside[3, 1] and inside[5].sum() == 1
    out, sums, rng = cref.ball_sum(v, np.array([1, 2, 3, 4, 5, -7], dtype=np.int64) << 32, 0.5)
    assert out.tolist() == [1, 6, 3, 6, 0, -7] and rng.tolist() == [0, 7]
    assert cref.ord_keys(rng).tolist() == [0x80000000, 0x80000000 | np.float32(7).view(np.uint32)]
    # the closed ball: d2 == r2 is inside
    lattice = mref.grid_points(3, 3) * np.float32(0.125)
    assert cref.members(lattice, 0.125).sum(1).tolist() == [3, 4, 3, 4, 5, 4, 3, 4, 3]
    # normalisation by hand
    assert cref.normalise(np.float32([-3, 1, 2]), np.float32([1, 3]), [0, 1, 2, 2]).tolist() == [1, 0, 0.5, 0.5]


def test_abi_version_signatures_and_exports():
    from geot_amd import _header, _lib, build
    from geot_amd.openpoints import dataset
    from geot_amd.openpoints.dataset import scan_set
    build.build()
    hdr = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    assert int(re.search(r"GEOT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 37
    entries, constants = _header.parse()
    names = {e.name: e for e in entries}
    assert constants["GEOT_CURVATURE_MAX_SCAN"] == 1 << 24
    lib = _lib.load()
    assert lib.geot_abi_version() == _lib.ABI_VERSION
    want = {"geot_mesh_angle_defects": "iiqqpppppppqqpppqp", "geot_scan_ball_sum": "ifpppppqp", "geot_curvature_sample": "iiiqppppppp p".replace(" ", "")}
    kinds = {"i": ctypes.c_int, "q": ctypes.c_longlong, "p": ctypes.c_void_p, "f": ctypes.c_float}
    for name, sig in want.items():
        assert names[name].streamed and names[name].ret == "int"
        assert _lib.PROTOTYPES[name] == [kinds[k] for k in sig], name
        assert getattr(lib, name).restype is ctypes.c_int
    assert _lib.PLAIN["geot_mesh_angle_defects_ws_bytes"] == ([ctypes.c_longlong], ctypes.c_longlong)
    assert _lib.PLAIN["geot_scan_ball_sum_ws_bytes"] == ([ctypes.c_int], ctypes.c_longlong)
    assert dataset.mesh_curvature is scan_set.mesh_curvature and callable(dataset.DeviceScanSet.compute_curvature)
    text = open(os.path.join(ROOT, "geot_amd", "openpoints", "dataset", "scan_set.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(trimesh|open3d)", text, flags=re.M)


def test_workspace_sizes_and_entry_point_refusals_need_no_device():
    from geot_amd import _lib
    lib = _lib.load()
    dws, bws = lib.geot_mesh_angle_defects_ws_bytes, lib.geot_scan_ball_sum_ws_bytes
    assert [dws(t) for t in (0, 1, 4, 5, 4225)] == [16, 32, 32, 48, 16912 + 16] and dws(-1) == -1 and dws((1 << 30) + 1) == -1
    assert dws(1 << 30) > 0
    assert all(bws(m) == lib.geot_knn_grid_ws_bytes(1, m) and bws(m) % 16 == 0 for m in (1, 63, 65, 4225, 1 << 24))
    assert bws(0) == -1 and bws(-5) == -1 and bws((1 << 24) + 1) == -1
    fake = 1 << 20
    # geot_mesh_angle_defects: hipErrorInvalidValue (1) before any launch: the pointers are never followed
    good = dict(b=2, n_scans=3, total=100, total_faces=50, points=fake, faces=fake, offsets=fake, face_offsets=fake, scan_ids=fake,
                out_offsets=fake, face_out_offsets=fake, batch_faces=50, total_out=100, defect_q=fake, stats=None, ws=fake,
                ws_bytes=dws(100))
    for change in (dict(b=-1), dict(b=65536), dict(n_scans=0), dict(total=0), dict(total_faces=-1), dict(batch_faces=-1),
                   dict(batch_faces=(2 ** 31 - 1) // 6 + 1), dict(total_out=-1), dict(total_out=(1 << 30) + 1, ws_bytes=1 << 40),
                   dict(points=None), dict(faces=None), dict(offsets=None), dict(face_offsets=None), dict(scan_ids=None),
                   dict(out_offsets=None), dict(face_out_offsets=None), dict(defect_q=None), dict(ws=None), dict(ws=fake + 4),
                   dict(ws=fake + 8), dict(ws_bytes=dws(100) - 16), dict(ws_bytes=0), dict(ws_bytes=-1)):
        assert lib.geot_mesh_angle_defects(*dict(good, **change).values(), None) == 1, change
    assert lib.geot_mesh_angle_defects(*dict(good, b=0).values(), None) == 0
    assert lib.geot_mesh_angle_defects(*dict(good, b=0, faces=None, total_faces=0, batch_faces=0).values(), None) == 0
    # geot_scan_ball_sum
    good = dict(m=100, radius=0.1, points=fake, value=fake, out=fake, absminmax=fake, ws=fake, ws_bytes=bws(100))
    for change in (dict(m=0), dict(m=-1), dict(m=(1 << 24) + 1, ws_bytes=1 << 40), dict(radius=0.0), dict(radius=-0.1),
                   dict(radius=float("inf")), dict(radius=float("nan")), dict(points=None), dict(value=None), dict(out=None),
                   dict(absminmax=None), dict(ws=None), dict(ws=fake + 4), dict(ws=fake + 8), dict(ws_bytes=bws(100) - 16),
                   dict(ws_bytes=0), dict(ws_bytes=-1)):
        assert lib.geot_scan_ball_sum(*dict(good, **change).values(), None) == 1, change
    # geot_curvature_sample
    good = dict(s=2, m=8, n_scans=3, total=100, curvature=fake, absminmax=fake, offsets=fake, scan_ids=fake, sel=fake, out=fake, bad=fake)
    for change in (dict(s=-1), dict(s=65536), dict(m=0), dict(m=-3), dict(n_scans=0), dict(total=0), dict(curvature=None),
                   dict(absminmax=None), dict(offsets=None), dict(scan_ids=None), dict(sel=None), dict(out=None), dict(bad=None)):
        assert lib.geot_curvature_sample(*dict(good, **change).values(), None) == 1, change
    assert lib.geot_curvature_sample(*dict(good, s=0).values(), None) == 0


def test_python_refusals_come_before_any_device_call():
    import torch
    from geot_amd.openpoints.dataset import DeviceScanSet, mesh_curvature
    from geot_amd.openpoints.dataset.scan_set import check_curvature, check_radius
    for bad in (0, 0.0, -0.1, float("inf"), float("nan"), None, "0.1", True, [0.1], 1e-60, 1e60, np.float32("nan")):
        with pytest.raises(ValueError, match="radius must be a finite positive number"):
            check_radius(bad, "t")
    assert check_radius(0.1, "t") == 0.1 and check_radius(np.float32(2), "t") == 2.0 and check_radius(3, "t") == 3.0
    bare = DeviceScanSet.__new__(DeviceScanSet)          # no device here: the checks below come before one is needed
    bare.faces = bare.has_mesh = bare.curvature = bare.curvature_radius = None
    bare.sizes = [4, 5]
    with pytest.raises(ValueError, match="the scan set holds no faces"):
        bare.compute_curvature()
    with pytest.raises(ValueError, match="the scan set holds no faces"):
        mesh_curvature(bare, 0.2)
    for call in (lambda: bare.compute_curvature(radius=-1), lambda: mesh_curvature(bare, radius=0), lambda: mesh_curvature(bare, None)):
        with pytest.raises(ValueError, match="radius must be a finite positive number"):
            call()
    with pytest.raises(ValueError, match="must be a DeviceScanSet"):
        mesh_curvature([np.zeros((3, 3))])
    with pytest.raises(ValueError, match=r"call scans.compute_curvature\(\) first"):
        check_curvature(bare, [0], "ValBatcher")
    bare.curvature, bare.has_mesh = torch.zeros(9), [True, False]
    check_curvature(bare, [0, 0], "ValBatcher")
    with pytest.raises(ValueError, match=r"batch slot 1 \(scan 1\) has no mesh"):
        check_curvature(bare, [0, 1], "ValBatcher")
    # the constructors take the switch and it is off by default
    import inspect
    from geot_amd.openpoints.dataset import FixMatchBatcher, SupervisedBatcher, ValBatcher, VoteBatcher
    for cls in (SupervisedBatcher, FixMatchBatcher, ValBatcher, VoteBatcher):
        assert inspect.signature(cls.__init__).parameters["curvatures"].default is False and cls.curvatures is False
