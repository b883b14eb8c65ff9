"""Scan meshes, the part that needs no GPU: the ABI and the binding of geot_mesh_neighbours, its workspace sizes, the refusals that
come before any device call (C and Python), read_obj on files written here, DeviceScanSet's checks of faces=, and the numpy
restatement the GPU tests compare against (tests/_mesh_ref.py) on meshes checked by hand -- with the two-sheets property the GPU
test relies on, shown on the restatements alone."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_ref as mref  # noqa: E402
import _scan_islands_ref as iref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_version_signatures_and_exports():
    import geot_amd
    from geot_amd import _lib, build, validation
    from geot_amd.openpoints import dataset
    build.build()
    hdr = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    assert int(re.search(r"GEOT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 36
    lib = _lib.load()
    assert lib.geot_abi_version() == _lib.ABI_VERSION
    decl = re.search(r"int geot_mesh_neighbours\(([^;]*)\);", hdr).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["int b", "int k", "int n_scans", "long long total", "long long total_faces", "const int *faces",
                    "const long long *offsets", "const long long *face_offsets", "const long long *scan_ids",
                    "const long long *out_offsets", "const long long *face_out_offsets", "long long batch_faces", "int *nbr",
                    "int *stats", "void *ws", "long long ws_bytes", "void *stream"]
    proto = _lib.PROTOTYPES["geot_mesh_neighbours"]
    assert len(proto) == len(args)
    for a, t in zip(args, proto):
        want = ctypes.c_void_p if "*" in a else ctypes.c_longlong if a.startswith("long long") else ctypes.c_int
        assert t is want, (a, t)
    assert lib.geot_mesh_neighbours.argtypes == proto and lib.geot_mesh_neighbours.restype is ctypes.c_int
    assert re.search(r"long long geot_mesh_neighbours_ws_bytes\(int b, long long total_out, long long batch_faces\);", hdr)
    assert _lib.PLAIN["geot_mesh_neighbours_ws_bytes"] == ([ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong], ctypes.c_longlong)
    assert _lib.CONSTANTS["GEOT_MESH_NEIGHBOURS_LANE_ROW"] == 64        # the lane / wave threshold the GPU test stands on
    assert callable(validation.mesh_neighbours) and geot_amd.mesh_neighbours is validation.mesh_neighbours
    assert validation.MESH_K == 16 and "mesh" in validation._CLEAN_KEYS
    assert callable(dataset.read_obj) and dataset.read_obj.__module__ == "geot_amd.openpoints.dataset.io"


def test_workspace_sizes_and_entry_point_refusals_need_no_device():
    from geot_amd import _lib
    lib = _lib.load()
    ws = lib.geot_mesh_neighbours_ws_bytes
    # the 6 raw entries of every face (24 bytes, rounded up to 16) ...
    assert ws(2, 0, 0) == 32 and ws(0, 0, 0) == 32
    assert [ws(2, 0, f) - ws(2, 0, 0) for f in (1, 2, 3, 1000)] == [32, 48, 80, 24000]
    assert ws(2, 5000, 2000) - ws(2, 5000, 0) == 48000 and ws(2, 5000, 4000) - ws(2, 5000, 2000) == 48000        # linear
    # ... and a unit of 16 bytes per vertex row, per started 4096 rows, and two: exact in total_out
    assert [ws(2, t, 0) for t in (1, 2, 4095, 4096, 4097, 8192)] == [16 * (t + t // 4096 + 2) for t in (1, 2, 4095, 4096, 4097, 8192)]
    assert ws(1, 8450, 16384) == 24 * 16384 + 16 * (8450 + 2 + 2)
    assert len({ws(3, t, 7) for t in range(4090, 4110)}) == 20                                                  # no two sizes alike
    assert all(ws(b, t, f) % 16 == 0 for b in (0, 1, 65535) for t in (0, 1, 7, 4097) for f in (0, 1, 2, 3, 4, 5))
    assert ws(65535, 1 << 30, (2 ** 31 - 1) // 6) > 0
    for b, total, f in ((-1, 10, 10), (65536, 10, 10), (2, -1, 10), (2, (1 << 30) + 1, 10), (2, 10, -1), (2, 10, (2 ** 31 - 1) // 6 + 1),
                        (2, 10, 1 << 40)):
        assert ws(b, total, f) == -1, (b, total, f)
    # hipErrorInvalidValue (1) before any launch: the pointers are never followed
    fake = 1 << 20
    size = ws(2, 100, 50)
    good = dict(b=2, k=16, n_scans=3, total=100, total_faces=50, faces=fake, offsets=fake, face_offsets=fake, scan_ids=fake,
                out_offsets=fake, face_out_offsets=fake, batch_faces=50, nbr=fake, stats=None, ws=fake, ws_bytes=size)
    for change in (dict(b=-1), dict(b=65536), dict(k=0), dict(k=33), dict(n_scans=0), dict(total=0), dict(total_faces=-1),
                   dict(batch_faces=-1), dict(batch_faces=(2 ** 31 - 1) // 6 + 1, ws_bytes=1 << 40), dict(faces=None),
                   dict(offsets=None), dict(face_offsets=None), dict(scan_ids=None), dict(out_offsets=None),
                   dict(face_out_offsets=None), dict(nbr=None), dict(ws=None), dict(ws=fake + 4), dict(ws=fake + 8),
                   dict(ws_bytes=ws(2, 0, 50) - 16), dict(ws_bytes=0), dict(ws_bytes=-1)):
        a = dict(good, **change)
        assert lib.geot_mesh_neighbours(*a.values(), None) == 1, change
    # nothing to do: b = 0 (and faces may be NULL when the set has none)
    assert lib.geot_mesh_neighbours(*dict(good, b=0).values(), None) == 0
    assert lib.geot_mesh_neighbours(*dict(good, b=0, faces=None, total_faces=0, batch_faces=0, ws_bytes=32).values(), None) == 0


# ---- read_obj ---------------------------------------------------------------------------------------------------------------------------
def test_read_obj_reads_vertices_and_faces_in_file_order(tmp_path):
    from geot_amd.openpoints.dataset import read_obj
    path = tmp_path / "scan.obj"
    path.write_text("# a comment\n"
                    "mtllib nothing.mtl\no tooth\n"
                    "v 0 0 0\nv 1 0 0.5\nvn 0 0 1\nv 1 1 0 0.2 0.3 0.4\nvt 0.5 0.5\nv 0 1 0\n\n"
                    "f 1 2 3\n"                     # a
                    "f 1/1 3/2 4/3\n"               # a/b
                    "f 2//1 3//1 4//1\n"            # a//c
                    "f 1/1/1 2/2/1 4/3/1\n"         # a/b/c
                    "v 2 2 2\nv -1.5e0 +2 3\n"
                    "f -1 -2 -6\n"                  # relative to the six vertices read so far: 5, 4, 0
                    "s off\nusemtl white\n"
                    "f 1 2 3 4\n"                   # a quad: a fan from its first corner
                    "f 1 2 3 4 5\n"                 # a pentagon
                    "g end\n")
    v, f = read_obj(str(path))
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.shape == (6, 3)
    assert v.tolist() == [[0, 0, 0], [1, 0, 0.5], [1, 1, 0], [0, 1, 0], [2, 2, 2], [-1.5, 2, 3]]
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [1, 2, 3], [0, 1, 3], [5, 4, 0], [0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [0, 3, 4]]
    # no faces, no vertices: empty arrays of the right shape; a positive index beyond the file's vertices is kept
    (tmp_path / "points.obj").write_text("v 1 2 3\nv 4 5 6\n")
    v, f = read_obj(tmp_path / "points.obj")
    assert v.shape == (2, 3) and f.shape == (0, 3) and f.dtype == np.int32
    (tmp_path / "empty.obj").write_text("# nothing\n")
    v, f = read_obj(tmp_path / "empty.obj")
    assert v.shape == (0, 3) and f.shape == (0, 3)
    (tmp_path / "beyond.obj").write_text("v 0 0 0\nf 1 2 9\n")
    assert read_obj(tmp_path / "beyond.obj")[1].tolist() == [[0, 1, 8]]


@pytest.mark.parametrize("text, line", [("v 0 0 0\nv 1 x 0\n", 2), ("v 0 0\n", 1), ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2\n", 4),
                                         ("v 0 0 0\nv 1 0 0\nv 0 1 0\n# c\nf 1 2 0\n", 5), ("v 0 0 0\nf 1 a/1 1\n", 2),
                                         ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf -1 -2 -4\n", 4), ("v 0 0 0\nf 1 //2 1\n", 2)])
def test_read_obj_names_the_line_of_a_malformed_entry(tmp_path, text, line):
    from geot_amd.openpoints.dataset import read_obj
    path = tmp_path / "bad.obj"
    path.write_text(text)
    with pytest.raises(ValueError, match=r"line %d\b" % line):
        read_obj(path)


def test_read_obj_needs_neither_trimesh_nor_open3d():
    import geot_amd.openpoints.dataset.io as io
    text = open(io.__file__).read()
    assert not re.search(r"^\s*(import|from)\s+(trimesh|open3d)", text, flags=re.M)


# ---- DeviceScanSet(faces=) -----------------------------------------------------------------------------------------------------------------
def test_scan_set_checks_faces_before_the_device_is_needed():
    import torch
    from geot_amd.openpoints.dataset import DeviceScanSet
    from geot_amd.openpoints.dataset.scan_set import check_faces
    tri = np.array([[0, 1, 2]], dtype=np.int32)
    got = check_faces([tri, None, np.zeros((0, 3), dtype=np.int64), torch.tensor([[2, 1, 0], [0, 2, 1]], dtype=torch.uint8)], 4)
    assert got[1] is None and [None if g is None else tuple(g.shape) for g in got] == [(1, 3), None, (0, 3), (2, 3)]
    for bad, n, msg in (([tri], 2, "one entry per scan"), ([tri, tri, tri], 2, "one entry per scan"), (tri, 1, "one entry per scan"),
                        ([tri.reshape(3)], 1, r"faces\[0\] must be \(F, 3\)"), ([tri, np.zeros((2, 4), dtype=np.int32)], 2, r"faces\[1\] must be \(F, 3\)"),
                        ([tri.astype(np.float32)], 1, r"faces\[0\] must hold integer"), ([tri > 0], 1, r"faces\[0\] must hold integer")):
        with pytest.raises(RuntimeError, match=msg):
            check_faces(bad, n)
    # through the constructor: the faces are refused before the device is looked at (this machine may have none)
    pts, labels = [np.zeros((3, 3), dtype=np.float32)], [np.zeros(3, dtype=np.int32)]
    with pytest.raises(RuntimeError, match=r"faces\[0\] must be \(F, 3\)"):
        DeviceScanSet(pts, labels, faces=[tri.reshape(3)], device="cpu")
    with pytest.raises(RuntimeError, match="one entry per scan"):
        DeviceScanSet(pts, labels, faces=[tri, tri], device="cpu")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        DeviceScanSet(pts, labels, faces=[tri], device="cpu")


# ---- the Python refusals ---------------------------------------------------------------------------------------------------------------------
def test_python_refusals_come_before_any_device_call():
    import torch
    from geot_amd import validation as V
    from geot_amd.fit import fit
    batch = {"scans": None, "sizes": [20, 30], "scan_ids": None, "mandible": [True, False], "ids": [0, 1]}
    preds = [torch.zeros(1, 20, dtype=torch.int64), torch.zeros(1, 30, dtype=torch.int64)]
    table = torch.zeros((50, 9), dtype=torch.int32)
    for call in (V.clean_scans, V.scan_components):
        for mesh in (True, 16):
            with pytest.raises(RuntimeError, match="mesh and nbr are two tables"):
                call(preds, batch, mesh=mesh, nbr=table)
        for bad in (0, 33, -1, 2.0, "yes", [16]):
            with pytest.raises(RuntimeError, match="mesh must be None, a bool or an int in 1..32"):
                call(preds, batch, mesh=bad)
    for bad in (0, 33, -1, 2.0, True, "16", None):
        with pytest.raises(ValueError, match="k must be an int in 1..32"):
            V.mesh_neighbours(batch, k=bad)
    assert [V._mesh_width(m, "t") for m in (None, False, True, 1, 32, np.int64(7))] == [None, None, 16, 1, 32, 7]

    class Never:
        def eval(self):
            raise AssertionError("called")
    for bad in ({"mesh": 0}, {"mesh": 33}, {"mesh": 2.5}, {"mesh": "yes"}, {"mesh": [8]}, {"mesh": True, "nbr": table},
                {"mesh": 8, "nbr": table}):
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
    for good in ({"mesh": True}, {"mesh": False, "nbr": table}, {"mesh": None}, {"mesh": 12, "min_size": 4}):
        assert V._islands_kw(good, "t") == good

    # a set without faces: fit() refuses before the first epoch (val or test, a set or a batcher on one); the label calls
    # before their forward pass
    class Faceless:
        faces = None

    class OnFaceless:
        scans = Faceless()
    for kw in (dict(val=Faceless()), dict(test=Faceless()), dict(val=OnFaceless())):
        with pytest.raises(ValueError, match="the scan set holds no faces"):
            fit(None, None, {"epochs": 1}, islands={"mesh": True}, **kw)
    with pytest.raises(ValueError, match="the scan set holds no faces"):
        V.predict_scans(None, {"scans": Faceless()}, islands={"mesh": 16})
    with pytest.raises(ValueError, match="the scan set holds no faces"):
        V.vote_scans(Never(), OnFaceless(), [0], 2, islands={"mesh": True})
    with pytest.raises(ValueError, match="the scan set holds no faces"):
        V.cover_scans(Never(), OnFaceless(), [0], islands={"mesh": True})
    with pytest.raises(ValueError, match="the scan set holds no faces"):
        V.decode_scans(Never(), OnFaceless(), [0], islands={"mesh": True})


def test_mesh_neighbours_names_the_slot_and_the_scan_without_a_mesh():
    import torch
    from geot_amd.validation import mesh_neighbours

    class Scans:
        device = torch.device("cpu")
        faces = None
        has_mesh = None

        def __len__(self):
            return 3
    batch = {"scans": Scans(), "sizes": [8, 30], "scan_ids": torch.zeros(2, dtype=torch.int64), "ids": [2, 1]}
    with pytest.raises(ValueError, match="the scan set holds no faces"):
        mesh_neighbours(batch)
    Scans.faces, Scans.has_mesh = torch.zeros((0, 3), dtype=torch.int32), [True, False, True]
    with pytest.raises(ValueError, match=r"batch slot 1 \(scan 1\) has no mesh"):
        mesh_neighbours(batch)
    with pytest.raises(ValueError, match=r'must carry its 2 scan numbers as host values \("ids"'):
        mesh_neighbours({key: value for key, value in batch.items() if key != "ids"})


# ---- the restatement on meshes small enough to check by hand ----------------------------------------------------------------------------
def test_restatement_by_hand():
    # a single triangle, either winding; an isolated vertex (3) has a row of -1
    for tri in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        table, st = mref.mesh_table([tri], 4, 3)
        assert table.tolist() == [[1, 2, -1], [0, 2, -1], [0, 1, -1], [-1, -1, -1]] and st == [1, 0, 0, 2]
    # two triangles sharing the edge 1-2; said twice and in another order: nothing changes
    two = [[0, 1, 2], [2, 1, 3]]
    table, st = mref.mesh_table(two, 4, 4)
    assert table.tolist() == [[1, 2, -1, -1], [0, 2, 3, -1], [0, 1, 3, -1], [1, 2, -1, -1]] and st == [2, 0, 0, 3]
    again, st2 = mref.mesh_table([[3, 2, 1], [0, 1, 2], [1, 2, 0], [2, 1, 3]], 4, 4)
    assert np.array_equal(again, table) and st2 == [4, 0, 0, 3]
    # a repeated index: the remaining distinct pair; all three equal: nothing, and the face still counts as usable
    table, st = mref.mesh_table([[0, 0, 1], [2, 2, 2]], 3, 2)
    assert table.tolist() == [[1, -1], [0, -1], [-1, -1]] and st == [2, 0, 0, 1]
    # a face with an index outside [0, m) is ignored as a whole and counted
    table, st = mref.mesh_table([[0, 1, 2], [0, 1, 3], [0, -1, 1], [2 ** 31 - 1, 0, 1]], 3, 2)
    assert table.tolist() == [[1, 2], [0, 2], [0, 1]] and st == [1, 3, 0, 2]
    # truncation at k and k + 1 neighbours: the centre of a fan of k / k + 1 rim vertices
    k = 5
    table, st = mref.mesh_table(mref.fan(k), k + 1, k)
    assert table[0].tolist() == [1, 2, 3, 4, 5] and st == [k, 0, 0, 5] and table[1].tolist() == [0, 2, 5, -1, -1]
    table, st = mref.mesh_table(mref.fan(k + 1), k + 2, k)
    assert table[0].tolist() == [1, 2, 3, 4, 5] and st == [k + 1, 0, 1, 5] and table[6].tolist() == [0, 1, 5, -1, -1]
    # no faces at all
    table, st = mref.mesh_table(np.zeros((0, 3)), 2, 3)
    assert table.tolist() == [[-1] * 3] * 2 and st == [0, 0, 0, 0]


def test_generators():
    f = mref.grid(65, 65)
    assert f.shape == (8192, 3) and f.min() == 0 and f.max() == 4224
    table, st = mref.mesh_table(f, 4225, 8)
    assert st == [8192, 0, 0, 6] and (table[66] == [1, 2, 65, 67, 130, 131, -1, -1]).all()        # an interior vertex: valence 6
    for kw in (dict(order=True), dict(corners=True), dict(corners=True, duplicate=0.1)):
        g = mref.shuffled(f, 3, **kw)
        assert not np.array_equal(g[:len(f)], f) and len(g) == len(f) + (819 if kw.get("duplicate") else 0)
        other, st2 = mref.mesh_table(g, 4225, 8)
        assert np.array_equal(other, table) and st2[1:] == st[1:]
    assert mref.fan(40).shape == (40, 3) and mref.mesh_table(mref.fan(40), 41, 32)[1] == [40, 0, 1, 32]


def test_two_sheets_are_one_piece_by_distance_and_two_over_the_mesh():
    """The property tests/test_mesh_islands_gpu.py shows on the GPU, on the two restatements alone: two sheets closer to each
    other than a mesh edge is long, all of one label -- the kNN table joins them, the mesh's one-ring does not."""
    g = 12
    pts, faces = mref.two_sheets(g, 0.25)
    labels = np.ones(2 * g * g, dtype=np.int64)
    knn = iref.knn_table(pts, 9)                                       # k = 8 and the vertex itself
    assert (iref.components(labels, knn, 17) == 0).all()                # ONE component
    mesh, st = mref.mesh_table(faces, 2 * g * g, 16)
    comp = iref.components(labels, mesh, 17)
    assert st == [4 * (g - 1) ** 2, 0, 0, 6]
    assert sorted(set(comp.tolist())) == [0, g * g] and (comp[:g * g] == 0).all() and (comp[g * g:] == g * g).all()      # TWO
