"""Scan files on the host.  The reference loads a Teeth3DS scan with trimesh.load(path, process=False) and keeps mesh.vertices
alone (openpoints/dataset/io.py); read_obj returns the same vertices in the same order -- nothing merged, nothing dropped -- and
the triangles beside them, which is what DeviceScanSet(faces=) and validation.mesh_neighbours start from.  Written from the
Wavefront OBJ format; numpy only (neither trimesh nor open3d is needed, and neither is imported)."""
import numpy as np


def _corner(token, n_vertices, path, number):
    """One corner of an `f` line -- `a`, `a/b`, `a//c` or `a/b/c` -> the 0-based vertex index: 1-based, or negative and
    relative to the vertices read so far."""
    try:
        i = int(token.split("/")[0])
    except ValueError:
        i = 0
    if i > 0:
        return i - 1
    if i < 0 and n_vertices + i >= 0:
        return n_vertices + i
    raise ValueError("read_obj: %s, line %d: %r is no vertex index" % (path, number, token))


def read_obj(path):
    """The `v` and `f` lines of a Wavefront OBJ file, in file order -> (vertices (N, 3) float32, faces (F, 3) int32, 0-based).
    A `v` line gives its first three numbers (a colour or w behind them is ignored).  An `f` corner is `a`, `a/b`, `a//c` or
    `a/b/c`; a is 1-based, or negative: relative to the vertices read so far.  A polygon of more than three corners becomes a
    fan from its first corner.  Every other line (comments, vn, vt, g, o, s, usemtl, ...) is ignored.  A malformed `v` or `f`
    line is a ValueError that names the line number.  A positive index beyond the file's vertices is kept as it is: index
    values are checked where they are used (geot_mesh_neighbours ignores such a face and counts it)."""
    vertices, faces = [], []
    with open(path, "r", errors="replace") as f:
        for number, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if parts[0] == "v":
                try:
                    x, y, z = (float(t) for t in parts[1:4])
                except ValueError:
                    raise ValueError("read_obj: %s, line %d: a vertex needs three numbers, got %r" % (path, number, line.strip())) from None
                vertices.append((x, y, z))
            elif parts[0] == "f":
                if len(parts) < 4:
                    raise ValueError("read_obj: %s, line %d: a face needs three corners, got %r" % (path, number, line.strip()))
                corners = [_corner(t, len(vertices), path, number) for t in parts[1:]]
                faces.extend((corners[0], corners[j], corners[j + 1]) for j in range(1, len(corners) - 1))
    return (np.asarray(vertices, dtype=np.float32).reshape(-1, 3), np.asarray(faces, dtype=np.int64).clip(-1, 2 ** 31 - 1)
            .astype(np.int32).reshape(-1, 3))
