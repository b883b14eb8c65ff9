"""geot_mesh_neighbours (include/geot_hip.h) restated in numpy from the header's text, and not by the kernel's algorithm: the
directed pairs of every usable face, self pairs dropped, made distinct and ordered by one np.unique, cut at k.  Integers only:
array_equal.  And the small meshes the tests are built from."""
import numpy as np


def mesh_table(faces, m, k):
    """One usable slot: faces (F, 3) of a scan of m vertices -> (table (m, k) int32, [usable faces, ignored faces, truncated
    vertices, the longest row written])."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < m)).all(axis=1)                     # usable: all three indices inside the scan
    g = f[ok]
    pairs = np.concatenate([g[:, [0, 1]], g[:, [1, 0]], g[:, [0, 2]], g[:, [2, 0]], g[:, [1, 2]], g[:, [2, 1]]])
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]                 # a vertex is never its own neighbour
    key = np.unique(pairs[:, 0] * m + pairs[:, 1])            # distinct, by vertex and then by ascending neighbour
    v, u = key // m, key % m
    valence = np.bincount(v, minlength=m)
    rank = np.arange(key.size) - (np.cumsum(valence) - valence)[v]
    table = np.full((m, k), -1, dtype=np.int32)
    table[v[rank < k], rank[rank < k]] = u[rank < k]
    return table, [int(ok.sum()), int((~ok).sum()), int((valence > k).sum()), int(min(k, valence.max())) if m else 0]


def grid(r, c):
    """An r x c grid of vertices (vertex y * c + x), every cell cut into two triangles: 2 (r - 1) (c - 1) faces, interior
    valence 6 -> faces (F, 3) int32."""
    y, x = np.meshgrid(np.arange(r - 1), np.arange(c - 1), indexing="ij")
    v = (y * c + x).reshape(-1)
    return np.stack([np.stack([v, v + 1, v + c], 1), np.stack([v + 1, v + c + 1, v + c], 1)], 1).reshape(-1, 3).astype(np.int32)


def grid_points(r, c, z=0.0):
    """The vertices of grid(r, c), unit-spaced in the plane at height z -> (r c, 3) float32."""
    y, x = np.meshgrid(np.arange(r), np.arange(c), indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), np.full(r * c, z)], 1).astype(np.float32)


def fan(rim):
    """A closed fan: vertex 0 in the middle of rim >= 3 vertices 1 .. rim, rim faces -- the centre has valence rim and a raw
    row of 2 rim entries, a rim vertex valence 3 -> faces (rim, 3) int32 of rim + 1 vertices."""
    i = np.arange(rim)
    return np.stack([np.zeros(rim, dtype=np.int64), 1 + i, 1 + (i + 1) % rim], 1).astype(np.int32)


def two_sheets(g, gap=0.25):
    """Two g x g unit-spaced sheets, `gap` apart, as ONE scan of 2 g g vertices: closer to each other in space than a mesh edge
    is long, and not connected by any face -> (points (2 g g, 3) float32, faces int32).  The second sheet starts at g * g."""
    pts = np.concatenate([grid_points(g, g, 0.0), grid_points(g, g, gap)])
    f = grid(g, g)
    return pts, np.concatenate([f, f + g * g]).astype(np.int32)


def shuffled(faces, seed, order=True, corners=False, duplicate=0.0):
    """The same SET of faces, said differently: face order permuted, every face's corners rotated and every other one's
    winding flipped, and a fraction `duplicate` of the faces said twice."""
    rng = np.random.default_rng(seed)
    f = np.asarray(faces).copy()
    if duplicate:
        f = np.concatenate([f, f[rng.choice(len(f), int(len(f) * duplicate), replace=False)]])
    if corners:
        turn = rng.integers(0, 3, size=len(f))
        f = np.stack([np.take_along_axis(f, ((turn + j) % 3)[:, None], 1)[:, 0] for j in range(3)], 1)
        flip = rng.random(len(f)) < 0.5
        f[flip] = f[flip][:, ::-1]
    if order:
        f = f[rng.permutation(len(f))]
    return np.ascontiguousarray(f.astype(np.int32))
