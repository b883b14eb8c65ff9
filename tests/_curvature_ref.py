"""The mesh-curvature entry points (include/geot_hip.h, ABI 37) restated in numpy from the header's text: the corner angle in
float32 with the library's own atan2 (every operation a separately rounded float32 +, -, *, / or sqrt: the kernel's bits), the
quantisation and the integer sums of geot_mesh_angle_defects; the brute-force float32 ball membership and the integer sum of
geot_scan_ball_sum; the normalisation of geot_curvature_sample.  Beside it an INDEPENDENT float64 computation (np.arctan2,
float64 distances) and the small closed meshes whose total defect is known.  trimesh is not involved anywhere."""
import numpy as np

F = np.float32
Q = 4294967296.0                                          # 2^32
Q2PI = int(np.rint(2.0 * np.pi * Q))                      # llrint(2 pi 2^32) from the double constant
PI_HI = F(np.pi)
PI_LO = F(np.pi - np.float64(PI_HI))
TAN_PIO8 = F(0.41421357)
U = 2.0 ** -24                                            # float32's unit roundoff

# The per-angle bound of the float32 restatement against float64, ABSOLUTE in radians and independent of the triangle's
# conditioning, by operation count (u = 2^-24; every rounded operation errs by at most u times its result).  Written down
# before any difference was looked at.
#   edges      each component of e1, e2 is one rounded subtraction: a relative u per component moves a vector's direction by
#              at most u: 2 u for the two edges
#   cross      a component is two rounded products and a rounded difference: at most u (|p1| + |p2|) + u |c| <= 2 u L,
#              L = |e1| |e2| (Cauchy-Schwarz on the component's two axes): the vector errs by at most 2 sqrt(3) u L < 3.5 u L
#   norm       three rounded squares and two rounded sums under a correctly rounded sqrtf: (3 / 2 + 1) u n = 2.5 u n <= 2.5 u L
#   dot        three rounded products and two rounded sums: at most u (|p1| + |p2| + |p3|) + u |s1| + u |d| <= 3 u L
#   atan2      n^2 + d^2 = L^2, so the angle moves by at most sqrt(dn^2 + dd^2) / L <= sqrt(6^2 + 3^2) u < 6.8 u
#   reduction  t = min / max: u t <= u; past tan(pi / 8) t' = (t - 1) / (t + 1), three more rounded operations on |t'| <= 0.4143
#              and dt' / dt = 2 / (t + 1)^2 <= 1: at most u + 3 * 0.4143 u < 2.3 u on the argument, and |atan'| <= 1
#   polynomial Horner on w <= 0.1716 and the final t + t w p, all values below 0.4143: at most 1 u; truncation (the Taylor
#              series cut before t^21 / 21) < 4.5e-10 < 0.01 u
#   constants  pi / 4 + r: the small part first (0.42 u), then a result below 0.79 (0.79 u); pi / 2 - r: 0.79 u and 1.58 u;
#              pi - r: 1.58 u and 3.15 u: 8.3 u in all when every step is taken; each constant is hi + lo with an error below u^2
# In all 2 + 6.8 + 2.3 + 1.01 + 8.3 = 20.41 u; second-order terms are below u^2 * 100.  ANGLE_BOUND rounds that up to 24 u.
ANGLE_BOUND = 24 * U                                      # 1.43e-6 rad


def atan2_f32(y, x):
    """The library's atan2 for y >= 0, on float32 arrays, operation for operation (csrc/mesh_curvature.hip mc_atan2)."""
    y, x = np.asarray(y, dtype=F), np.asarray(x, dtype=F)
    with np.errstate(all="ignore"):
        ax = np.where(x < 0, -x, x).astype(F)
        dead = ~(y < np.inf) | ~(ax < np.inf)
        steep = y > ax
        lo, hi = np.where(steep, ax, y).astype(F), np.where(steep, y, ax).astype(F)
        dead |= hi == 0
        t = (lo / np.where(dead, F(1), hi)).astype(F)
        upper = t > TAN_PIO8
        t = np.where(upper, ((t - F(1)) / (t + F(1))).astype(F), t).astype(F)
        w = (t * t).astype(F)
        p = np.full(t.shape, -F(1.0 / 19.0), dtype=F)
        for k, sign in ((17, 1), (15, -1), (13, 1), (11, -1), (9, 1), (7, -1), (5, 1), (3, -1)):
            c = F(1.0 / k)
            p = (p * w).astype(F)
            p = (p + c if sign > 0 else p - c).astype(F)
        r = (t + ((t * w).astype(F) * p).astype(F)).astype(F)
        r = np.where(upper, (F(0.25) * PI_HI + (F(0.25) * PI_LO + r).astype(F)).astype(F), r)
        r = np.where(steep, (F(0.5) * PI_HI - (r - F(0.5) * PI_LO).astype(F)).astype(F), r)
        r = np.where(x < 0, (PI_HI - (r - PI_LO).astype(F)).astype(F), r)
    return np.where(dead, F(0), r).astype(F)


def corner_angles_f32(a, b, c):
    """The angle at corner a of the faces (a, b, c): (F, 3) float32 coordinates each -> (F,) float32, the kernel's bits."""
    a, b, c = (np.asarray(v, dtype=F) for v in (a, b, c))
    with np.errstate(all="ignore"):
        u, v = (b - a).astype(F), (c - a).astype(F)
        cx = ((u[:, 1] * v[:, 2]).astype(F) - (u[:, 2] * v[:, 1]).astype(F)).astype(F)
        cy = ((u[:, 2] * v[:, 0]).astype(F) - (u[:, 0] * v[:, 2]).astype(F)).astype(F)
        cz = ((u[:, 0] * v[:, 1]).astype(F) - (u[:, 1] * v[:, 0]).astype(F)).astype(F)
        n = np.sqrt((((cx * cx).astype(F) + (cy * cy).astype(F)).astype(F) + (cz * cz).astype(F)).astype(F)).astype(F)
        d = (((u[:, 0] * v[:, 0]).astype(F) + (u[:, 1] * v[:, 1]).astype(F)).astype(F) + (u[:, 2] * v[:, 2]).astype(F)).astype(F)
    return atan2_f32(n, d)


def corner_angles_f64(a, b, c):
    """The same angle in float64 with np.arctan2: the independent computation."""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in (a, b, c))
    u, v = b - a, c - a
    return np.arctan2(np.linalg.norm(np.cross(u, v), axis=1), (u * v).sum(axis=1))


def _classes(points, faces):
    m = len(points)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < m)).all(axis=1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    g = f[ok]
    p = np.asarray(points)[g]                               # (G, 3 corners, 3)
    finite = np.isfinite(p).all(axis=(1, 2))
    with np.errstate(invalid="ignore"):
        same = (p[:, 0] == p[:, 1]).all(1) | (p[:, 1] == p[:, 2]).all(1) | (p[:, 0] == p[:, 2]).all(1)
    return f, ok, g, p, ~finite | same


def defects_q(points, faces):
    """geot_mesh_angle_defects on one usable slot: points (M, 3) float32, faces (F, 3) -> (defect_q (M,) int64, [usable,
    ignored, degenerate faces, vertices in no usable face])."""
    points = np.asarray(points, dtype=F)
    m = len(points)
    f, ok, g, p, degenerate = _classes(points, faces)
    total = np.zeros(m, dtype=np.int64)
    live = ~degenerate
    for e in range(3):
        ang = corner_angles_f32(p[live, e], p[live, (e + 1) % 3], p[live, (e + 2) % 3])
        np.add.at(total, g[live, e], np.rint(ang.astype(np.float64) * Q).astype(np.int64))
    valence = np.bincount(g.reshape(-1), minlength=m)
    return Q2PI - total, [int(ok.sum()), int((~ok).sum()), int(degenerate.sum()), int((valence == 0).sum())]


def defects_f64(points, faces):
    """The defects in float64 radians under the same face rules -> (M,) float64."""
    points = np.asarray(points, dtype=F)
    f, ok, g, p, degenerate = _classes(points, faces)
    total = np.zeros(len(points), dtype=np.float64)
    live = ~degenerate
    for e in range(3):
        np.add.at(total, g[live, e], corner_angles_f64(p[live, e], p[live, (e + 1) % 3], p[live, (e + 2) % 3]))
    return 2.0 * np.pi - total


def sqdist_f32(points, v):
    """sqdist3 of every point to vertex v, ((dx dx) + (dy dy)) + (dz dz) with every operation rounded to float32."""
    with np.errstate(all="ignore"):
        d = (points - points[v]).astype(F)
        return (((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F) + (d[:, 2] * d[:, 2]).astype(F)).astype(F)


def members(points, radius):
    """The closed balls by brute force in float32 -> (M, M) bool, row v: the u with sqdist3(u, v) <= radius * radius."""
    points = np.asarray(points, dtype=F)
    r2 = F(F(radius) * F(radius))
    with np.errstate(invalid="ignore"):
        return np.stack([sqdist_f32(points, v) <= r2 for v in range(len(points))])


def ball_sum(points, value, radius, inside=None):
    """geot_scan_ball_sum: -> (out (M,) float32, the integer sums (M,) int64, [min |out|, max |out|] float32)."""
    inside = members(points, radius) if inside is None else inside
    value = np.asarray(value, dtype=np.int64)
    sums = np.array([value[row].sum(dtype=np.int64) for row in inside], dtype=np.int64)
    out = (sums.astype(np.float64) * (1.0 / Q)).astype(F)
    return out, sums, np.array([np.abs(out).min(), np.abs(out).max()], dtype=F)


def ord_keys(lo_hi):
    """Two non-negative float32 -> the order-preserving unsigned keys geot_scan_ball_sum writes."""
    return np.asarray(lo_hi, dtype=F).view(np.uint32) | np.uint32(0x80000000)


def curvature(points, faces, radius, inside=None):
    """The whole definition on one scan -> (curvature (M,) float32, range (2,) float32, defect_q, stats)."""
    dq, stats = defects_q(points, faces)
    out, _, rng = ball_sum(points, dq, radius, inside)
    return out, rng, dq, stats


def _rows_f64(points, chunk=256):
    """(first row, float64 squared distances of rows first .. first + chunk to every vertex), chunk by chunk."""
    p = np.asarray(points, dtype=np.float64)
    for first in range(0, len(p), chunk):
        yield first, ((p[first:first + chunk, None, :] - p[None, :, :]) ** 2).sum(-1)


def curvature_f64(points, faces, radius):
    """Independent: float64 angles, float64 distances -> (curvature (M,) float64, ball members per vertex (M,) int, the sum of
    the members' valences per vertex (M,) int)."""
    d = defects_f64(points, faces)
    _, _, g, _, _ = _classes(np.asarray(points, dtype=F), faces)
    valence = np.bincount(g.reshape(-1), minlength=len(d))
    cur, count, load = np.zeros(len(d)), np.zeros(len(d), dtype=np.int64), np.zeros(len(d), dtype=np.int64)
    for first, d2 in _rows_f64(points):
        with np.errstate(invalid="ignore"):
            inside = d2 <= float(radius) ** 2
        rows = slice(first, first + len(d2))
        cur[rows], count[rows], load[rows] = np.where(inside, d[None, :], 0.0).sum(1), inside.sum(1), (inside * valence[None, :]).sum(1)
    return cur, count, load


def near_the_radius(points, radius, rel=2.0 ** -18):
    """How many ordered pairs of vertices lie within a relative `rel` of the radius (float64 distances): there float32 and
    float64 may disagree about membership."""
    return int(sum((np.abs(np.sqrt(d2) - float(radius)) <= rel * float(radius)).sum() for _, d2 in _rows_f64(points)))


def normalise(cur, rng, sel=None):
    """geot_curvature_sample for one scan in float32: (|cur[sel]| - min) / (max - min), 0 everywhere unless max > min."""
    cur, (lo, hi) = np.asarray(cur, dtype=F), np.asarray(rng, dtype=F)
    picked = np.abs(cur if sel is None else cur[np.asarray(sel)]).astype(F)
    if not hi > lo:
        return np.zeros(picked.shape, dtype=F)
    return ((picked - lo).astype(F) / F(hi - lo)).astype(F)


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=F)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int32)
    return v, f


def icosphere(levels=1):
    """An icosahedron subdivided `levels` times, its vertices on the unit sphere: closed, genus 0."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(levels):
        mid, out = {}, []

        def middle(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.asarray(v, dtype=F), np.asarray(f, dtype=np.int32)


def torus(n=16, big=2.0, small=0.75):
    """An n x n grid on a torus, every cell cut into two triangles: closed, genus 1 (total defect 0)."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a, b = 2 * np.pi * i / n, 2 * np.pi * j / n
    v = np.stack([(big + small * np.cos(b)) * np.cos(a), (big + small * np.cos(b)) * np.sin(a), small * np.sin(b)], -1).reshape(-1, 3)
    at = lambda y, x: ((y % n) * n + (x % n)).reshape(-1)            # noqa: E731
    f = np.concatenate([np.stack([at(i, j), at(i + 1, j), at(i, j + 1)], 1), np.stack([at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)], 1)])
    return v.astype(F), f.astype(np.int32)


def cube():
    """A cube of 8 vertices and 12 triangles: every vertex has defect pi / 2 however its faces are cut."""
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=F)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return v, np.asarray(f, dtype=np.int32)


def height_field(r, c, seed, pitch=1.0, height=0.3, jitter=0.2):
    """The vertices of _mesh_ref.grid(r, c) as a rough height field: a jittered lattice of `pitch`, z random in [0, height)."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(r), np.arange(c), indexing="ij")
    p = np.stack([x.reshape(-1) + jitter * (rng.random(r * c) - 0.5), y.reshape(-1) + jitter * (rng.random(r * c) - 0.5),
                  height * rng.random(r * c) / pitch], 1) * pitch
    return p.astype(F)
