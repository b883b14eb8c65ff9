"""Case tables and referees of the data-preparation kernels (geot_amd/csrc/dataprep.hip): grid subsampling, pc_norm +
sample + class weights for one scan, and the same for a batch of scans.  Imports nothing from geot_amd.

Every row of a table names the branch it exists for.  The bounds those branches sit at are parsed from the sources
(constants()), so a changed constant fails the census of tests/test_dataprep_cases_cpu.py instead of silently un-covering a
branch.  Inputs are seeded numpy.

Referees
  grid subsampling  oracle.np_data.grid_subsampling: the project's restatement, held to the reference's compiled code by
                    tests/test_data_cpu.py and, at the edges used here, by tests/golden/grid_subsampling_edges_ref.npz.
  pc_norm           np_data.pc_norm_f64 for the tolerances; norm_given_centroid() -- numpy's own fp32 statements after the
                    centroid -- fed the kernel's centroid, for the bits.
  class weights     class_weights(): np_data.class_weights for any class count and with labels outside [0, C) dropped.
"""
import os
import re

import numpy as np

from oracle import np_data

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "geot_amd", "csrc")
EDGES = os.path.join(ROOT, "tests", "golden", "grid_subsampling_edges_ref.npz")
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
B_POS = 1e-5                 # the project's bound on a normalised position (tests/test_data_gpu.py, tests/test_views_gpu.py)
TIED_SHARE = 0.10            # most voxels of a fixture case whose label vote may be tied


# ---- the bounds, read from the sources ----------------------------------------------------------------------------------------
def constants():
    src = open(os.path.join(CSRC, "dataprep.hip")).read()
    common = open(os.path.join(CSRC, "geot_common.h")).read()

    def one(pattern, text=src):
        found = re.findall(pattern, text)
        assert len(found) >= 1 and len(set(found)) == 1, (pattern, found)
        return found[0], len(found)

    c = {}
    c["GS_HDR"] = int(one(r"constexpr int GS_HDR = (\d+);")[0])
    (blocks, threads), _ = one(r"constexpr int PN_BLOCKS = (\d+), PN_THREADS = (\d+);")
    c["PN_BLOCKS"], c["PN_THREADS"] = int(blocks), int(threads)
    c["SCAN_CHUNK"] = int(one(r"constexpr int SCAN_CHUNK = (\d+);", common)[0])
    assert "(total + 1 + SCAN_CHUNK - 1) / SCAN_CHUNK" in common                  # scan_blocks: over total + 1 entries
    # the capped grids: gs_bbox, pn_max, pn_sample, pnb_sample -- one workgroup size, one cap
    (cap, cap2), count = one(r"dim3\(nb < (\d+) \? nb : (\d+)")
    assert cap == cap2 and count == 4, (cap, cap2, count)
    c["BLOCK_CAP"] = int(cap)
    (add, div), count = one(r"const int nb = \(\w+ \+ (\d+)\) / (\d+);")
    assert int(add) + 1 == int(div) and count == 4, (add, div, count)
    c["BLOCK"] = int(div)
    for kernel in ("gs_bbox_kernel", "pn_max_kernel", "pn_sample_kernel", "pnb_sample_kernel", "pnb_max_kernel", "gs_key_kernel"):
        assert re.search(r"__launch_bounds__\(%d\) void %s\(" % (c["BLOCK"], kernel), src), kernel
    c["WEIGHT_THREADS"] = int(one(r"hipLaunchKernelGGL\(pn_weights_kernel, dim3\(1\), dim3\((\d+)\)")[0])
    assert one(r"hipLaunchKernelGGL\(pn_weights_kernel, dim3\(1\), dim3\((\d+)\)")[1] == 2          # the m == 0 path too
    assert int(one(r"hipLaunchKernelGGL\(pnb_weights_kernel, dim3\(s\), dim3\((\d+)\)")[0]) == c["WEIGHT_THREADS"]
    assert int(one(r"hipLaunchKernelGGL\(pnb_centroid_kernel, dim3\(s\), dim3\((\d+)\)")[0]) == c["WEIGHT_THREADS"]
    c["PNB_MAX_BLOCKS"] = int(one(r"hipLaunchKernelGGL\(pnb_max_kernel, dim3\((\d+), s\)")[0])
    assert "i += PN_BLOCKS * PN_THREADS" in src
    return c


def gs_branches(n, c=None):
    """The launch branches a grid-subsampling call of n points reaches."""
    c = c or constants()
    blocks = -(-n // c["BLOCK"])
    return {"blocks:1" if blocks == 1 else "blocks:>1",
            "bbox:one-trip" if blocks <= c["BLOCK_CAP"] else "bbox:grid-stride",
            "scan:1-block" if -(-(n + 1) // c["SCAN_CHUNK"]) == 1 else "scan:2-blocks"}


def pn_branches(n, m, classes, c=None):
    """The launch branches geot_pc_norm_stats + geot_cloud_sample reach for n points, m samples and C classes (one slot of
    geot_cloud_sample_batch reaches the same ones, its maximum with a fixed grid of PNB_MAX_BLOCKS workgroups)."""
    c = c or constants()
    out = {"sum:one-trip" if n <= c["PN_BLOCKS"] * c["PN_THREADS"] else "sum:stride",
           "max:one-trip" if -(-n // c["BLOCK"]) <= c["BLOCK_CAP"] else "max:grid-stride",
           "batch-max:one-trip" if n <= c["PNB_MAX_BLOCKS"] * c["BLOCK"] else "batch-max:stride"}
    if m:
        out.add("sample:blocks:1" if m <= c["BLOCK"] else "sample:blocks:>1")
        out.add("sample:one-trip" if -(-m // c["BLOCK"]) <= c["BLOCK_CAP"] else "sample:grid-stride")
    else:
        out.add("sample:none")
    if classes:
        out.add("weights:one-trip" if classes <= c["WEIGHT_THREADS"] else "weights:stride")
        out.add("lds:one-trip" if classes <= c["BLOCK"] else "lds:stride")
    return out


# ---- comparing bits ---------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(got, want):
    """Equality of the stored bits -- -0.0 is not 0.0 -- but for NaNs: a NaN equals any NaN in the same place (0 / 0 has the
    sign bit set on x86 and clear on the device; no statement of the reference tells them apart)."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def first_difference(got, want):
    """A line for an assertion message: shapes, and the first rows that differ."""
    if got.shape != want.shape:
        return "shape %s, expected %s" % (got.shape, want.shape)
    nan = np.isnan(want) & np.isnan(got) if got.dtype.kind == "f" else np.zeros(got.shape, dtype=bool)
    rows = np.flatnonzero(((bits(got) != bits(want)) & ~nan).reshape(len(got), -1).any(axis=1))
    if not len(rows):
        return "equal"
    r = rows[0]
    return "%d of %d rows differ, first row %d: %s, expected %s" % (len(rows), len(got), r, got[r].tolist(), want[r].tolist())


# ---- grid subsampling: the grid, restated with signed indices ---------------------------------------------------------------
def grid_of(points, dl):
    """fp32 origin and the SIGNED cell indices of grid_subsampling.cpp:24-31, 52-56 -> (origin (3,), ijk (n, 3) int64, (NX, NY))."""
    p = np.ascontiguousarray(points, dtype=F32)
    dl = F32(dl)
    inv = F32(1) / dl
    origin = np.floor(p.min(axis=0) * inv).astype(F32) * dl
    ijk = np.floor((p - origin[None, :]) / dl).astype(np.int64)
    top = np.floor((p.max(axis=0) - origin) / dl).astype(np.int64) + 1
    return origin, ijk, (int(top[0]), int(top[1]))


def _cloud(seed, n, fdim, ldim, lo=(-1.0, -0.7, -0.4), hi=(1.0, 0.7, 0.4), labels=(-2, 6)):
    rng = np.random.default_rng(seed)
    p = rng.uniform(lo, hi, (n, 3)).astype(F32)
    if n > 100:
        p[rng.integers(0, n, n // 50)] = p[rng.integers(0, n, n // 50)]
    f = rng.standard_normal((n, fdim)).astype(F32) if fdim else None
    lab = rng.integers(labels[0], labels[1], (n, ldim)).astype(np.int32) if ldim else None
    return p, f, lab


def _two(one_voxel):
    p = np.array([[0.31, 0.32, 0.33], [0.34, 0.35, 0.36] if one_voxel else [0.34, 0.75, 0.36]], dtype=F32)
    f = np.array([[1.5, -2.0], [0.25, 3.0]], dtype=F32)
    return p, f, np.array([[4], [-3]], dtype=np.int32), 0.5


def wide_cloud(ldim=1):
    """300 points in [0, 10)^3, 50 of them near-duplicates of others, for dl = 0.001: about 10^4 cells per axis, keys of 40
    bits.  A near-duplicate carries its source's labels, so a voxel's vote is tied only where two sources meet."""
    rng = np.random.default_rng(7001)
    p = rng.uniform(0, 10, (300, 3)).astype(F32)
    src = rng.integers(0, 250, 50)
    p[250:] = p[src] + rng.uniform(-2e-4, 2e-4, (50, 3)).astype(F32)
    p = np.clip(p, 0, np.nextafter(F32(10), F32(0))).astype(F32)
    f = rng.standard_normal((300, 2)).astype(F32)
    lab = rng.integers(0, 4, (300, ldim)).astype(np.int32)
    lab[250:] = lab[src]
    return p, f, lab, 0.001


# (dl, a cloud's minimum coordinate) for which the fp32 origin lands above the minimum: floor((min - origin) / dl) = -1
NEG_MINIMA = [(0.05, 1.9499999284744263), (0.013, -3.2110002040863037), (0.02, -2.4200000762939453), (0.06, 5.999999523162842)]


def negative_cloud(axis, which, merge=False, n=800):
    """A cloud whose minimum on `axis` is NEG_MINIMA[which]: one point sits there, mid-cloud on the other two axes, so that
    its wrapped key falls between the others'.  The others lie at least 0.001 above it on that axis: over 3.5 cells there
    and four cells on the other axes, and one point alone in the cell above them at the low corner, so the cell the wrapped
    key names -- (NX - 1, iy - 1, iz) for an x index of -1 -- is empty.  merge (axis 0) puts one more point into that cell.
    fdim = 2, ldim = 1 (labels 0..3, 70 % of them 0: few tied votes)."""
    dl, lowest = NEG_MINIMA[which]
    rng = np.random.default_rng(7100 + 10 * axis + which)
    lo = np.array([0.3, -1.1, 2.2], dtype=np.float64)
    lo[axis] = lowest + 0.001
    span = np.full(3, 4 * dl)
    span[axis] = 3.5 * dl
    p = (lo + rng.uniform(0, 1, (n, 3)) * span).astype(F32)
    p[:, axis] = np.maximum(p[:, axis], F32(lowest + 0.001))
    at, top = n // 3, 2 * n // 3
    p[at] = (lo + 2.5 * dl).astype(F32)               # the minimum point
    p[at, axis] = F32(lowest)
    p[top] = (lo + 0.5 * dl).astype(F32)              # the maximum on `axis`, alone in its layer of cells
    p[top, axis] = F32(lo[axis] + 4.5 * dl)
    lab = np.where(rng.uniform(size=(n, 1)) < 0.7, 0, rng.integers(1, 4, (n, 1))).astype(np.int32)
    if merge:
        assert axis == 0
        origin, ijk, _ = grid_of(p, dl)
        extra = p[at].copy()
        extra[0] = p[top, 0]                                          # cell NX - 1
        extra[1] = origin[1] + F32((ijk[at, 1] - 1 + 0.5) * dl)
        p = np.concatenate([p[:n // 2], extra[None], p[n // 2:]])
        lab = np.concatenate([lab[:n // 2], [[3]], lab[n // 2:]]).astype(np.int32)
    f = rng.standard_normal((len(p), 2)).astype(F32)
    return p, f, lab, dl


def order_cloud():
    """One voxel holds x = (1e8, 1, -1e8, 1) in that input order: the sum is 1, every sorted order gives 0 or 2.  The cell is
    1e17 wide -- 1e8 is below the fp32 spacing of the 2e17 the origin lies away, which is what lets both signs share a cell --
    and other voxels lie around it.  A feature column holds the same four values."""
    big = 1e17
    rng = np.random.default_rng(7200)
    around = np.array([[-1.5, 0.2, 0.1], [-0.5, 0.3, 0.2], [1.5, 0.1, 0.3], [0.4, 1.5, 0.2], [0.3, -1.5, 0.1], [-1.5, -1.5, -1.5],
                       [1.5, 1.5, 1.5], [-0.5, 0.35, 0.25]]) * big
    core = np.array([[1e8, 0.2 * big, 0.3 * big], [1.0, 0.25 * big, 0.2 * big], [-1e8, 0.3 * big, 0.1 * big],
                     [1.0, 0.1 * big, 0.25 * big]])
    p = np.concatenate([around[:3], core[:1], around[3:5], core[1:3], around[5:], core[3:]]).astype(F32)
    core_rows = np.array([3, 6, 7, 11])
    f = rng.standard_normal((len(p), 2)).astype(F32)
    f[core_rows, 1] = [1e8, 1.0, -1e8, 1.0]
    return p, f, None, big, core_rows


def label_cloud():
    """Six voxels of planted votes in three label columns (dl = 1, one voxel per unit of x).  Column 0 holds the multisets
    below; columns 1 and 2 hold them shifted by two and four voxels, so every voxel meets three of them."""
    votes = [[5, 3, 5, 3],                                   # two-way tie: 3
             [7, 2, 9, 2, 7, 9],                             # three-way tie: 2
             [1, 1, INT_MAX, INT_MAX, INT_MAX],              # the majority label is the largest
             [INT_MIN, -1, INT_MIN, INT_MAX],                # INT_MIN wins outright
             [INT_MAX, INT_MIN],                             # a tie of the two extremes: INT_MIN
             [-1, -1, 4, 4, 4, -1, 0]]                       # 3 : 3 between -1 and 4: -1
    rng = np.random.default_rng(7300)
    pts, labs = [], []
    for cell in range(len(votes)):               # whole copies of each column's multiset: the proportions of the vote stay
        row = [votes[(cell + 2 * d) % len(votes)] for d in range(3)]
        for j in range(int(np.lcm.reduce([len(v) for v in row]))):
            pts.append([cell + rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9)])
            labs.append([v[j % len(v)] for v in row])
    order = rng.permutation(len(pts))
    return np.asarray(pts, dtype=F32)[order], None, np.asarray(labs, dtype=np.int64).astype(np.int32)[order], 1.0, votes


def _identical(n, value):
    return np.tile(np.asarray(value, dtype=F32), (n, 1))


def _gs_case(name):
    """-> (points, features, labels, dl)."""
    kind = name.split(":")
    if kind[0] == "n":                                       # n:<n>:<fdim>:<ldim>:<dl>
        n, fdim, ldim, dl = int(kind[1]), int(kind[2]), int(kind[3]), float(kind[4])
        return _cloud(7000 + n, n, fdim, ldim) + (dl,)
    if kind[0] == "two":
        return _two(kind[1] == "one-voxel")
    if kind[0] == "big":
        p, f, _ = _cloud(7050, 262145, 1, 0, lo=(0, 0, 0), hi=(1, 1, 1))
        p[-1] = (-0.03, 1.03, 0.5)                           # the last point -- the one the grid-stride loop's second trip
        return p, f, None, 0.07                              # reads -- is the corner of the box; 16 x 16 x 15 cells at most
    if kind[0] == "wide":
        return wide_cloud(int(kind[1]))
    if kind[0] == "flat":                                    # the wide cloud pressed into one layer of finer cells: the order
        p, f, lab, _ = wide_cloud(1)                         # of the keys is decided by NX * iy, which passes 2^32
        p[:, 2] *= F32(1e-6)
        return p, f, lab, 0.0001
    if kind[0] == "neg":
        return negative_cloud(int(kind[1]), int(kind[2]), merge=len(kind) > 3)
    if kind[0] == "order":
        return order_cloud()[:4]
    if kind[0] == "labels":
        return label_cloud()[:4]
    if kind[0] == "same":
        p = _identical(5000, (0.3, -0.7, 1.1))
        rng = np.random.default_rng(7400)
        return p, rng.standard_normal((5000, 1)).astype(F32), rng.integers(0, 3, (5000, 1)).astype(np.int32), 0.1
    if kind[0] == "negzero":
        p = _identical(300, (-0.0, -0.0, -0.0))
        p[::3] = (0.0, -0.0, 0.0)
        p[5] = (0.25, -0.0, 0.0)
        p[6] = (-0.0, 0.35, -0.25)
        return p, None, None, 0.1
    raise KeyError(name)


# name, the branches the case is in the table for
GS_CASES = [
    ("n:1:1:1:0.1", ["blocks:1", "scan:1-block", "size:1"]),
    ("two:one-voxel", ["size:2", "voxels:1"]),
    ("two:two-voxels", ["size:2", "voxels:2"]),
    ("n:255:0:0:0.2", ["blocks:1", "fdim:0"]),
    ("n:256:1:2:0.2", ["blocks:1", "fdim:1"]),
    ("n:257:64:1:0.2", ["blocks:>1", "fdim:64"]),
    ("n:4095:5:1:0.05", ["scan:1-block", "fdim:5"]),
    ("n:4096:0:1:0.05", ["scan:2-blocks"]),
    ("n:4097:1:0:0.05", ["scan:2-blocks"]),
    ("big", ["bbox:grid-stride", "scan:2-blocks"]),
    ("wide:1", ["key:40-bits"]),
    ("wide:2", ["key:40-bits", "label-key:wide-voxel-ids"]),
    ("flat", ["key:iy-term:>32-bits"]),
    ("neg:0:0", ["index:-1:x"]),
    ("neg:1:1", ["index:-1:y"]),
    ("neg:2:2", ["index:-1:z"]),
    ("neg:0:3:merge", ["index:-1:x", "index:-1:merged"]),
    ("order", ["sum:input-order"]),
    ("labels", ["labels:ties", "labels:extremes", "ldim:3", "fdim:0"]),
    ("same", ["extent:0", "voxels:1"]),
    ("negzero", ["coordinate:-0.0"]),
]
GS_NAMES = [name for name, _ in GS_CASES]
FIXTURE_CASES = ["neg:0:0", "neg:1:1", "neg:2:2", "wide:1"]          # tests/golden/grid_subsampling_edges_ref.npz
_GS_CACHE = {}


def gs_case(name):
    """-> dict(p, f, lab, dl, want): the inputs and np_data's result, computed once per process and left unchanged."""
    if name not in _GS_CACHE:
        p, f, lab, dl = _gs_case(name)
        _GS_CACHE[name] = {"p": p, "f": f, "lab": lab, "dl": dl, "want": np_data.grid_subsampling(p, f, lab, dl)}
    return _GS_CACHE[name]


def fixture_key(name):
    return name.replace(":", "_")


# ---- pc_norm / sample / class weights -----------------------------------------------------------------------------------------
def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(F32)).astype(np.float64)


def centroid_bound(pc):
    """|c - mean64| <= ulp32(mean64) / 2 + n 2^-53 mean|x| per axis: the final rounding to fp32, and an fp64 sum of n terms in
    any order (each partial sum within 2^-53 relative of sum|x|) divided by n.  -> (mean64, bound), (3,) each."""
    p64 = np.asarray(pc, dtype=np.float64)
    mean = p64.mean(axis=0)
    return mean, ulp32(mean) / 2 + len(p64) * 2.0 ** -53 * np.abs(p64).mean(axis=0)


def norm_given_centroid(pc, centroid):
    """tooth_dataset.py:110-113 as numpy executes it in fp32, from a given centroid -> (normalised, scale)."""
    q = np.asarray(pc, dtype=F32) - np.asarray(centroid, dtype=F32)
    m = np.max(np.sqrt(np.sum(q ** 2, axis=1)))
    with np.errstate(invalid="ignore", divide="ignore"):
        return q / m, m


def class_weights(sampled_labels, classes):
    """np_data.class_weights for any class count; a label outside [0, C) is dropped from the histogram.  (The reference's
    torch.histogram closes the last bin on the right, so a label of exactly C would count as C - 1 there; its label map never
    produces one.)  No label in range: 0 / 0, every weight NaN."""
    lab = np.asarray(sampled_labels).astype(np.int64).reshape(-1)
    lab = lab[(lab >= 0) & (lab < classes)]
    h = np.bincount(lab, minlength=classes)[:classes].astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = h / h.sum(dtype=F32)
    return np.where(np.isinf(w), F32(0), w).astype(F32)


def _pn_points(kind, n, rng):
    base = rng.standard_normal((n, 3)) * np.array([30, 20, 8])
    if kind == "plain":
        if n > 2:
            base[-1] = (150, -120, 60)             # the last point -- a grid-stride loop's last trip -- is the farthest one
        return (base + np.array([5, -40, 12])).astype(F32)
    if kind == "shifted":
        return (base + np.array([1e4, -1e4, 5e3])).astype(F32)
    if kind == "symmetric":                                    # x and -x in pairs, then a nudge: mean ~ 1e-6 of the extent
        half = base[:n // 2]
        p = np.concatenate([half, -half, np.zeros((n - 2 * (n // 2), 3))])
        return (p + np.array([1e-4, -6e-5, 2e-5])).astype(F32)
    raise KeyError(kind)


def _pn_labels(kind, n, classes, rng):
    if kind == "cover":                                        # every class present among the first C points
        lab = rng.integers(0, classes, n)
        lab[:min(n, classes)] = np.arange(min(n, classes))
    elif kind == "stray":                                      # -1, C and C + 5 among valid labels
        lab = rng.integers(0, classes, n)
        lab[1::7], lab[2::7], lab[3::11] = -1, classes, classes + 5
    elif kind == "all-stray":
        lab = rng.choice([-1, classes, classes + 5, INT_MIN, INT_MAX], n)
    else:
        raise KeyError(kind)
    return lab.astype(np.int32)


def _pn_sel(kind, n, m, classes, rng):
    if kind == "identity":
        assert m == n
        return None
    sel = rng.choice(n, m, replace=n < m)                       # tooth_dataset.py:133-135
    if kind == "cover" and m >= min(n, classes):
        sel[:min(n, classes)] = np.arange(min(n, classes))
    return sel.astype(np.int64)


# name, n, m, classes, points, labels, selection, the branches the case is in the table for
PN_CASES = [
    ("one-point", 1, 5, 1, "plain", "cover", "cover", ["size:1", "scale:0", "repeats", "classes:1"]),
    ("two-points", 2, 1, 17, "plain", "cover", "cover", ["sample:blocks:1", "classes:17"]),
    ("n255", 255, 256, 64, "plain", "cover", "cover", ["repeats", "weights:one-trip", "classes:64", "sample:blocks:1"]),
    ("n256", 256, 257, 65, "plain", "cover", "cover", ["repeats", "weights:stride", "classes:65", "sample:blocks:>1"]),
    ("n257", 257, 257, 257, "plain", "cover", "identity", ["identity", "lds:stride", "classes:257"]),
    ("n65535", 65535, 256, 256, "plain", "cover", "cover", ["sum:one-trip", "lds:one-trip", "classes:256"]),
    ("n65536", 65536, 1, 4096, "plain", "cover", "cover", ["sum:one-trip", "classes:4096", "batch-max:one-trip"]),
    ("n65537", 65537, 262145, 4096, "plain", "cover", "cover",
     ["sum:stride", "batch-max:stride", "sample:grid-stride", "repeats", "classes:4096", "lds:stride"]),
    ("n262145", 262145, 262145, 17, "plain", "cover", "identity", ["max:grid-stride", "sample:grid-stride", "identity", "sum:stride"]),
    ("shifted", 65537, 257, 17, "shifted", "cover", "cover", ["centroid:shifted"]),
    ("symmetric", 20000, 256, 17, "symmetric", "cover", "cover", ["centroid:near-zero"]),
    ("stray-labels", 300, 300, 17, "plain", "stray", "cover", ["labels:stray"]),
    ("all-stray", 300, 64, 17, "plain", "all-stray", "cover", ["labels:all-stray"]),
    ("none-sampled", 300, 0, 17, "plain", "cover", "cover", ["sample:none"]),
]
PN_NAMES = [row[0] for row in PN_CASES]
_PN_CACHE = {}


def pn_case(name):
    """-> dict(n, m, classes, pc, labels, sel (None: identity), idx, q64, c64, m64, weights, branches)."""
    if name not in _PN_CACHE:
        _, n, m, classes, points, labels, selection, claims = PN_CASES[PN_NAMES.index(name)]
        rng = np.random.default_rng(7500 + PN_NAMES.index(name))
        pc = _pn_points(points, n, rng)
        lab = _pn_labels(labels, n, classes, rng)
        sel = _pn_sel(selection, n, m, classes, rng)
        idx = np.arange(n) if sel is None else sel
        q64, c64, m64 = np_data.pc_norm_f64(pc)
        _PN_CACHE[name] = {"n": n, "m": m, "classes": classes, "pc": pc, "labels": lab, "sel": sel, "idx": idx, "q64": q64,
                           "c64": c64, "m64": m64, "weights": class_weights(lab[idx], classes), "claims": claims}
    return _PN_CACHE[name]


# ---- the batch ---------------------------------------------------------------------------------------------------------------
BATCH_SIZES = (1, 300, 65537)
# name, classes, m, the set scan of every slot (None: scan_ids == NULL, slot i is scan i), the branches
BATCH_CASES = [
    ("c1-m1", 1, 1, [2, 0, 1, 2], ["classes:1", "sample:blocks:1", "scan-twice", "out-of-order"]),
    ("c17-m257", 17, 257, [1, 2, 0], ["classes:17", "sample:blocks:>1", "out-of-order", "labels:stray"]),
    ("c65-m1", 65, 1, [0, 1, 2], ["classes:65", "weights:stride"]),
    ("c257-m257", 257, 257, [2, 2, 1], ["classes:257", "lds:stride", "scan-twice"]),
    ("c4096-m257", 4096, 257, [1, 0, 2, 1], ["classes:4096", "scan-twice"]),
    ("identity-s3", 17, 257, None, ["ids:null"]),
    ("identity-s2", 65, 1, None, ["ids:null", "ids:null:s<n_scans"]),
]
BATCH_NAMES = [row[0] for row in BATCH_CASES]
_BATCH_CACHE = {}


def batch_set(classes):
    """The three scans of BATCH_SIZES with labels for `classes` classes (a few outside [0, C) at 17 classes)."""
    if classes not in _BATCH_CACHE:
        rng = np.random.default_rng(7600 + classes)
        scans = [_pn_points("plain", n, rng) + F32(i) for i, n in enumerate(BATCH_SIZES)]
        labels = [_pn_labels("stray" if classes == 17 else "cover", n, classes, rng) for n in BATCH_SIZES]
        _BATCH_CACHE[classes] = (scans, labels)
    return _BATCH_CACHE[classes]


def batch_case(name):
    """-> dict(classes, m, ids (list; identity spelled out), null_ids, scans, labels, sel (s, m) int64)."""
    _, classes, m, ids, claims = BATCH_CASES[BATCH_NAMES.index(name)]
    scans, labels = batch_set(classes)
    null_ids = ids is None
    ids = list(range(2 if name.endswith("s2") else 3)) if null_ids else ids
    rng = np.random.default_rng(7700 + BATCH_NAMES.index(name))
    sel = np.stack([rng.choice(BATCH_SIZES[i], m, replace=BATCH_SIZES[i] < m) for i in ids]).astype(np.int64)
    return {"classes": classes, "m": m, "ids": ids, "null_ids": null_ids, "scans": scans, "labels": labels, "sel": sel,
            "claims": claims}


def unusable_table():
    """A scan table with every kind of unusable entry beside good ones, for geot_cloud_sample_batch called directly.
    The arrays passed as `points` / `labels` start MARGIN rows inside a larger allocation that also extends MARGIN rows past
    `total`, so a kernel that did follow a refused entry would still read inside the allocation.
    -> dict(total, margin, offsets (n_scans + 1), n_scans, ids, why (per slot: None for a usable one), clean_ids)."""
    total, margin = 1000, 64
    offsets = np.array([0, 300, 300, 650, total + 10, -5, 200], dtype=np.int64)
    n_scans = len(offsets) - 1
    slots = [(0, None), (-1, "scan id -1"), (2, None), (n_scans, "scan id n_scans"), (1, "empty scan"),
             (3, "offsets[i + 1] > total"), (5, "offsets[i] < 0"), (2, None)]
    assert margin >= 10 and margin >= 5
    return {"total": total, "margin": margin, "offsets": offsets, "n_scans": n_scans, "ids": [i for i, _ in slots],
            "why": [w for _, w in slots], "clean_ids": [i for i, w in slots if w is None]}
