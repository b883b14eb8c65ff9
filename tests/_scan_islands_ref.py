"""geot_scan_islands (include/geot_hip.h) restated in numpy, rule by rule, and not by the kernel's algorithm: the components
come from iterating comp = min(comp, comp[neighbours]) over the symmetrised same-label edges to the fixed point; sizes, the
largest piece, islands, votes and stats are then taken literally from the header's text.  Integers only: array_equal."""
import numpy as np


def existing(nbr, m):
    """(m, k) mask of the entries of a slot's table that exist: not negative, below m, not the row's own vertex."""
    nbr = np.asarray(nbr).reshape(m, -1)
    return (nbr >= 0) & (nbr < m) & (nbr != np.arange(m)[:, None])


def components(labels, nbr, c):
    """comp (m,) int32: the lowest vertex index of every vertex's component; a label outside [0, c) is its own."""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    m = labels.size
    nbr = np.asarray(nbr, dtype=np.int64).reshape(m, -1)
    ok = existing(nbr, m)
    v, e = np.nonzero(ok)
    u = nbr[v, e]
    valid = (labels >= 0) & (labels < c)
    edge = valid[v] & (labels[v] == labels[u])
    a, b = np.concatenate([v[edge], u[edge]]), np.concatenate([u[edge], v[edge]])     # the edge is not directed
    comp = np.arange(m, dtype=np.int64)
    while True:
        new = comp.copy()
        np.minimum.at(new, a, comp[b])
        new = new[new]                              # (comp[v] is always a member of v's component: so is comp[comp[v]])
        if np.array_equal(new, comp):
            return comp.astype(np.int32)
        comp = new


def scan_islands_slot(labels, nbr, c, min_size, keep=0, allowed=None):
    """One usable slot -> (new labels int64, comp int32, [components, islands, changed, stranded])."""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    m = labels.size
    nbr = np.asarray(nbr, dtype=np.int64).reshape(m, -1)
    allowed = 0xffffffff if allowed is None else int(allowed)
    keep = int(keep)
    comp = components(labels, nbr, c)
    valid = (labels >= 0) & (labels < c)
    roots = [int(r) for r in np.unique(comp[valid])]
    count = np.bincount(comp[valid], minlength=m + 1)
    size = {r: int(count[r]) for r in roots}
    largest = {}
    for r in roots:                                 # ascending roots: among equal sizes the first (lowest) stays
        i = int(labels[r])
        if i not in largest or size[r] > size[largest[i]]:
            largest[i] = r
    island = {}
    for r in roots:
        i = int(labels[r])
        island[r] = bool(size[r] < min_size or not (allowed >> i) & 1 or ((keep >> i) & 1 and largest[i] != r))
    ok = existing(nbr, m)
    out = labels.copy()
    changed = stranded = 0
    for r in roots:
        if not island[r]:
            continue
        i = int(labels[r])
        votes = np.zeros(c, dtype=np.int64)
        for v in np.nonzero((comp == r) & valid)[0]:
            for u in nbr[v][ok[v]]:                 # forward entries only, a duplicate counts again
                lu = int(labels[u])
                if 0 <= lu < c and lu != i and not island[int(comp[u])]:
                    votes[lu] += 1
        if votes.max() == 0:
            stranded += size[r]
            continue
        out[(comp == r) & valid] = int(np.argmax(votes))        # the first maximum: the lowest class among equals
        changed += size[r]
    return out, comp, [len(roots), sum(island.values()), changed, stranded]


def scan_islands(preds, nbrs, c, min_size, keep=None, allowed=None, usable=None):
    """Per-slot lists -> (labels list, comp list, (b, 4) int32 stats); usable[s] False: the slot is skipped (labels as they
    came, comp None, stats zero)."""
    outs, comps, stats = [], [], np.zeros((len(preds), 4), dtype=np.int32)
    for s, (p, t) in enumerate(zip(preds, nbrs)):
        if usable is not None and not usable[s]:
            outs.append(np.asarray(p, dtype=np.int64).copy())
            comps.append(None)
            continue
        o, cp, st = scan_islands_slot(p, t, c, min_size, 0 if keep is None else keep[s], None if allowed is None else allowed[s])
        outs.append(o)
        comps.append(cp)
        stats[s] = st
    return outs, comps, stats


def knn_table(points, k1):
    """The (m, k1) table of the k1 nearest vertices by (d2, index), d2 = ((dx dx) + (dy dy)) + (dz dz) in fp32 without
    contraction -- geot_knn_sorted's order; the vertex itself (d2 = 0) is among them."""
    p = np.asarray(points, dtype=np.float32)
    m = len(p)
    out = np.empty((m, k1), dtype=np.int32)
    for lo in range(0, m, 1024):
        q = p[lo:lo + 1024]
        d = q[:, None, :] - p[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        out[lo:lo + 1024] = np.argsort(d2, axis=1, kind="stable")[:, :k1]
    return out


def surface_scan(m, seed, teeth=6, extent=40.0):
    """A surface-like cloud with blob "teeth": m points on a gently curved sheet in a spatially coherent order (sorted along
    x), labels 1 .. teeth inside discs around well-separated centres and 0 (the gingiva) elsewhere -> (points fp32, labels)."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, extent, size=(m, 2))
    xy = xy[np.argsort(xy[:, 0], kind="stable")]
    z = 2.0 * np.sin(xy[:, 0] / 7.0) + 1.5 * np.cos(xy[:, 1] / 5.0)
    pts = np.concatenate([xy, z[:, None]], 1).astype(np.float32)
    cols = int(np.ceil(np.sqrt(teeth)))
    step = extent / cols
    labels = np.zeros(m, dtype=np.int64)
    for t in range(teeth):
        cx, cy = (t % cols + 0.5) * step, (t // cols + 0.5) * step
        labels[(xy[:, 0] - cx) ** 2 + (xy[:, 1] - cy) ** 2 < (0.32 * step) ** 2] = t + 1
    return pts, labels


def inject(labels, nbr, seed, clusters, size, teeth):
    """Small clusters of a WRONG tooth label strictly inside teeth: `clusters` seeds, each with the first size - 1 entries of
    its row, taken only where every entry of every member's row carries the seed's tooth label and no member or entry of an
    earlier cluster is touched -- so every member keeps neighbours of its true tooth that are in no cluster.
    -> (noisy labels, the injected vertex indices)."""
    rng = np.random.default_rng(seed)
    labels = np.asarray(labels, dtype=np.int64)
    out = labels.copy()
    taken = np.zeros(labels.size, dtype=bool)
    members = []
    for v in rng.permutation(labels.size):
        if len(members) == clusters:
            break
        if labels[v] == 0:
            continue
        group = np.unique(np.concatenate([[v], nbr[v][:size]]))[:size]
        reach = np.unique(nbr[group].reshape(-1))
        if (labels[reach] != labels[v]).any() or taken[reach].any() or taken[group].any():
            continue
        taken[reach] = True
        taken[group] = True
        out[group] = (labels[v] - 1 + 1 + int(rng.integers(teeth - 1))) % teeth + 1       # another tooth, never the gingiva
        members.append(group)
    assert len(members) == clusters, "inject: only %d of %d clusters placed" % (len(members), clusters)
    return out, np.concatenate(members)


# The synthetic property case of the tests: (vertices, scan seed, injection seed) of two scans; five clusters of six vertices of
# a wrong tooth label strictly inside other teeth, below min_size = 10.  tests/test_scan_islands_cpu.py checks that the
# restatement alone restores the uninjected labels exactly for THESE placements; the GPU test relies on that.
PROPERTY_SCANS = ((3000, 3, 5), (2500, 5, 6))
PROPERTY_K, PROPERTY_MIN_SIZE, PROPERTY_TEETH, PROPERTY_KEEP = 8, 10, 6, 0x1fffe       # keep: every class from 1 up, c = 17


def property_case():
    """-> per scan (points, true labels, (M, 9) table, noisy labels)."""
    out = []
    for m, seed, noise in PROPERTY_SCANS:
        pts, labels = surface_scan(m, seed, PROPERTY_TEETH)
        nbr = knn_table(pts, PROPERTY_K + 1)
        noisy, _ = inject(labels, nbr, noise, 5, 6, PROPERTY_TEETH)
        out.append((pts, labels, nbr, noisy))
    return out
