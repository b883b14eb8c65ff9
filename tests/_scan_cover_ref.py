"""numpy restatement of geot_sample_draw_cover's contract and of geot_scan_cover's ownership rule (include/geot_hip.h), built
on tests/_sample_draw_ref.py: nothing of geot_amd is imported.

    sigma(n, seed, d)                         the walked bijection of draw id d on [0, n), as one (n,) int64 table
    cover_rows(n, m, seed, d, passes)         (len(passes), m) int64: row p holds sigma[(p m + j) mod n], q in python integers
    owners(n, m, p)                           (m,) bool: position p m + j < n -- the samples of pass p that own their vertex
    cover_passes(n, m)                        ceil(n / m)
    sample_draw_cover_ref(sizes, m, seed, draw_base, p)     (sel (S, m) int64, bad (S,) int32); sizes[i] == 0: an unusable slot
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sample_draw_ref as sref  # noqa: E402

_tables = {}


def sigma(n, seed, d):
    """sigma_d(x) for every x of [0, n): the n >= m branch of the sample_draw restatement with m = n (its row IS the table:
    element j is the walk that starts at j)."""
    key = (int(n), int(seed), int(d) & 0xFFFFFFFFFFFFFFFF)
    if key not in _tables:
        _tables[key] = sref.draw_rows(key[0], key[0], key[1], [key[2]])[0]
    return _tables[key]


def cover_passes(n, m):
    return -(-int(n) // int(m))


def cover_rows(n, m, seed, d, passes):
    n, m = int(n), int(m)
    table = sigma(n, seed, d)
    out = np.empty((len(passes), m), dtype=np.int64)
    for row, p in enumerate(passes):
        first = (int(p) * m) % n                     # python integers: no width to overflow
        out[row] = table[(first + np.arange(m, dtype=np.int64)) % n]
    return out


def owners(n, m, p):
    return int(p) * int(m) + np.arange(int(m), dtype=np.int64) < int(n) if int(p) * int(m) < int(n) else np.zeros(int(m), dtype=bool)


def sample_draw_cover_ref(sizes, m, seed, draw_base, p):
    sel = np.zeros((len(sizes), int(m)), dtype=np.int64)
    bad = np.zeros(len(sizes), dtype=np.int32)
    for i, n in enumerate(sizes):
        if int(n) == 0:
            bad[i] = 2
            continue
        sel[i] = cover_rows(n, m, seed, (int(draw_base) + i) & 0xFFFFFFFFFFFFFFFF, [p])[0]
    return sel, bad
