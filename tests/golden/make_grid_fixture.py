"""Regenerate tests/golden/grid_subsampling_ref.npz, grid_subsampling_compiled_ref.npz and grid_subsampling_edges_ref.npz
(run where the reference checkout is present).

    python oracle/build_ref.py && python tests/golden/make_grid_fixture.py [edges]

("edges" writes grid_subsampling_edges_ref.npz alone.)

Inputs: seeded clouds (with duplicate points and negative coordinates).  Expected outputs: what the
REFERENCE's own grid_subsampling() returns for them -- compiled from /root/reference by oracle/build_ref.py
into oracle/_ref/ -- in the reference's own row order.  grid_subsampling_ref.npz holds inputs and outputs only;
grid_subsampling_compiled_ref.npz only digests and labels (compiled_cases); grid_subsampling_edges_ref.npz the clouds of
tests/_dataprep_ref.py at which a cell index is -1 or a key 40 bits wide, inputs and outputs (edge_cases).
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import np_data  # noqa: E402

CASES = [  # name, n, dl, fdim, ldim, scale
    ("a", 1500, 0.10, 0, 0, (1.0, 0.7, 0.4)),
    ("b", 2000, 0.05, 2, 1, (1.0, 1.0, 0.3)),
    ("c", 800, 0.30, 1, 2, (2.0, 0.5, 0.5)),
]
# tests/test_data_cpu.py::test_grid_subsampling_restatement_matches_compiled_reference: seed, n, dl, fdim, ldim
COMPILED_CASES = [(0, 5000, 0.1, 0, 0), (1, 20000, 0.05, 4, 1), (2, 3000, 0.3, 2, 2),
                  (3, 1, 0.1, 1, 1), (4, 60, 10.0, 1, 1), (5, 40000, 0.013, 1, 1)]


def main():
    assert np_data.have_reference(), "run oracle/build_ref.py first"
    out = {}
    for i, (name, n, dl, fdim, ldim, scale) in enumerate(CASES):
        rng = np.random.default_rng(4100 + i)
        p = (rng.standard_normal((n, 3)) * np.array(scale)).astype(np.float32)
        p[rng.integers(0, n, n // 40)] = p[rng.integers(0, n, n // 40)]
        f = rng.standard_normal((n, fdim)).astype(np.float32) if fdim else None
        lab = rng.integers(-1, 5, (n, ldim)).astype(np.int32) if ldim else None
        r = np_data.grid_subsampling_reference(p, f, lab, dl)
        out[name + "_points"], out[name + "_dl"] = p, np.float32(dl)
        out[name + "_ref_points"] = r["points"]
        if fdim:
            out[name + "_features"], out[name + "_ref_features"] = f, r["features"]
        if ldim:
            out[name + "_labels"], out[name + "_ref_labels"] = lab, r["labels"]
    np.savez_compressed(os.path.join(HERE, "grid_subsampling_ref.npz"), **out)
    print("wrote", sorted(out))
    compiled_cases()
    edge_cases()


def edge_cases():
    """grid_subsampling_edges_ref.npz: the clouds of tests/_dataprep_ref.py's FIXTURE_CASES -- one per axis whose minimum
    point gets a cell index of -1, and the cloud whose keys are 40 bits wide -- with the reference's rows for them, keyed
    "<case>_<name>" as in grid_subsampling_ref.npz.  Inputs and outputs only."""
    sys.path.insert(0, os.path.dirname(HERE))
    import _dataprep_ref as R
    out = {}
    for case in R.FIXTURE_CASES:
        c, name = R.gs_case(case), R.fixture_key(case)
        origin, ijk, _ = R.grid_of(c["p"], c["dl"])
        assert ("neg" in case) == bool((ijk == -1).any()), case
        share = c["want"]["tied"].any(axis=1).mean()
        assert share <= R.TIED_SHARE, (case, share)
        r = np_data.grid_subsampling_reference(c["p"], c["f"], c["lab"], c["dl"])
        out[name + "_points"], out[name + "_dl"] = c["p"], np.float32(c["dl"])
        out[name + "_features"], out[name + "_labels"] = c["f"], c["lab"]
        out[name + "_ref_points"], out[name + "_ref_features"], out[name + "_ref_labels"] = r["points"], r["features"], r["labels"]
    np.savez_compressed(os.path.join(HERE, "grid_subsampling_edges_ref.npz"), **out)
    print("wrote", sorted(out))


def compiled_case_inputs(seed, n, fdim, ldim):
    """The seeded cloud of one COMPILED_CASES entry (the test regenerates it; the fixture keeps its digest)."""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal((n, 3)) * np.array([1, 0.7, 0.4])).astype(np.float32)
    if n > 100:
        p[rng.integers(0, n, n // 50)] = p[rng.integers(0, n, n // 50)]
    f = rng.standard_normal((n, fdim)).astype(np.float32) if fdim else None
    lab = rng.integers(-2, 6, (n, ldim)).astype(np.int32) if ldim else None
    return p, f, lab


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def compiled_cases():
    """grid_subsampling_compiled_ref.npz, keyed "<seed>_<name>": the digest of the case's inputs, and of the reference's
    rows for them sorted by np_data.row_order (points; features), the row count, and the sorted labels themselves (int8:
    they are compared only where the vote is not tied)."""
    out = {}
    for seed, n, dl, fdim, ldim in COMPILED_CASES:
        p, f, lab = compiled_case_inputs(seed, n, fdim, ldim)
        r = np_data.grid_subsampling_reference(p, f, lab, dl)
        order = np_data.row_order(r["points"])
        out["%d_inputs_sha256" % seed] = np.array(digest(p, f, lab))
        out["%d_rows" % seed] = np.int64(len(order))
        out["%d_points_sha256" % seed] = np.array(digest(r["points"][order]))
        if fdim:
            out["%d_features_sha256" % seed] = np.array(digest(r["features"][order]))
        if ldim:
            assert r["labels"].min() >= -128 and r["labels"].max() <= 127
            out["%d_ref_labels" % seed] = r["labels"][order].astype(np.int8)
    np.savez_compressed(os.path.join(HERE, "grid_subsampling_compiled_ref.npz"), **out)
    print("wrote", sorted(out))


if __name__ == "__main__":
    if sys.argv[1:] == ["edges"]:            # the edge fixture alone: the other two files keep their bytes
        assert np_data.have_reference(), "run oracle/build_ref.py first"
        edge_cases()
    else:
        main()
