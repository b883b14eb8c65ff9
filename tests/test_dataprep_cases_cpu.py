"""Census of the case tables of tests/_dataprep_ref.py (the GPU suite is tests/test_dataprep_gpu.py), without a GPU.

From the constants parsed out of csrc/dataprep.hip and csrc/geot_common.h: on which side of every launch bound each case
lies -- workgroup count against its cap, blocks of the head-flag scan, the stride of the fp64 sum, trips of the class loops --
that every branch the tables name is reached and that every case reaches what it claims.  The preconditions the GPU tests
lean on: a cell index of -1 where a case says so, 40-bit keys, the planted label votes, the input-order sum.  And np_data --
the referee of every grid case -- against the reference's compiled rows at those edges
(tests/golden/grid_subsampling_edges_ref.npz)."""
import numpy as np
import pytest

import _dataprep_ref as R
from oracle import np_data
from test_data_cpu import compare_with_reference_rows


@pytest.fixture(scope="module")
def consts():
    return R.constants()


def test_parsed_constants_are_the_bounds_the_tables_were_written_for(consts):
    assert consts == {"GS_HDR": 8, "PN_BLOCKS": 256, "PN_THREADS": 256, "SCAN_CHUNK": 4096, "BLOCK_CAP": 1024, "BLOCK": 256,
                      "WEIGHT_THREADS": 64, "PNB_MAX_BLOCKS": 256}


def _gs_reached(name, consts):
    c = R.gs_case(name)
    p, f, lab, want = c["p"], c["f"], c["lab"], c["want"]
    n = len(p)
    _, ijk, (nx, ny) = R.grid_of(p, c["dl"])
    out = R.gs_branches(n, consts)
    if ijk.min() >= 0 and nx * int(ijk[:, 1].max()) >= 2 ** 32:
        cut = ijk[:, 0] + (nx * ijk[:, 1]) % 2 ** 32 + nx * ny * ijk[:, 2]
        full = ijk[:, 0] + nx * ijk[:, 1] + nx * ny * ijk[:, 2]
        if not np.array_equal(np.argsort(cut, kind="stable"), np.argsort(full, kind="stable")):
            out.add("key:iy-term:>32-bits")              # and a term cut to 32 bits would change the order of the rows
    out |= {"size:%d" % n, "voxels:%d" % len(want["points"]), "fdim:%d" % (0 if f is None else f.shape[1]),
            "ldim:%d" % (0 if lab is None else lab.shape[1])}
    for axis, letter in enumerate("xyz"):
        if (ijk[:, axis] == -1).any():
            out.add("index:-1:" + letter)
    if (ijk == -1).any() and len(want["points"]) == len(np.unique(ijk, axis=0)) - 1:
        out.add("index:-1:merged")
    bits = int(want["keys"][want["keys"] < 2 ** 63].max()).bit_length()
    if bits > 32:
        out.add("key:%d-bits" % bits)
        if lab is not None and lab.shape[1] >= 2 and len(want["points"]) > 256:
            out.add("label-key:wide-voxel-ids")
    if np.ptp(p, axis=0).max() == 0:
        out.add("extent:0")
    if (np.signbit(p) & (p == 0)).any():
        out.add("coordinate:-0.0")
    if lab is not None:
        if want["tied"].any():
            out.add("labels:ties")
        if {R.INT_MIN, R.INT_MAX, -1} <= set(lab.reshape(-1).tolist()):
            out.add("labels:extremes")
    if name == "order":
        out.add("sum:input-order")
    return out


def test_every_grid_case_reaches_what_it_claims_and_every_branch_is_reached(consts):
    reached = set()
    for name, claims in R.GS_CASES:
        got = _gs_reached(name, consts)
        assert set(claims) <= got, (name, sorted(set(claims) - got))
        reached |= got
    need = {"blocks:1", "blocks:>1", "bbox:one-trip", "bbox:grid-stride", "scan:1-block", "scan:2-blocks", "size:1", "size:2",
            "size:255", "size:256", "size:257", "size:4095", "size:4096", "size:4097", "size:262145", "voxels:1", "voxels:2",
            "fdim:0", "fdim:1", "fdim:5", "fdim:64", "ldim:0", "ldim:1", "ldim:2", "ldim:3", "index:-1:x", "index:-1:y",
            "index:-1:z", "index:-1:merged", "key:40-bits", "key:iy-term:>32-bits", "label-key:wide-voxel-ids",
            "extent:0", "coordinate:-0.0", "labels:ties", "labels:extremes", "sum:input-order"}
    assert need <= reached, sorted(need - reached)
    # the two sides of every bound are one point apart
    assert R.gs_branches(consts["BLOCK"], consts) != R.gs_branches(consts["BLOCK"] + 1, consts)
    assert R.gs_branches(consts["SCAN_CHUNK"] - 1, consts) != R.gs_branches(consts["SCAN_CHUNK"], consts)
    cap = consts["BLOCK"] * consts["BLOCK_CAP"]
    assert R.gs_branches(cap, consts) != R.gs_branches(cap + 1, consts) and cap + 1 == 262145
    big = R.gs_case("big")
    assert len(big["want"]["points"]) <= 4000 and big["f"].shape[1] == 1 and big["lab"] is None
    # the one point past the capped grid's first trip decides the box: a skipped second trip cannot go unnoticed
    assert big["p"][-1, 0] < big["p"][:cap, 0].min() and big["p"][-1, 1] > big["p"][:cap, 1].max()


def test_negative_index_cases_have_an_index_of_minus_one_and_wrap_as_the_reference_does():
    """floor((min - origin) / dl) == -1 in fp32 for the minimum point, nowhere else; its key is the wrapped one; without
    the planted neighbour no two cells share a key, with it the minimum point's cell merges into (NX - 1, iy - 1, iz)."""
    for name in ("neg:0:0", "neg:1:1", "neg:2:2", "neg:0:3:merge"):
        c = R.gs_case(name)
        axis, which = int(name.split(":")[1]), int(name.split(":")[2])
        dl, lowest = R.NEG_MINIMA[which]
        p = c["p"]
        assert c["dl"] == dl and p[:, axis].min() == np.float32(lowest)
        origin, ijk, (nx, ny) = R.grid_of(p, dl)
        at = int(np.argmin(p[:, axis]))
        assert origin[axis] > p[at, axis] and ijk[at, axis] == -1 and (ijk == -1).sum() == 1 and ijk.min() == -1
        assert np.sort(p[:, axis])[1] >= np.float32(lowest) + np.float32(0.001) - np.spacing(np.float32(abs(lowest) + 1))
        others = [a for a in range(3) if a != axis]
        assert all(np.ptp(ijk[:, a]) >= 1 for a in others)                      # more than one cell on the other two axes
        assert c["f"].shape[1] == 2 and c["lab"].shape[1] == 1
        keys, (knx, kny) = np_data.grid_keys(p, dl)
        assert (knx, kny) == (nx, ny)
        stride = np.array([1, nx, nx * ny], dtype=object)
        assert int(keys[at]) == int((ijk[at].astype(object) * stride).sum()) % 2 ** 64
        cells, rows = len(np.unique(ijk, axis=0)), len(c["want"]["points"])
        if name.endswith("merge"):
            target = np.array([nx - 1, ijk[at, 1] - 1, ijk[at, 2]])
            assert (ijk == target).all(axis=1).any() and int(keys[at]) == int((target.astype(object) * stride).sum())
            assert rows == cells - 1
        else:
            assert rows == cells
        if axis < 2:            # a saturating conversion (2^32 - 1) would sort the point last: the wrapped key does not
            assert 0 < np.searchsorted(c["want"]["keys"], keys[at]) < rows - 1


def test_wide_key_cases_need_more_than_32_bits():
    for name in ("wide:1", "wide:2"):
        c = R.gs_case(name)
        keys = c["want"]["keys"]
        assert int(keys.max()).bit_length() == 40 and (keys >> np.uint64(32) > 0).mean() > 0.9
        assert len(np.unique(keys & np.uint64(0xffffffff))) <= len(keys)
        assert len(c["p"]) == 300 and c["dl"] == 0.001 and 250 < len(keys) < 300       # near-duplicates share voxels
    assert R.gs_case("wide:2")["lab"].shape[1] == 2


def test_order_case_sums_to_one_in_input_order_only():
    p, f, _, dl, rows = R.order_cloud()
    keys, _ = np_data.grid_keys(p, dl)
    assert len(set(keys[rows].tolist())) == 1 and (keys == keys[rows[0]]).sum() == 4 and len(set(keys.tolist())) > 4
    assert list(rows) == sorted(rows)
    for column in (p[rows, 0], f[rows, 1]):
        assert column.tolist() == [1e8, 1.0, -1e8, 1.0]
        acc = np.float32(0)
        for v in column:
            acc = acc + v
        assert acc == 1
        for other in (column[::-1], np.sort(column), np.sort(column)[::-1], column[[0, 2, 1, 3]]):
            acc = np.float32(0)
            for v in other:
                acc = acc + v
            assert acc in (0, 2)
    want = R.gs_case("order")["want"]
    at = int(np.flatnonzero(want["count"] == 4)[0])
    assert want["points"][at, 0] == 0.25 and want["features"][at, 1] == 0.25


def test_label_case_holds_the_planted_votes():
    p, _, lab, dl, votes = R.label_cloud()
    want = R.gs_case("labels")["want"]
    winners = [3, 2, R.INT_MAX, R.INT_MIN, R.INT_MIN, -1]
    tied = [True, True, False, False, True, True]
    assert len(want["points"]) == len(votes)
    for cell in range(len(votes)):
        for d in range(3):
            v = (cell + 2 * d) % len(votes)
            assert want["labels"][cell, d] == winners[v] and want["tied"][cell, d] == tied[v]
    assert max(votes[2]) == winners[2]                              # a majority label that is the voxel's largest
    ways = [sum(v.count(l) == max(map(v.count, v)) for l in set(v)) for v in votes]
    assert ways == [2, 3, 1, 1, 2, 2]                               # two-way and three-way ties


def test_np_data_equals_the_compiled_reference_at_the_edges():
    """The oracle is pinned to the reference's own compiled code where the kernel is judged by it: an index of -1 on every
    axis and 40-bit keys.  At most a tenth of a case's voxels may have a tied vote (they are left out of the comparison)."""
    z = np.load(R.EDGES)
    assert sorted({k.rsplit("_", 2)[0] if "_ref_" in k else k.rsplit("_", 1)[0] for k in z.files}) == \
        sorted(R.fixture_key(n) for n in R.FIXTURE_CASES)
    for name in R.FIXTURE_CASES:
        c, key = R.gs_case(name), R.fixture_key(name)
        for part, arr in (("points", c["p"]), ("features", c["f"]), ("labels", c["lab"])):
            assert R.same_bits(z[key + "_" + part], arr), (name, part)         # the fixture's inputs are the table's
        assert float(z[key + "_dl"]) == np.float32(c["dl"])
        assert c["want"]["tied"].any(axis=1).mean() <= R.TIED_SHARE
        compare_with_reference_rows(c["want"], z[key + "_ref_points"], z[key + "_ref_features"], z[key + "_ref_labels"])
    if np_data.have_reference():          # where oracle/build_ref.py built it: the library itself, the merged cell included
        for name in R.FIXTURE_CASES + ["neg:0:3:merge", "wide:2"]:
            c = R.gs_case(name)
            r = np_data.grid_subsampling_reference(c["p"], c["f"], c["lab"], c["dl"])
            compare_with_reference_rows(c["want"], r["points"], r["features"], r["labels"])


def test_every_scan_case_reaches_what_it_claims_and_every_branch_is_reached(consts):
    reached = set()
    for name, n, m, classes, points, labels, selection, claims in R.PN_CASES:
        c = R.pn_case(name)
        got = R.pn_branches(n, m, classes, consts) | {"size:%d" % n, "samples:%d" % m, "classes:%d" % classes}
        if c["m64"] == 0:
            got.add("scale:0")
        if m > n:
            got.add("repeats")
            assert len(np.unique(c["idx"])) < m
        if c["sel"] is None:
            got.add("identity")
        stray = (c["labels"][c["idx"]] < 0) | (c["labels"][c["idx"]] >= classes)
        if stray.all() and m:
            got.add("labels:all-stray")
            assert np.isnan(c["weights"]).all()
        elif stray.any():
            got.add("labels:stray")
            assert {-1, classes, classes + 5} <= set(c["labels"][c["idx"]].tolist())
        else:
            assert np.array_equal(c["weights"], np_data.class_weights(c["labels"][c["idx"]], classes)) or m == 0
        if classes <= 257 and m >= classes and labels == "cover":
            assert set(c["labels"][c["idx"]].tolist()) == set(range(classes)), name          # every class is present
        if points == "shifted":
            got.add("centroid:shifted")
            assert np.allclose(c["c64"], [1e4, -1e4, 5e3], atol=2)
        if points == "symmetric":
            got.add("centroid:near-zero")
            assert np.abs(c["c64"]).max() < 3e-6 * np.ptp(c["pc"], axis=0).min()
        if n > 2 and points == "plain":            # the last point is the farthest: the scale hangs on a loop's last trip
            r = np.sqrt(((c["pc"].astype(np.float64) - c["c64"]) ** 2).sum(axis=1))
            assert r.argmax() == n - 1 and r[-1] > 1.2 * r[:-1].max()
        assert set(claims) <= got, (name, sorted(set(claims) - got))
        reached |= got
    need = {"sum:one-trip", "sum:stride", "max:one-trip", "max:grid-stride", "batch-max:one-trip", "batch-max:stride",
            "sample:blocks:1", "sample:blocks:>1", "sample:one-trip", "sample:grid-stride", "sample:none", "weights:one-trip",
            "weights:stride", "lds:one-trip", "lds:stride", "scale:0", "repeats", "identity", "labels:stray", "labels:all-stray",
            "centroid:shifted", "centroid:near-zero"}
    need |= {"size:%d" % n for n in (1, 2, 255, 256, 257, 65535, 65536, 65537, 262145)}
    need |= {"samples:%d" % m for m in (0, 1, 256, 257, 262145)} | {"classes:%d" % c for c in (1, 17, 64, 65, 256, 257, 4096)}
    assert need <= reached, sorted(need - reached)
    stride = consts["PN_BLOCKS"] * consts["PN_THREADS"]
    assert stride == 65536 and R.pn_branches(stride, 1, 1, consts) != R.pn_branches(stride + 1, 1, 1, consts)
    assert R.pn_branches(9, 9, consts["WEIGHT_THREADS"], consts) != R.pn_branches(9, 9, consts["WEIGHT_THREADS"] + 1, consts)
    assert R.pn_branches(9, 9, consts["BLOCK"], consts) != R.pn_branches(9, 9, consts["BLOCK"] + 1, consts)


def test_every_batch_case_reaches_what_it_claims_and_every_branch_is_reached(consts):
    reached = set()
    for name, classes, m, ids, claims in R.BATCH_CASES:
        c = R.batch_case(name)
        got = {"classes:%d" % classes, "samples:%d" % m}
        for i in c["ids"]:
            got |= R.pn_branches(R.BATCH_SIZES[i], m, classes, consts) | {"size:%d" % R.BATCH_SIZES[i]}
        if len(set(c["ids"])) < len(c["ids"]):
            got.add("scan-twice")
        if c["ids"] != sorted(c["ids"]):
            got.add("out-of-order")
        if c["null_ids"]:
            got.add("ids:null")
            if len(c["ids"]) < len(R.BATCH_SIZES):
                got.add("ids:null:s<n_scans")
        labels = np.concatenate([c["labels"][i][row] for i, row in zip(c["ids"], c["sel"])])
        if ((labels < 0) | (labels >= classes)).any():
            got.add("labels:stray")
        assert c["sel"].shape == (len(c["ids"]), m) and all((row < R.BATCH_SIZES[i]).all() for i, row in zip(c["ids"], c["sel"]))
        assert set(claims) <= got, (name, sorted(set(claims) - got))
        reached |= got
    need = {"classes:%d" % c for c in (1, 17, 65, 257, 4096)} | {"samples:1", "samples:257", "size:1", "size:300", "size:65537",
            "scan-twice", "out-of-order", "ids:null", "ids:null:s<n_scans", "sum:stride", "batch-max:stride", "weights:stride",
            "lds:stride", "sample:blocks:1", "sample:blocks:>1", "labels:stray"}
    assert need <= reached, sorted(need - reached)
    t = R.unusable_table()
    off, total = t["offsets"], t["total"]
    kinds = set()
    for i, why in zip(t["ids"], t["why"]):
        usable = 0 <= i < t["n_scans"] and off[i] >= 0 and off[i + 1] <= total and off[i + 1] > off[i]
        assert usable == (why is None), (i, why)
        if 0 <= i < t["n_scans"]:                          # a refused entry, if followed, stays inside the margins
            assert off[i] >= -t["margin"] and off[i + 1] <= total + t["margin"]
        kinds.add(why)
    assert kinds == {None, "scan id -1", "scan id n_scans", "empty scan", "offsets[i + 1] > total", "offsets[i] < 0"}
    assert t["clean_ids"] == [0, 2, 2]


def test_referees_hold_their_own_bounds():
    """numpy's fp32 statements from the fp64 centroid rounded to fp32 stay within B_POS of the fp64 pipeline on every case:
    the bound the kernels are held to is one their referee meets."""
    for name in R.PN_NAMES:
        c = R.pn_case(name)
        if c["n"] == 1:
            continue
        q, scale = R.norm_given_centroid(c["pc"], c["c64"].astype(np.float32))
        assert abs(scale - c["m64"]) <= 1e-5 * c["m64"]
        assert np.abs(q - c["q64"]).max() <= R.B_POS, name
    assert np.isnan(R.class_weights([-1, 17], 17)).all() and R.class_weights([], 3).shape == (3,)
    assert R.class_weights([0, 0, 1, 5, -1, 3], 3).tolist() == [np.float32(2) / np.float32(3), np.float32(1) / np.float32(3), 0]
