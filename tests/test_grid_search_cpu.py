"""CPU suite: the census of tests/test_grid_search_gpu.py, with no GPU.

knn_grid_kernel and ball_grid_kernel pick a branch per query from the data.  tests/_grid_ref.py restates the grid in fp32
NumPy and names the branch of every query of every GPU case; here each class a case is meant to reach must hold at least
MIN_PER_CLASS queries that are not marginal (a query is marginal when its class changes with the certified radius scaled
by 1 +- 1e-5), and at most MARGINAL_CAP of a case's queries may be marginal.  The model is checked against grids that can
be written down by hand.  The classifier names branches only; every expected result of the GPU file comes from the CPU
oracle.
"""
import numpy as np
import pytest

import _grid_ref as R
from _grid_ref import F


@pytest.fixture(scope="module")
def lib():
    from geot_amd import _lib
    return _lib.load()


@pytest.fixture()
def grid_env(monkeypatch):
    monkeypatch.setenv("GEOT_NN_IMPL", "grid")


def _table(title, counts, classes):
    rows = ["%s\n%-10s" % (title, "cloud") + "".join("%19s" % c for c in classes)]
    for name in R.CLOUDS + ("any",):
        rows.append("%-10s" % name + "".join("%19d" % counts.get((name, c), 0) for c in classes))
    return "\n".join(rows)


# ---- the inputs sit where the issue puts them -------------------------------------------------------------------------
def test_inputs_sit_on_the_eligibility_floor_and_off_the_workgroup_size(lib, grid_env):
    for k in R.KNN_KS:
        assert lib.geot_knn_grid_eligible(len(R.CLOUDS), R.NQ, R.NR, k) == 1
        assert lib.geot_knn_grid_eligible(len(R.CLOUDS), R.NQ, R.NR - 1, k) == 0      # 2048 is the smallest reference count
        assert R.NQ % R.knn_plan(lib, len(R.CLOUDS), R.NQ, R.NR, k)["waves"] != 0
    for radius, ns in R.BALL_CASES:
        assert lib.geot_ball_grid_eligible(len(R.CLOUDS), R.NR, R.NQ, radius, ns) == 1
        assert lib.geot_ball_grid_eligible(len(R.CLOUDS), R.NR - 1, R.NQ, radius, ns) == 0
        assert R.NQ % R.ball_plan(lib, len(R.CLOUDS), R.NR, R.NQ, radius, ns)["waves"] != 0
    plan = R.knn_plan(lib, len(R.CLOUDS), R.NQ, R.NR, 16)
    ks = set(R.KNN_KS)
    # both ends of the select band from both sides, and the last list the grid takes
    assert {plan["kmin"] - 1, plan["kmin"], plan["kmax"], plan["kmax"] + 1, 64} <= ks
    assert lib.geot_knn_grid_eligible(len(R.CLOUDS), R.NQ, R.NR, 65) == 0


def test_clouds_and_queries_are_what_the_cases_say():
    ref, qry = R.inputs(R.NR)
    assert ref.shape == (len(R.CLOUDS), R.NR, 3) and qry.shape == (len(R.CLOUDS), R.NQ, 3) and ref.dtype == qry.dtype == F
    c = {name: ref[i] for i, name in enumerate(R.CLOUDS)}
    assert (c["identical"] == c["identical"][0]).all()
    assert np.isnan(c["naninf"][5]).all() and np.isinf(c["naninf"][9, 0]) and np.isfinite(np.delete(c["naninf"], [5, 9], 0)).all()
    assert tuple(c["outlier"][7]) == (50.0, -30.0, 10.0) and np.delete(c["outlier"], 7, 0).max() <= 0.01
    assert len(np.unique(c["dups"], axis=0)) <= R.NR // 2 and (c["line"][:, 1:] == 0).all() and (c["lattice"][:, 2] == 0).all()
    assert np.array_equal(c["lattice"][:, :2] * 64, np.round(c["lattice"][:, :2] * 64))
    for i in range(len(R.CLOUDS)):
        assert np.array_equal(qry[i, :150], ref[i, :150], equal_nan=True) and np.isnan(qry[i, -1]).all()
    far = qry[0, 150:180]
    assert ((far < 0) | (far > 1)).any(1).mean() > 0.8                    # N(0, 3^2): mostly outside the unit box


@pytest.mark.parametrize("radius,ns", R.BALL_CASES)
def test_ball_queries_hold_exact_radius_ties_and_points_outside_the_box(radius, ns):
    """d2 < r2 is strict: on the clouds with z = 0 the shifted queries are exactly radius away from their reference, in
    fp32, and every cloud has queries outside its box by less than the radius, on each of the six sides"""
    ref, _ = R.inputs(R.NR)
    qry = R.make_ball_queries(ref, radius)
    r2 = F(F(radius) * F(radius))
    for name in ("line", "lattice", "identical"):
        c = R.CLOUDS.index(name)
        ties = sum(int((R.sqdist(qry[c, j], ref[c]) == r2).any()) for j in range(120, 140))
        assert ties >= 5, (name, ties)
    for c, name in enumerate(R.CLOUDS):
        lo, hi = R.box(ref[c])
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            continue
        out = qry[c, 140:164]
        below, above = (lo[None] - out), (out - hi[None])
        assert ((below > 0).sum(0) >= 3).all() and ((above > 0).sum(0) >= 3).all(), name
        assert max(below.max(), above.max()) <= 0.9 * radius * 1.0001, name


# ---- the census -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nr,k", R.KNN_CASES)
def test_knn_census(lib, grid_env, nr, k):
    case = R.knn_case(lib, nr, k)
    keep = [~m for m in case["marginal"]]
    counts = R.census(case["fast"], keep)
    counts.update(R.census(case["ring"], keep))
    print(_table("kNN nr = %d, k = %d, G = %d: fast-path class" % (nr, k, case["plan"]["G"]), counts, R.FAST_CLASSES))
    print(_table("kNN nr = %d, k = %d: ring class of the queries the general loop answers" % (nr, k), counts, R.RING_CLASSES))
    marginal = sum(int(m.sum()) for m in case["marginal"])
    print("marginal: %d of %d" % (marginal, len(R.CLOUDS) * R.NQ))
    assert marginal <= R.MARGINAL_CAP * len(R.CLOUDS) * R.NQ
    for cell in R.KNN_INTENDED[nr, k]:
        assert counts.get(cell, 0) >= R.MIN_PER_CLASS, "k = %d: %s has %d queries" % (k, cell, counts.get(cell, 0))
    band = case["plan"]["kmin"] <= k <= case["plan"]["kmax"]
    assert (counts.get(("any", "rings_only"), 0) == 0) == band           # the band is the plan's, not a number written here
    if not band:
        assert counts["any", "rings_only"] == len(R.CLOUDS) * R.NQ - marginal
    # a query is answered by exactly one of the two stages
    for c in range(len(R.CLOUDS)):
        done = np.isin(case["fast"][c], ("direct", "bisect_found"))
        assert ((case["ring"][c] == "") == done).all()


@pytest.mark.parametrize("radius,ns", R.BALL_CASES)
def test_ball_census(lib, grid_env, radius, ns):
    case = R.ball_case(lib, R.NR, radius, ns)
    counts = R.census(case["cls"])
    print(_table("ball query radius = %g, nsample = %d" % (radius, ns), counts, R.BALL_CLASSES))
    for cell in R.BALL_INTENDED[radius, ns]:
        assert counts.get(cell, 0) >= R.MIN_PER_CLASS, "(%g, %d): %s has %d queries" % (radius, ns, cell, counts.get(cell, 0))
    if radius == 2.5:                                                    # every box but the outlier's fits in one cell
        assert all(g.dim == [1, 1, 1] for g, name in zip(case["grids"], R.CLOUDS) if name != "outlier")


def test_every_class_is_reached_by_some_case(lib, grid_env):
    """all the branches the two kernels have, over the whole GPU file (rmax1 excepted: see below)"""
    seen = set()
    for nr, k in R.KNN_CASES:
        seen |= {c for _, c in R.KNN_INTENDED[nr, k]}
    assert seen >= (set(R.FAST_CLASSES) | set(R.RING_CLASSES)) - {"rmax1", "zero_radius"}
    assert {c for v in R.BALL_INTENDED.values() for _, c in v} == set(R.BALL_CLASSES)


def test_rmax1_is_unreachable_from_the_public_entry_points(lib, grid_env):
    """The select fast path has a branch for a block that covers the grid (rmax <= 1: no certified radius, b2 = 3e38).
    It cannot run: the grid needs nr >= 2048 even when forced; in the band k <= kmax = 48 gives G >= 5 cells on the
    longest axis, so max(c, G - 1 - c) >= 2 for every cell; and a cloud without a finite positive extent (all points
    identical, an infinite coordinate) is ONE cell of nr >= 2048 records, more than the slots hold.  A fact, asserted over
    the eligible range -- should it stop holding, rmax1 needs inputs of its own."""
    rng = np.random.default_rng(0)
    sizes = [2048, 2049, 2050, 2100, 4096, 24000, 2 ** 20, 2 ** 31 - 1] + [int(v) for v in rng.integers(2048, 2 ** 24, 200)]
    assert lib.geot_knn_grid_eligible(1, 1, 2047, 8) == 0 and R.knn_plan(lib, 1, 1, 2047, 8) is None
    base = R.knn_plan(lib, 1, 1, 2048, 8)
    for nr in sizes:
        for k in range(base["kmin"], base["kmax"] + 1):
            plan = R.knn_plan(lib, 1, 1, nr, k)
            assert plan is not None and plan["G"] >= 5 and nr > 64 * plan["slots"], (nr, k, plan)
    for G in range(5, base["gmax"] + 1):
        assert min(max(c, G - 1 - c) for c in range(G)) >= 2
    # in the model: no query of any case is labelled rmax1, the longest axis has G cells wherever the box is a box, and
    # the clouds without one are a single cell
    for nr, k in R.KNN_CASES:
        case = R.knn_case(lib, nr, k)
        assert not any((f == "rmax1").any() for f in case["fast"])
        for g, name in zip(case["grids"], R.CLOUDS):
            assert (max(g.dim) == case["plan"]["G"]) if g.ok else (g.dim == [1, 1, 1] and g.start[-1] == nr), name
        assert [name for g, name in zip(case["grids"], R.CLOUDS) if not g.ok] == ["identical", "naninf"]


# ---- the model against grids that can be written down -----------------------------------------------------------------
def test_model_on_a_two_cubed_lattice():
    ref = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], F)          # index = x + 2 y + 4 z
    g = R.build_grid(ref, 2)
    assert g.ok and g.dim == [2, 2, 2] and g.h == F(0.5) and g.inv_h == F(2) and (g.lo == 0).all()
    assert np.array_equal(g.cells, ref.astype(np.int64))                 # coordinate 1 -> f = 2 -> clamped to dim - 1
    assert list(g.start) == list(range(9)) and list(g.rec) == list(range(8))
    e = (0, 0)
    assert R.row_ranges(g, (0, 0, 0)) == [e, e, e, e, (0, 2), (2, 4), e, (4, 6), (6, 8)]
    assert R.row_ranges(g, (1, 1, 1)) == [(0, 2), (2, 4), e, (4, 6), (6, 8), e, e, e, e]
    assert R.slot_count(R.row_ranges(g, (1, 0, 1))) == 4 and R.slot_count([(0, 64), (64, 129), (5, 5)]) == 3
    assert R.rmax_of(g, (0, 1, 0)) == 1
    assert R.face_bound(g, np.array([0.2, 0.2, 0.2], F), (0, 0, 0), 1) == np.inf                # the block covers the grid
    q = np.array([[0.5, 0.49999997, -3.0], [np.nan, 7.0, np.inf]], F)
    assert R.cells_of(g, q).tolist() == [[1, 0, 0], [0, 1, 1]]
    # a 4^3 grid over the unit box: the face two cells up, minus the h / 1000 slack; and the ball query's cell counts
    unit = np.array([[0, 0, 0], [1, 1, 1], [0.3, 0.3, 0.3]], F)
    g4 = R.build_grid(unit, 4)
    assert g4.dim == [4, 4, 4] and g4.h == F(0.25) and R.cells_of(g4, unit[2:]).tolist() == [[1, 1, 1]] and R.rmax_of(g4, (1, 1, 1)) == 2
    want = F(F(F(0.75) - F(0.3)) - F(F(0.25) * F(1e-3)))
    assert R.face_bound(g4, unit[2], (1, 1, 1), 1) == want and R.face_bound(g4, unit[2], (1, 1, 1), 2) == np.inf
    low = np.array([0.8, 0.8, 0.8], F)                                   # cell 3: only the faces below have cells behind
    assert R.face_bound(g4, low, (3, 3, 3), 1) == F(F(F(0.8) - F(0.5)) - F(F(0.25) * F(1e-3)))
    nanq = np.full(3, np.nan, F)
    assert R.face_bound(g4, nanq, (0, 0, 0), 1) == np.inf                # fminf drops the NaN operands
    for min_h, cells in ((0.3, 3), (2.0, 1), (0.01, 32), (1.0, 1), (0.5, 2)):
        gb = R.build_grid(unit, 1, min_h=F(min_h), gmax=32)
        assert gb.gtarget == cells and gb.dim == [cells] * 3 and gb.h == F(F(1) / F(cells))
        assert gb.h >= F(min_h) or cells == 1                           # one cell holds every hit whatever its edge
    assert R.sqdist(np.array([1, 2, 3], F), np.array([[0, 0, 0], [1, 2, 3]], F)).tolist() == [14.0, 0.0]
    assert R.morton_keys(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], F), 32).tolist() == [
        0, 0b001001001001001, 0b010010010010010, 0b100100100100100, 0b111111111111111]


@pytest.mark.parametrize("kind", ["identical", "inf"])
def test_model_on_clouds_without_a_box(kind):
    """mx == 0, or an infinite extent: ok == false, h = inf, inv_h = 0, one cell that holds everything"""
    ref = np.tile(np.array(R.SAME_POINT, F), (100, 1))
    if kind == "inf":
        ref = np.random.default_rng(0).random((100, 3)).astype(F)
        ref[9, 0] = np.inf
        ref[5] = np.nan
    g = R.build_grid(ref, 12)
    assert not g.ok and g.h == np.inf and g.inv_h == 0 and g.dim == [1, 1, 1]
    assert (g.cells == 0).all() and list(g.start) == [0, 100] and sorted(g.rec) == list(range(100))
    e = (0, 0)
    assert R.row_ranges(g, (0, 0, 0)) == [e, e, e, e, (0, 100), e, e, e, e] and R.rmax_of(g, (0, 0, 0)) == 0
    q = np.array([[5.0, -np.inf, np.nan]], F)
    assert R.cells_of(g, q).tolist() == [[0, 0, 0]]
    plan = dict(G=12, gmax=32, slots=12, kmin=8, kmax=48, waves=4, sort_max=1 << 22)
    fast, ring, marg, _ = R.classify_knn(ref, ref[:20], 8, plan)
    # 100 records fit the slots: only a cloud too small for the entry points gets here (query 5 of "inf" is the NaN point)
    assert (np.delete(fast, 5) == "rmax1").all() and fast[5] == ("nan_query" if kind == "inf" else "rmax1") and not marg.any()
    assert set(ring) <= {"", "r1_covered"}
    cls, gb = R.classify_ball(ref, ref[:20], 0.1, 4, dict(gmax=32, slots=12, waves=4))
    assert gb.dim == [1, 1, 1] and set(cls) <= {"direct", "bisect", "zero_hits", "short_fill"}
    assert R.morton_keys(ref, 32).tolist() == [0] * 100


def test_face_rounding_cloud_is_decided_by_the_slack_of_the_ring_stop(lib, grid_env):
    """The cloud of the GPU file's test_knn_ring_stop_keeps_its_slack: the nearest point p of the designed query lies
    OUTSIDE its 3-cell block, nearer than the block's face by more than the stop test's 0.99999 covers, and the only
    point inside the block, v, is farther than p yet within bound^2 * 0.99999 taken without the h / 1000 slack."""
    case = R.make_face_rounding_case()
    plan = R.knn_plan(lib, 1, 8, R.NR, R.FACE_K)
    assert plan["G"] == plan["gmax"] == 32 and not plan["kmin"] <= R.FACE_K <= plan["kmax"]
    ref, q = case["ref"][0], case["qry"][0, 0]
    g = R.build_grid(ref, plan["G"])
    cq = R.cells_of(g, case["qry"][0])[0]
    c = case["c"]
    assert g.dim == [32, 1, 1] and cq.tolist() == [c - 2, 0, 0] and g.cells[case["p_index"]].tolist() == [c, 0, 0]
    cheb = np.abs(g.cells - cq[None]).max(1)
    assert np.flatnonzero(cheb <= 1).tolist() == [case["v_index"]]                  # the block holds v and nothing else
    d = R.sqdist(q, ref)
    order = np.argsort(d, kind="stable")
    assert order[:2].tolist() == [case["p_index"], case["v_index"]] and d[order[0]] < d[order[1]]
    assert d[case["p_index"]] == case["d2p"] and d[case["v_index"]] == case["d2v"]
    bound = R.face_bound(g, q, cq, 1)                                               # with the slack, as the kernel has it
    thr = F(F(bound * bound) * F(0.99999))
    assert thr == case["thr"] and not case["d2v"] < thr                             # ring 1 does not stop: ring 2 finds p
    assert case["d2p"] < case["d2v"] <= case["thr_mut"]                             # without the slack it would have
    assert float(ref[case["p_index"], 0]) < float(F(g.lo[0] + F(F(c) * g.h)))      # p sits below the face of its own cell
    fast, ring, marg, _ = R.classify_knn(ref, case["qry"][0], R.FACE_K, plan)
    assert fast[0] == "rings_only" and ring[0] == "r2_3_bound" and not marg[0]
