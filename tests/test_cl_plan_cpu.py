"""The launch geometry of the point-major FP stage kernels (csrc/channels_last.hip), without a GPU.

* the row deal of fp_front_cl as tests/_cl_ref.py restates it: over a dense grid and random (R, T, granule), every row of
  [0, R) is dealt exactly once, a workgroup's rows ascend with its slot i (the kernel stops a stage at the first slot past
  its range: "the valid ones are a prefix"), and there are 8 ranges exactly when T is a multiple of 8
* what the size queries refuse, and that GEOT_CL_TILES pins both of them (capped at ceil(rows / 16))
* the census of tests/test_cl_kernels_gpu.py's case tables: every class its docstring names occurs, so that a later edit of
  a shape cannot silently lose one
"""
import numpy as np
import pytest

import _cl_ref as R

GRANULES = (None, 1, 0, 7, 128, 10000)          # None: unset -> 8; 0: one contiguous run per workgroup


@pytest.fixture(scope="module")
def lib():
    from geot_amd import _lib
    return _lib.load()


@pytest.fixture()
def tiles_env(monkeypatch):
    monkeypatch.delenv("GEOT_CL_TILES_MULT", raising=False)
    monkeypatch.delenv("GEOT_CL_TILES", raising=False)
    return monkeypatch


def _deal_violations(rows, T, setting):
    g = R.granule_of(setting, rows, T)
    r, ok = R.deal_table(rows, T, g)
    bad = []
    times = np.bincount(r[ok], minlength=rows)
    if times.size != rows or not (times == 1).all():
        bad.append("rows dealt %s times" % sorted(set(times.tolist())))
    if r.shape[1] > 1 and not (np.diff(r, axis=1) > 0).all():
        bad.append("a workgroup's rows do not ascend with i")
    if not (ok[:, :-1] >= ok[:, 1:]).all():
        bad.append("the valid slots are not a prefix")
    nx = R.cl_deal(rows, T, g, 0)["nx"]
    if (nx == 8) != (T >= 8 and T % 8 == 0) or nx not in (1, 8):
        bad.append("nx = %d" % nx)
    return bad


def test_row_deal_partitions_the_rows_dense_grid():
    for T in range(1, 33):
        for rows in range(1, 601):
            for setting in GRANULES:
                bad = _deal_violations(rows, T, setting)
                assert not bad, (rows, T, setting, bad)


def test_row_deal_partitions_the_rows_random():
    rng = np.random.default_rng(11)
    for _ in range(400):
        rows = int(rng.integers(1, 8000))
        T = int(rng.choice([rng.integers(1, 64), 8 * rng.integers(1, 33), rng.integers(1, 300)]))
        T = max(1, min(T, (rows + 15) // 16))
        setting = [None, 0, int(rng.integers(1, 300)), int(rng.integers(1, 50000))][int(rng.integers(0, 4))]
        bad = _deal_violations(rows, T, setting)
        assert not bad, (rows, T, setting, bad)


def test_the_stage_loop_takes_exactly_the_dealt_rows():
    """deal_rows (the kernel's loop: stages of 128 slots, out at the first stage that is not full) against the table"""
    for rows, T, setting in [(303, 5, None), (303, 5, 128), (303, 5, 10000), (1027, 8, None), (2055, 8, None), (1200, 24, None),
                             (256, 1, None), (128, 1, 0), (1, 1, None), (600, 16, 7)]:
        g = R.granule_of(setting, rows, T)
        r, ok = R.deal_table(rows, T, g)
        for blk in range(T):
            assert np.array_equal(R.deal_rows(rows, T, g, blk), r[blk][ok[blk]]), (rows, T, setting, blk)
            st = R.stage_counts(int(ok[blk].sum()))
            assert all(v == R.CL_STAGE for v in st[:-1]) and 0 <= st[-1] < R.CL_STAGE


def test_size_queries_refuse_what_the_kernels_do_not_cover(lib, tiles_env):
    for c in (1, 2, 3, 6, 258, 4098):                                          # C % 4, C < 4
        assert lib.geot_cl_tiles(1, 100, c) == -1, c
        assert lib.geot_fp_front_cl_tiles(1, c, 100, 0) == -1, c
    assert lib.geot_cl_tiles(1, 100, 0) == -1 and lib.geot_cl_tiles(1, 100, -4) == -1
    assert lib.geot_cl_tiles(1, 100, 4100) == -1 and lib.geot_fp_front_cl_tiles(1, 4100, 100, 0) == -1      # C > 4096
    assert lib.geot_cl_tiles(1, 100, 4096) >= 1 and lib.geot_cl_tiles(1, 100, 4) >= 1
    assert lib.geot_cl_tiles(0, 100, 64) == -1 and lib.geot_cl_tiles(-1, 100, 64) == -1               # batches < 1
    assert lib.geot_cl_tiles(1, 0, 64) == -1 and lib.geot_cl_tiles(1, -5, 64) == -1
    assert lib.geot_cl_tiles(1, 2 ** 31, 64) == -1 and lib.geot_cl_tiles(2, 2 ** 30, 64) == -1        # rows > 2^31 - 1
    assert lib.geot_cl_tiles(1, 2 ** 31 - 1, 64) >= 1
    assert lib.geot_fp_front_cl_tiles(1, 64, 100, -1) == -1 and lib.geot_fp_front_cl_tiles(1, 64, 100, 9) == -1
    assert all(lib.geot_fp_front_cl_tiles(1, 64, 100, cs) >= 1 for cs in range(9))
    assert lib.geot_fp_front_cl_tiles(0, 64, 100, 0) == -1 and lib.geot_fp_front_cl_tiles(1, 64, 0, 0) == -1
    assert lib.geot_fp_front_cl_tiles(2, 64, 2 ** 29, 0) == -1                                       # b n > 2^30 - 1
    assert lib.geot_fp_front_cl_tiles(1, 64, 2 ** 30, 0) == -1
    assert lib.geot_fp_front_cl_tiles(1, 64, 2 ** 30 - 1, 0) >= 1
    assert lib.geot_cl_stat_floats(-1, 4) == -1 and lib.geot_cl_stat_floats(4, -1) == -1
    assert lib.geot_cl_stat_floats(0, 4) == 0 and lib.geot_cl_stat_floats(7, 260) == 7 * (3 * 260 + 1)


def test_the_tiles_knob_pins_both_queries(lib, tiles_env):
    base = [(lib.geot_cl_tiles(b, n, c), lib.geot_fp_front_cl_tiles(b, c, n, cs))
            for b, n, c, cs in ((2, 150, 260, 3), (8, 24000, 1536, 5), (1, 5, 4, 0))]
    for T in (1, 5, 8, 24, 64, 100000):
        tiles_env.setenv("GEOT_CL_TILES", str(T))
        for b, n, c, cs in ((2, 150, 260, 3), (3, 101, 4096, 8), (1, 1, 4, 0), (1, 16, 64, 1), (1, 17, 64, 0), (25, 41, 68, 2),
                            (8, 24000, 1536, 5)):
            want = max(1, min(T, (b * n + 15) // 16))
            assert lib.geot_cl_tiles(b, n, c) == want == R.cl_tiles_for(b * n, c, T), (T, b, n, c)
            assert lib.geot_cl_tiles(1, b * n, c) == want
            assert lib.geot_fp_front_cl_tiles(b, c, n, cs) == want, (T, b, n, c, cs)
        assert lib.geot_cl_tiles(1, 100, 6) == -1 and lib.geot_fp_front_cl_tiles(1, 64, 100, 9) == -1     # still refused
    tiles_env.setenv("GEOT_CL_TILES", "4")                                    # the multiplier still applies, then the cap
    tiles_env.setenv("GEOT_CL_TILES_MULT", "3")
    assert lib.geot_cl_tiles(1, 1000, 64) == 12 and lib.geot_fp_front_cl_tiles(1, 64, 1000, 2) == 12
    assert lib.geot_cl_tiles(1, 100, 64) == 7
    tiles_env.delenv("GEOT_CL_TILES_MULT")
    for junk in ("0", "-3", "", "x"):                                         # not a positive count: as if unset
        tiles_env.setenv("GEOT_CL_TILES", junk)
        assert [(lib.geot_cl_tiles(b, n, c), lib.geot_fp_front_cl_tiles(b, c, n, cs))
                for b, n, c, cs in ((2, 150, 260, 3), (8, 24000, 1536, 5), (1, 5, 4, 0))] == base, junk


# ---- census of the GPU suite's case tables ---------------------------------------------------------------------------
def test_census_fp_front_cases():
    seen_wg, seen_rows, names = set(), set(), set()
    for case in R.FP_FRONT_CASES:
        assert case["name"] not in names
        names.add(case["name"])
        b, n, c, T = case["b"], case["n"], case["c"], case["T"]
        assert T == R.cl_tiles_for(b * n, c, T), "%s: T is capped" % case["name"]
        assert b * n * c * 4 < 16 << 20 and (c < 4096 or b * n <= 303)
        wg, rows = R.fp_front_classes(b, n, T, case["granule"])
        for s in wg:
            seen_wg |= s
        seen_rows |= set(rows.tolist())
        counts = [len(r) for r in R.fp_front_rows(b, n, T, case["granule"])]
        assert sum(counts) == b * n
        if case["name"] in R.FP_FRONT_COUNTS:
            assert counts == R.FP_FRONT_COUNTS[case["name"]], case["name"]
    assert set(R.FP_FRONT_COUNTS) <= names
    assert seen_wg == set(R.FP_FRONT_WG_CLASSES), (seen_wg ^ set(R.FP_FRONT_WG_CLASSES))
    for nx in (1, 8):
        for st in (0, 1, 2):
            assert any(s.startswith("nx%d stage %d" % (nx, st)) for s in seen_rows), (nx, st)
    assert any(s.endswith("odd last row") for s in seen_rows) and any(s.endswith("partial group") for s in seen_rows)
    # the axes the issue of this suite lists
    assert {case["c"] // 4 for case in R.FP_FRONT_CASES} >= {1, 63, 64, 65, 1024}
    assert {R.cl_block(case["c"] // 4) for case in R.FP_FRONT_CASES} >= {64, 128, 1024}
    assert {case["cs"] for case in R.FP_FRONT_CASES} == set(range(9))
    assert {case["m"] for case in R.FP_FRONT_CASES} >= {1, 3, 50}
    assert {case["T"] for case in R.FP_FRONT_CASES} >= {1, 5, 8, 12, 16, 24}
    assert {case["granule"] for case in R.FP_FRONT_CASES} >= {None, 1, 0, 128, 10000}
    assert {case["b"] * case["n"] for case in R.FP_FRONT_CASES if case["T"] == 1} >= {1, 2, 3, 5, 6, 7, 130, 131}
    assert {case["ordered"] for case in R.FP_FRONT_CASES} == {False, True}


def test_census_reduce_and_apply_cases():
    for table in (R.REDUCE_CASES, R.SKIP_REDUCE_CASES):
        seen = set()
        for case in table:
            rows = case["b"] * case["n"]
            assert rows * case["c"] * 4 < 16 << 20 and (case["c"] < 4096 or rows <= 303)
            seen |= R.reduce_classes(case)
        assert seen >= set(R.REDUCE_CLASSES), set(R.REDUCE_CLASSES) - seen
        assert {case["c"] for case in table} >= set(R.WIDTHS)
    assert {case["cs"] for case in R.SKIP_REDUCE_CASES} == set(range(9))
    tiles, per = R.cl_launch_dims(1025, 68, 64)
    assert (tiles, per) == (64, 17) and sum(r0 == r1 for r0, r1 in R.tile_ranges(1025, tiles, per)) == 3
    assert R.cl_launch_dims(17, 68, 8) == (2, 9) and R.cl_launch_dims(16, 68, 8) == (1, 16) and R.cl_launch_dims(1, 68, 8) == (1, 1)


def test_census_sums_wgrad_and_node_cases():
    # bn_sums_cl: 16 parts, 4 tiles in flight per part -- the unrolled loop runs from 49 tiles on, its tail below and beside it
    assert {t < 16 for t in R.SUMS_TILES} == {True, False} and {t >= 49 for t in R.SUMS_TILES} == {True, False}
    assert any(t % 64 for t in R.SUMS_TILES if t > 64) and 64 in R.SUMS_TILES and 65 in R.SUMS_TILES
    assert {c % 64 == 0 for c in R.SUMS_C} == {True, False} and max(R.SUMS_C) > 64 and min(R.SUMS_K) == 2 and max(R.SUMS_K) == R.CL_MAX_SUMS
    assert {c * cs < 256 for c, cs in R.WGRAD_CASES} == {True, False} and any(c * cs == 256 for c, cs in R.WGRAD_CASES)
    assert {cs for _, cs in R.WGRAD_CASES} == set(range(1, 9))
    for key, want in (("n", {33, 257}), ("m", {3, 17}), ("c", {252, 260}), ("cs", {0, 1, 8}), ("relu", {True, False}),
                      ("training", {True, False}), ("ordered", {True, False}), ("kind", {"nn", "hub", "one"})):
        assert {case[key] for case in R.NODE_CASES} == want, key
