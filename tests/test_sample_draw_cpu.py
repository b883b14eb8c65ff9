"""The contract of geot_sample_draw (include/geot_hip.h) itself, on tests/_sample_draw_ref.py -- no GPU: the Philox known
answers, the bijection (every row without replacement is m distinct values of [0, n)) and the uniformity of what it draws.

Uniformity: seed 0x1234567 and draws 0 .. D-1 are fixed here and were not tuned.  Every chi-square statistic must stay below
dof + 4 sqrt(2 dof) (four standard deviations of the chi-square law above its mean); np.random.choice itself, under seeds
0, 1, 2, gave 195-235 (triples), 982-1029 (inclusion), 958-1088 (positions) and 976-1066 (differences) on these shapes.
"""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sample_draw_ref as sd  # noqa: E402

SEED = 0x1234567


def bound(dof):
    return dof + 4.0 * np.sqrt(2.0 * dof)


def chi2(counts, expected):
    counts = np.asarray(counts, dtype=np.float64)
    return float(((counts - expected) ** 2 / expected).sum())


@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    got = tuple(int(w) for w in sd.philox4x32(*ctr, *key))
    assert got == want, [hex(w) for w in got]


def test_feistel_is_a_bijection_at_every_width():
    for b in (10, 11, 16, 17):
        for d in (0, 5, 2 ** 32 + 1):
            image = sd.feistel(np.arange(1 << b), d, b, SEED)
            assert np.array_equal(np.sort(image), np.arange(1 << b, dtype=np.uint64)), (b, d)


def test_tabulated_round_function_gives_the_same_rows():
    """The restatement looks the round function up per draw where that is cheaper (small scans): no other values."""
    for n, m in ((7, 3), (30, 30), (1000, 200), (1025, 700)):
        draws = np.array([0, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1], dtype=np.uint64)
        direct = sd._without_replacement(n, m, SEED, draws, tabled=False)
        assert np.array_equal(direct, sd._without_replacement(n, m, SEED, draws, tabled=True)), (n, m)
        assert np.array_equal(direct, sd.draw_rows(n, m, SEED, draws))
        for row, d in zip(direct, draws):                # and the definition, element by element
            for j in (0, m - 1):
                x = sd.feistel(j, d, sd.width(n), SEED)
                while x >= n:
                    x = sd.feistel(x, d, sd.width(n), SEED)
                assert int(x) == row[j]


@pytest.mark.parametrize("n, m", [(1, 1), (5, 5), (7, 3), (512, 511), (513, 200), (1000, 200), (1025, 1025), (65537, 3000),
                                  (200003, 24000)])
def test_rows_without_replacement_are_distinct_and_in_range(n, m):
    rows = sd.draw_rows(n, m, SEED, np.arange(4))
    assert rows.shape == (4, m) and rows.dtype == np.int64
    assert rows.min() >= 0 and rows.max() < n
    for row in rows:
        assert np.unique(row).size == m
    if n >= 512:
        assert not np.array_equal(rows[0], rows[1])


def test_ordered_triples_of_seven_are_uniform():
    d = 42000
    rows = sd.draw_rows(7, 3, SEED, np.arange(d))
    code = rows[:, 0] * 49 + rows[:, 1] * 7 + rows[:, 2]
    triples = [a * 49 + b * 7 + c for a, b, c in itertools.permutations(range(7), 3)]
    assert len(triples) == 210 and np.isin(code, triples).all()
    stat = chi2([(code == t).sum() for t in triples], d / 210.0)
    print("triples: chi2 %.1f, bound %.1f" % (stat, bound(209)))
    assert stat < bound(209)


def test_permutations_of_five_are_uniform_and_all_occur():
    d = 24000
    rows = sd.draw_rows(5, 5, SEED, np.arange(d))
    code = (rows * 5 ** np.arange(5)).sum(1)
    perms = [sum(v * 5 ** i for i, v in enumerate(p)) for p in itertools.permutations(range(5))]
    assert np.isin(code, perms).all()
    counts = np.array([(code == p).sum() for p in perms])
    assert (counts > 0).all()
    stat = chi2(counts, d / 120.0)
    print("permutations of 5: chi2 %.1f, bound %.1f" % (stat, bound(119)))
    assert stat < bound(119)


@pytest.fixture(scope="module")
def thousand():
    return sd.draw_rows(1000, 200, SEED, np.arange(2000))


def test_inclusion_counts_are_uniform(thousand):
    n, m, d = 1000, 200, 2000
    p = m / n
    counts = np.bincount(thousand.reshape(-1), minlength=n).astype(np.float64)
    stat = float(((counts - d * p) ** 2 / (d * p * (1 - p))).sum())
    print("inclusion: chi2 %.1f, bound %.1f" % (stat, bound(999)))
    assert stat < bound(999)


@pytest.mark.parametrize("position", [0, 199])
def test_first_and_last_position_are_uniform(thousand, position):
    stat = chi2(np.bincount(thousand[:, position], minlength=1000), 2000 / 1000.0)
    print("position %d: chi2 %.1f, bound %.1f" % (position, stat, bound(999)))
    assert stat < bound(999)


def test_neighbour_differences_are_uniform(thousand):
    diff = (thousand[:, 1:] - thousand[:, :-1]) % 1000
    assert diff.min() >= 1
    counts = np.bincount(diff.reshape(-1), minlength=1000)[1:]
    stat = chi2(counts, diff.size / 999.0)
    print("differences: chi2 %.1f, bound %.1f" % (stat, bound(998)))
    assert stat < bound(998)


def test_with_replacement_values_are_uniform():
    rows = sd.draw_rows(5, 4000, SEED, np.arange(50))
    assert rows.shape == (50, 4000) and rows.min() >= 0 and rows.max() < 5
    stat = chi2(np.bincount(rows.reshape(-1), minlength=5), rows.size / 5.0)
    print("with replacement: chi2 %.1f, bound %.1f" % (stat, bound(4)))
    assert stat < bound(4)


@pytest.mark.parametrize("n, m", [(1000, 200), (5, 40)])
def test_two_seeds_give_different_rows(n, m):
    a, b = sd.draw_rows(n, m, SEED, [0, 1]), sd.draw_rows(n, m, SEED + 1, [0, 1])
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])
    hi = sd.draw_rows(n, m, SEED + (1 << 32), [0])           # the high key word counts too
    assert not np.array_equal(a[0], hi[0])


@pytest.mark.parametrize("base", [0, 7, 2 ** 32 - 2, 2 ** 64 - 2])
def test_draw_d_of_base_zero_is_slot_zero_of_base_d(base):
    sizes = [1000, 5, 1000, 0, 300]
    sel, bad = sd.sample_draw_ref(sizes, 200, SEED, base)
    assert list(bad) == [0, 0, 0, 2, 0] and not sel[3].any()
    for i, n in enumerate(sizes):
        if n:
            one, flag = sd.sample_draw_ref([n], 200, SEED, (base + i) % 2 ** 64)
            assert np.array_equal(one[0], sel[i]) and flag[0] == 0
            assert np.array_equal(sd.draw_rows(n, 200, SEED, [(base + i) % 2 ** 64])[0], sel[i])


# ------------------------------------------------------------------------------------------------ the boundary, without a GPU
def test_argument_errors_are_returned_before_any_launch():
    """No GPU here: a call that returns hipErrorInvalidValue has not launched (a launch would fail otherwise)."""
    from geot_amd import _lib
    lib = _lib.load()
    good = [4, 16, 3, 100, 0x1000, None, SEED, 0, 0x2000, 0x3000]        # (the pointers are never dereferenced on the host)
    for at, value in ((0, 0), (0, -1), (0, 65536), (1, 0), (1, -3), (2, 0), (3, 0), (4, None), (8, None), (9, None)):
        args = list(good)
        args[at] = value
        assert lib.geot_sample_draw(*args, None) == 1, (at, value)


def test_device_draws_counter_and_exports():
    import geot_amd.openpoints.dataset as ds
    assert callable(ds.sample_draw)
    d = ds.DeviceDraws(SEED)
    assert (d.take(7), d.take(0), d.take(16), d.counter) == (0, 7, 7, 23)
    other = ds.DeviceDraws(1)
    other.set_state(d.state())
    assert other.state() == {"seed": SEED, "counter": 23} and other.take(1) == 23
    wrap = ds.DeviceDraws(2 ** 64 + 5, 2 ** 64 - 1)                       # both are 64-bit values
    assert wrap.seed == 5 and wrap.take(2) == 2 ** 64 - 1 and wrap.counter == 1
    with pytest.raises(RuntimeError):
        d.take(-1)
    import inspect
    for cls in (ds.FixMatchBatcher, ds.SupervisedBatcher, ds.ValBatcher):
        assert inspect.signature(cls.__init__).parameters["draws"].default is None
        assert inspect.signature(cls.batch).parameters["draws"].default is None
    import torch
    with pytest.raises(RuntimeError, match="DeviceScanSet"):
        ds.sample_draw(torch.zeros(8, 3), None, 4, 0, 0)
