"""The contract of geot_view_draw (include/geot_hip.h) itself, on tests/_view_draw_ref.py -- no GPU: the error of the two
approximations the normals are made of (measured against numpy float64 over ALL 2^24 inputs each), the exact values the
rotation relies on, the counter words, the distributions of everything drawn, and the host side of the boundary (the plan
and template checks of the entry point, DeviceDraws' flag).  tests/test_view_draw_gpu.py shows that the kernel equals the
restatement bit for bit, so what is measured here is what the kernel draws.

Error bound: a normal z = r cos / r sin must be within 2^-24 / 0.01 of the exact one -- one ulp of a unit-scale coordinate at
the largest default sigma (0.01).  |cos| <= 1 and r <= sqrt(2 ln 2^24) = 5.7682, so the radius may be off by the bound and
cos / sin by the bound over 5.7682.

Distributions: the seed and the draw ids are fixed here and were not tuned.  Every statistic is gated at the 1 - 1e-6
quantile of its law: chi-square with the stated degrees of freedom (Q below, from the chi-square quantile function); the
moment statistics are squares of asymptotically standard normal values, chi-square with 1 degree."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sample_draw_ref as sd  # noqa: E402
import _view_draw_ref as vr  # noqa: E402

F = np.float32
SEED = 0x5EEDC0DE1234567
N24 = 1 << 24
BOUND = 2.0 ** -24 / 0.01
Q = {1: 23.92812697687947, 3: 30.66484970615427, 5: 35.88818687961042, 65: 134.2020789688319, 255: 377.0781154988172}


def chi2(counts, expected):
    counts, expected = np.asarray(counts, dtype=np.float64), np.asarray(expected, dtype=np.float64)
    return float(((counts - expected) ** 2 / expected).sum())


# ---------------------------------------------------------------------------------------------------- the approximations
@pytest.fixture(scope="module")
def radii():
    return vr.radius(np.arange(N24, dtype=np.uint64) << np.uint64(8))


def test_radius_error_over_all_inputs(radii):
    k = np.arange(N24, dtype=np.float64)
    exact = np.sqrt(-2.0 * np.log((k + 1.0) / N24))
    err = float(np.abs(radii.astype(np.float64) - exact).max())
    print("radius: max abs error %.3g, bound %.3g; largest radius %.7g" % (err, BOUND, radii.max()))
    assert err <= BOUND
    assert radii.dtype == F and radii[-1] == 0 and not np.signbit(radii[-1]) and radii[0] == radii.max() < 5.7683
    assert np.isfinite(radii).all() and (np.diff(radii.astype(np.float64)) <= 1e-6).all()      # never rising by more than noise


def test_sincos_error_over_all_fractions(radii):
    k = np.arange(N24, dtype=np.float64)
    c, s = vr.sincos_turns((np.arange(N24, dtype=np.uint64)).astype(F) * F(2.0 ** -24))
    ang = 2.0 * np.pi * k / N24
    err = max(float(np.abs(c.astype(np.float64) - np.cos(ang)).max()), float(np.abs(s.astype(np.float64) - np.sin(ang)).max()))
    print("sincos: max abs error %.3g, times the largest radius %.3g, bound %.3g" % (err, err * float(radii.max()), BOUND))
    assert err * float(radii.max()) <= BOUND
    assert c.dtype == s.dtype == F and np.abs(c).max() <= 1 and np.abs(s).max() <= 1


def test_sincos_of_negative_and_whole_turns():
    """The rotation's range: t in [-angle / 2, angle / 2] turns with |angle| up to 1024, against float64."""
    rng = np.random.default_rng(7)
    t = np.concatenate([rng.uniform(-2, 2, 200000), rng.uniform(-512, 512, 200000), [-0.5, 0.5, -0.25, 0.75, 1.0, -3.0]]).astype(F)
    c, s = vr.sincos_turns(t)
    ang = 2.0 * np.pi * t.astype(np.float64)
    err = max(float(np.abs(c - np.cos(ang)).max()), float(np.abs(s - np.sin(ang)).max()))
    print("sincos on [-512, 512] turns: max abs error %.3g" % err)
    assert err <= BOUND / 5.7683


def test_exact_values_the_rotation_relies_on():
    for t, want in ((0.0, (1, 0)), (0.25, (0, 1)), (0.5, (-1, 0)), (0.75, (0, -1)), (-0.25, (0, -1)), (1.0, (1, 0)), (-2.0, (1, 0))):
        c, s = vr.sincos_turns(F(t))
        assert (float(c), float(s)) == want, (t, c, s)
    c, s = vr.sincos_turns(F(0))
    assert not np.signbit(c) and not np.signbit(s) and c.view(np.uint32) == 0x3F800000 and s.view(np.uint32) == 0
    for d in range(64):                                   # an angle bound of 0: R is the identity, bit for bit, in every order
        R, order = vr.rotation(np.zeros(3, F), 2, 3, SEED, d)
        assert np.array_equal(R.view(np.uint32), np.eye(3, dtype=F).view(np.uint32)), (d, order)
    R, _ = vr.rotation(np.array([1, 0.5, 0.25], F), 2, 3, SEED, 1)
    assert np.abs(R.astype(np.float64) @ R.astype(np.float64).T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R.astype(np.float64)) - 1) < 1e-6


def test_rotation_equals_the_reference_statement_in_float64():
    """R = A B C of axis rotations by angle pi (2u - 1) in the drawn order -- the class's own statement, in float64."""
    bound = np.array([1, 0.5, 0.25], F)
    for d in range(32):
        R, order = vr.rotation(bound, 0, 2, SEED, d)
        w = vr.words(0, 0, 2, vr.Q_ROTATE, SEED, d)
        mats = []
        for ax in range(3):
            th = float(bound[ax]) * np.pi * (2.0 * float(vr.uniform(w[ax])) - 1.0)
            c, s = math.cos(th), math.sin(th)
            mats.append({0: np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), 1: np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
                         2: np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[ax])
        assert np.abs(R - mats[order[0]] @ mats[order[1]] @ mats[order[2]]).max() < 1e-6


def test_tag_never_equals_a_counter_word_of_sample_draw():
    taken = set(range(8)) | {0xFFFFFFFF}
    tags = [vr.tag(v, p, q) for v in range(3) for p in (0, 1, 15, 255, 4095) for q in range(8)]
    assert len(set(tags)) == len(tags) and not (set(tags) & taken)
    assert all(t >> 30 == 1 for t in tags)                 # bit 30 set, bit 31 clear: structurally none of 0..7, 0xFFFFFFFF
    # and the words differ: the slot's vertex sample (second word 0..7, 0xFFFFFFFF) shares the draw id with its views
    mine = vr.words(0, 0, 0, 0, SEED, 5)
    for c1 in sorted(taken):
        theirs = sd.philox4x32(0, c1, 5, 0, SEED & 0xFFFFFFFF, SEED >> 32)
        assert [int(a) for a in mine] != [int(b) for b in theirs]


# ---------------------------------------------------------------------------------------------------- the distributions
@pytest.fixture(scope="module")
def normals():
    return vr.normals3(*vr.words(np.arange(1 << 17), 0, 3, vr.Q_NOISE, SEED, 11)).astype(np.float64).reshape(-1)


def test_moments_of_the_normals(normals):
    z, n = normals, normals.size
    mean, var = z.mean(), z.var()
    skew, kurt = ((z - mean) ** 3).mean() / var ** 1.5, ((z - mean) ** 4).mean() / var ** 2
    stats = {"mean": n * mean ** 2, "variance": (n * (z ** 2).mean() - n) ** 2 / (2.0 * n), "skewness": n / 6.0 * skew ** 2,
             "kurtosis": n / 24.0 * (kurt - 3.0) ** 2}
    print("normals (n = %d): mean %.3e var %.6f skew %.3e kurt %.5f; statistics %s, bound %.2f"
          % (n, mean, var, skew, kurt, {k: round(v, 2) for k, v in stats.items()}, Q[1]))
    assert all(v < Q[1] for v in stats.values()), stats


def test_normals_fill_their_bins(normals):
    edges = np.linspace(-4, 4, 65)
    cdf = np.array([0.5 * (1 + math.erf(e / math.sqrt(2))) for e in edges])
    prob = np.concatenate([[cdf[0]], np.diff(cdf), [1 - cdf[-1]]])
    counts = np.bincount(np.searchsorted(edges, normals), minlength=66)
    stat = chi2(counts, prob * normals.size)
    print("normals over 66 bins: chi2 %.1f, bound %.1f" % (stat, Q[65]))
    assert stat < Q[65]
    # the three components of a point are uncorrelated
    z = normals.reshape(-1, 3)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert z.shape[0] * np.corrcoef(z[:, a], z[:, b])[0, 1] ** 2 < Q[1]


def test_uniforms_fill_their_bins():
    draws = np.arange(200000, dtype=np.uint64)
    for q, word in ((vr.Q_SCALE, 0), (vr.Q_SCALE, 2), (vr.Q_SHIFT, 1), (vr.Q_ROTATE, 0)):
        u = vr.uniform(vr.words(0, 2, 1, q, SEED, draws)[word])
        assert u.min() >= 0 and u.max() < 1
        stat = chi2(np.bincount((u * F(256)).astype(np.int64), minlength=256), draws.size / 256.0)
        print("uniform (quantity %d word %d): chi2 %.1f, bound %.1f" % (q, word, stat, Q[255]))
        assert stat < Q[255]


class _Step:
    color_drop, aug_prob, horz_axes = 0.2, 0.95, (0, 1)


def test_masks_and_drops_hit_their_probability():
    m = 400000
    keep = vr.point_mask(_Step, m, 0, 4, SEED, 3)
    p = float(F(_Step.color_drop))
    p_keep = 1.0 - math.ceil(p * N24) / N24 - 1.0 / N24 + (1.0 / N24 if p * N24 != math.ceil(p * N24) else 0)   # u > p, u = k 2^-24
    stat = chi2([keep.sum(), m - keep.sum()], [m * p_keep, m * (1 - p_keep)])
    print("per-point mask: kept %.5f of %d, chi2 %.2f, bound %.2f" % (keep.mean(), m, stat, Q[1]))
    assert set(np.unique(keep)) == {0.0, 1.0} and stat < Q[1]
    d = np.arange(200000, dtype=np.uint64)
    drops = vr.uniform(vr.words(0, 0, 4, vr.Q_DROP, SEED, d)[0]) < F(_Step.color_drop)
    stat = chi2([drops.sum(), d.size - drops.sum()], [d.size * p, d.size * (1 - p)])
    print("drop: %.5f of %d, chi2 %.2f, bound %.2f" % (drops.mean(), d.size, stat, Q[1]))
    assert stat < Q[1]
    assert all(vr.drop(_Step, 0, 4, SEED, int(i)) == bool(drops[i]) for i in range(50))


def test_flips_and_rotation_orders_are_uniform():
    n = 6000
    sets = [tuple(vr.flips(_Step, 1, 2, SEED, d)) for d in range(n)]
    p = float(F(_Step.aug_prob))
    counts = [sets.count(()), sets.count((0,)), sets.count((1,)), sets.count((0, 1))]
    stat = chi2(counts, [n * (1 - 0.75 * p), n * p / 4, n * p / 4, n * p / 4])
    print("flips: %s, chi2 %.2f, bound %.2f" % (counts, stat, Q[3]))
    assert stat < Q[3]
    orders = [vr.rotation(np.zeros(3, F), 1, 2, SEED, d)[1] for d in range(n)]
    counts = [orders.count(o) for o in vr.ORDERS]
    stat = chi2(counts, n / 6.0)
    print("rotation orders: %s, chi2 %.2f, bound %.2f" % (counts, stat, Q[5]))
    assert stat < Q[5]


def test_views_positions_seeds_and_draw_ids_give_other_values():
    base = vr.noise_rows(64, 0, 3, SEED, 9, 0.01, 0.05)
    for other in (vr.noise_rows(64, 1, 3, SEED, 9, 0.01, 0.05), vr.noise_rows(64, 0, 4, SEED, 9, 0.01, 0.05),
                  vr.noise_rows(64, 0, 3, SEED + 1, 9, 0.01, 0.05), vr.noise_rows(64, 0, 3, SEED + (1 << 32), 9, 0.01, 0.05),
                  vr.noise_rows(64, 0, 3, SEED, 10, 0.01, 0.05), vr.noise_rows(64, 0, 3, SEED, 9 + (1 << 32), 0.01, 0.05)):
        assert not np.array_equal(base, other)
    assert np.array_equal(base, vr.noise_rows(64, 0, 3, SEED, 9 + (1 << 64), 0.01, 0.05))      # a draw id is mod 2^64
    assert np.array_equal(base[:16], vr.noise_rows(16, 0, 3, SEED, 9, 0.01, 0.05))             # a point does not depend on m
    assert np.abs(vr.noise_rows(4096, 0, 3, SEED, 9, 0.01, 0.005)).max() == F(0.005)           # the clamp


# ---------------------------------------------------------------------------------------------------- the host side
ALL = ["PointsToTensor", "PointCloudJitter_s", "ChromaticPerDropGPU", "RandomHorizontalFlip", "ChromaticDropGPU",
       "PointCloudScaleAndJitter", "PointCloudRotation", "ChromaticPerDropGPU", "PointCloudTranslation",
       "PointCloudScaleAndTranslate", "ChromaticPerDropGPU", "ChromaticDropGPU"]
ALL_KW = {"upright_axis": "z", "mirror": [0.5, 0, 1], "angle": [1, 0.25, 0.1], "jitter_sigma_s": 0.01, "color_drop": 0.3}


def test_restatement_returns_what_the_host_draw_returns():
    from geot_amd.openpoints.dataset import ViewProgram
    prog = ViewProgram(ALL, ALL_KW)
    mine, host = vr.draw(prog, 9, SEED, 0, 2), prog.draw(9)
    assert len(mine) == len(host) == len(ALL)
    for a, b in zip(mine, host):
        assert set(a) == set(b)
        for key in set(a) - {"flip", "drop"}:              # (a list of axes and a bool: no shape to compare)
            assert np.asarray(a[key]).shape == np.asarray(b[key]).shape, key
            assert np.asarray(a[key]).dtype == np.asarray(b[key]).dtype, key
    prog.compile(mine, 9)                                  # the unchanged host path takes it


def test_fixed_layout_equals_the_folded_one_where_nothing_folds():
    """compile_fixed (what the device fills in) against compile (the host path): the same ops once SCALE-by-one stands for
    every flip and zeroing that was not drawn; the template is the worst case of every draw."""
    from geot_amd import _lib
    from geot_amd.openpoints.dataset import ViewProgram, pack_fixed_jobs
    from geot_amd.openpoints.dataset import view_program as vp
    prog = ViewProgram(ALL, ALL_KW)
    tmpl = prog.compile_fixed(None, 9)
    assert [o[0] for o in tmpl["ops"]] == [vp.JITTER, vp.MASK, vp.FLIP, vp.FLIP, vp.ZERO, vp.STORE_X, vp.SCALE_JITTER, vp.ROTATE,
                                           vp.TRANSLATE, vp.SCALE_TRANSLATE]
    assert tmpl["ops"][5][1] == 2 | (1 << 2) and tmpl["store_at"] == 5 and (tmpl["n_noise"], tmpl["n_mask"]) == (2, 2)
    modes = set()
    for d in range(24):
        params = vr.draw(prog, 9, SEED, d, 0)
        fixed, (ops, noise, masks) = prog.compile_fixed(params, 9), prog.compile(params, 9)
        kept = [o for o in fixed["ops"] if not (o[0] == vp.SCALE and o[1] == 0 and np.array_equal(o[2], np.ones(3, F))
                                                and len(o[2]) == 3 and o is not fixed["ops"][0])]
        assert [(o[0], o[1]) for o in kept] == [(o[0], o[1]) for o in ops]
        assert all(np.array_equal(np.asarray(a[2], F), np.asarray(b[2], F)) for a, b in zip(kept, ops))
        assert len(fixed["ops"]) == len(tmpl["ops"]) and all(np.array_equal(a, b) for a, b in zip(fixed["noise"], noise))
        assert np.array_equal(fixed["masks"][0], masks[0])
        mode = fixed["ops"][5][1] & 3
        modes.add(mode)
        if mode == 2:
            assert np.array_equal(fixed["masks"][1], masks[1]) and np.array_equal(masks[1], params[7]["mask"] * params[10]["mask"])
    assert modes == {1, 2}
    table, plans, noise, masks = pack_fixed_jobs([(1, 0, prog, None), (0, 1, prog, None)], 2, 2, 9, [1, 2], [4, 4])
    assert table.shape == (2, _lib.VIEW_PROGRAM_JOB_WORDS) and plans.shape == (2, _lib.VIEW_DRAW_PLAN_WORDS) == (2, 296)
    assert plans[1, :4].tolist() == [2, 4, 13, 5] and table[1, :5].tolist() == [0, 1, 10, 2, 2]
    assert noise.shape == (4, 9, 3) and masks.shape == (4, 9)


def test_entry_point_refuses_bad_plans_and_templates_without_a_device():
    """hipErrorInvalidValue (1) before any launch.  The device pointers are bogus non-null addresses: every call here must
    be refused BEFORE the launch, so no accepted call can be part of this test."""
    from geot_amd import _lib
    from geot_amd.openpoints.dataset import ViewProgram, pack_fixed_jobs
    lib = _lib.load()
    prog = ViewProgram(ALL, ALL_KW)
    m = 8
    table, plans, noise, masks = pack_fixed_jobs([(0, 0, prog, None)], 1, 1, m)
    n_noise, n_mask = len(noise), len(masks)

    def args(tab=table, pl=plans, **kw):
        tab, pl = np.ascontiguousarray(tab), np.ascontiguousarray(pl)
        keep.extend([tab, pl])
        a = {"j": 1, "m": m, "n_noise": n_noise, "n_mask": n_mask, "th": tab.ctypes.data, "ph": pl.ctypes.data, "t": 0x1000,
             "p": 0x2000, "seed": SEED, "base": 0, "jobs": 0x3000, "noise": 0x4000, "mask": 0x5000}
        a.update(kw)
        return list(a.values()) + [None]
    keep = []
    for bad in ({"j": 0}, {"j": 65536}, {"m": 0}, {"m": 357913942}, {"n_noise": -1}, {"n_mask": -1}, {"th": None}, {"ph": None},
                {"t": None}, {"p": None}, {"jobs": None}, {"noise": None}, {"mask": None},
                {"n_noise": n_noise - 1}, {"n_mask": n_mask - 1}):
        assert lib.geot_view_draw(*args(**bad)) == 1, bad
    step = lambda k: 8 + 12 * k                       # noqa: E731 -- word of step k: kind, op, pos, flags, c[8]
    kinds = [int(plans[0, step(k)]) for k in range(int(plans[0, 2]))]
    for word, value in ((0, 3), (0, -1), (1, -1), (2, 25), (2, -1), (3, 99), (3, 0),                 # view, slot, steps, store op
                        (step(0), 0), (step(0), 8), (step(0) + 1, 16), (step(0) + 1, 1), (step(0) + 2, 4096), (step(0) + 2, -1),
                        (step(0) + 3, -1),
                        (step(kinds.index(1)) + 1, 0), (step(kinds.index(1)) + 3, 3 << 4),           # SCALE on a JITTER op; mirror form 3
                        (step(kinds.index(2)) + 1, 7), (step(kinds.index(4)) + 1, 0),                # SHIFT / ROTATE on other kinds
                        (step(kinds.index(4)) + 4, np.float32(np.nan).view(np.int32)),               # angle bound NaN
                        (step(kinds.index(4)) + 5, np.float32(2048).view(np.int32)),
                        (step(kinds.index(5)) + 1, 3), (step(kinds.index(5)) + 1, 9),                # FLIP: second op no FLIP; out of range
                        (step(kinds.index(6)) + 1, 0), (step(kinds.index(7)) + 1, 0)):               # DROP / PERMASK on a JITTER op
        pl = plans.copy()
        pl[0, word] = value
        assert lib.geot_view_draw(*args(pl=pl)) == 1, (word, value)
    for word, value in ((2, 17), (2, -1), (8 + 14 * 5 + 1, 0),                   # op count; STORE_X no longer masked
                        (8 + 14 * 0 + 1, 2), (8 + 14 * 1 + 1, 2), (3, 1), (4, 1), (3, -1), (4, -1)):     # rows outside the buffers
        tab = table.copy()
        tab[0, word] = value
        assert lib.geot_view_draw(*args(tab=tab)) == 1, (word, value)
    # x-side steps without a STORE_X op to act on
    pl = plans.copy()
    pl[0, 3] = -1
    assert lib.geot_view_draw(*args(pl=pl)) == 1


def test_header_declares_the_entry_point_and_abi_20():
    import ctypes
    import re
    from geot_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "geot_hip.h")).read()
    assert re.search(r"\bint geot_view_draw\(", hdr) and "geot_view_draw" in _lib.PROTOTYPES
    assert int(re.search(r"GEOT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 20
    assert int(re.search(r"#define GEOT_VIEW_DRAW_MAX_STEPS (\d+)", hdr).group(1)) == _lib.VIEW_DRAW_MAX_STEPS
    assert _lib.load().geot_abi_version() == _lib.ABI_VERSION
    assert "view_draw.hip" in build.SOURCES and "philox.h" in build.HEADERS and "view_draw.h" in build.HEADERS
    assert len(_lib.PROTOTYPES["geot_view_draw"]) == 14 and _lib.PROTOTYPES["geot_view_draw"][-1] is ctypes.c_void_p
    src = os.path.join(root, "geot_amd", "csrc")
    assert "philox4x32_10" not in open(os.path.join(src, "sample_draw.hip")).read().split("sd_permute")[0]    # shared, not copied
    assert '#include "philox.h"' in open(os.path.join(src, "sample_draw.hip")).read()


def test_device_draws_flag_and_state_round_trip():
    import inspect
    import geot_amd.openpoints.dataset as ds
    plain, views = ds.DeviceDraws(SEED), ds.DeviceDraws(SEED, 5, views=True)
    assert plain.views is False and views.views is True and inspect.signature(ds.DeviceDraws.__init__).parameters["views"].default is False
    assert plain.state() == {"seed": SEED, "counter": 0}                   # without the flag: the state as it was
    assert views.state() == {"seed": SEED, "counter": 5, "views": True}
    other = ds.DeviceDraws(1)
    other.set_state(views.state())
    assert other.views is True and other.take(3) == 5 and other.state() == {"seed": SEED, "counter": 8, "views": True}
    other.set_state(plain.state())
    assert other.views is False and other.counter == 0
    h = ds.ViewDrawHandle(SEED, 7, 12)
    assert (h.seed, h.base, h.count) == (SEED, 7, 12) and "base=7" in repr(h)
    for name in ("view_draw", "view_program_draw", "view_program_views_drawn", "DrawLayout", "pack_fixed_jobs"):
        assert callable(getattr(ds, name))
    import torch
    with pytest.raises(RuntimeError, match="DrawLayout"):
        ds.view_draw(torch.zeros(3), 0, 0)
