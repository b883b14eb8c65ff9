"""Every bound of the scatter-gradient planner, over the whole shape space, without a GPU.

The *_grad_ws / _grad_out / _grad_from entry points (three_interpolate_grad, group_points_grad, gather_points_grad and the
kNN graph feature's neighbour gradient) take one of three forms per call: the sorted pair stream of csrc/tile_scatter.hip
(tiles), the whole-row list walk (csr) or the channels-last scatter with float atomics.  geot_scatter_grad_plan reports
the form and the tile plan through the same host function the launches use; a plan it returns must be launchable as it
stands: within the CU's 160 KB of LDS for both kernels, the 16-bit and 12-bit fields of the pair stream and the slack the
entry prefetch reads past a wave's chunks."""
import math

import numpy as np
import pytest

from _scatter_ref import CL, CSR, NONE, TILES, plan, switch, ws_floats_ref

TS_LDS = 160 * 1024
TS_BUILD_STATIC = 2048          # ts_build_kernel's static shared arrays fit in this much
TS_MAX_M, TS_MAX_Q, TS_WAVES, TS_NPF = 32768, 1024, 16, 4
TLDS_FLOATS = 36864             # csr: whole rows of L sources in LDS
BS = (1, 8)
CS = (1, 2, 3, 4, 5, 16, 64, 384)
NTS = ((1, False), (3, True))   # (slots per source, weighted) as at the real call sites

# entry point -> (c, m, L, nt) of shapes that used to be planned past the LDS limit (the retune after the fit)
REGRESSION = {
    "gather_points_grad": (2, 11385, 1275160, 1),
    "group_points_grad": (16, 30000, 729160, 1),
    "three_interpolate_grad": (4, 5524, 679433, 3),
    "three_interpolate_grad_wide": (64, 8587, 1989578, 3),
    "gather_points_grad_one_channel": (1, 24000, 2243858, 1),
}


@pytest.fixture(scope="module")
def lib():
    from geot_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def default_forms(monkeypatch):
    monkeypatch.delenv("GEOT_GATHER_IMPL", raising=False)


def violations(lib, b, c, m, L, nt, weighted):
    """the bounds this shape's plan breaks (empty: none)"""
    form, p = plan(lib, b, c, m, L, nt, weighted)
    zero = lib.geot_grad_ws_needs_zero(b, c, m, L, nt)
    bad = []
    if form == TILES:
        ch, tl, q, ppp, cap = p["ch"], p["tl"], p["q"], p["ppp"], p["cap"]
        lds = ((m * ch + 3) & ~3) * 4 + 2 * tl * ch * 4 + q * TS_WAVES * 4
        checks = [
            ("lds <= 160 KiB", p["lds"] <= TS_LDS),
            ("lds_build <= 160 KiB - static", p["lds_build"] <= TS_LDS - TS_BUILD_STATIC),
            ("ch in {1, 2, 4}, ch <= c", ch in (1, 2, 4) and ch <= c),
            ("tl % 4 == 0, tl >= 4", tl % 4 == 0 and tl >= 4),
            ("tl * ch <= 4096 (staging), tl <= 4096 (12-bit source)", tl * ch <= 4096 and tl <= 4096),
            ("q == ceil(L / tl), no empty tile", q == -(-L // tl) and (q - 1) * tl < L),
            ("q <= 1024", q <= TS_MAX_Q),
            ("ppp == tl * nt <= 0xfff0", ppp == tl * nt and ppp <= 0xFFF0),
            ("ppp + prefetch slack <= cap <= 0xffff", ppp + 64 * TS_WAVES + 64 * TS_NPF <= cap <= 0xFFFF),
            ("lds recomputed", p["lds"] == lds),
            ("lds_build recomputed", p["lds_build"] == (m + 1) * 4 + ppp * 4),
            ("m <= 32768", m <= TS_MAX_M),
            ("ints <= workspace", 0 < p["ints"] <= lib.geot_scatter_grad_ws_floats(b, c, m, L, nt, int(weighted))),
            ("needs_zero == 0", zero == 0),
        ]
    elif form == CSR:
        checks = [("L <= 36864, L * c >= 65536", L <= TLDS_FLOATS and L * c >= 65536), ("needs_zero == 0", zero == 0)]
    elif form == CL:
        checks = [("needs_zero == 1", zero == 1)]
    else:
        checks = [("a valid shape has a form", False)]
    bad = [name for name, ok in checks if not ok]
    return ["%s: %s %s %s" % (name, (b, c, m, L, nt), form, p) for name in bad]


def sweep(lib, shapes):
    bad = []
    for b, c, m, L, nt, w in shapes:
        bad += violations(lib, b, c, m, L, nt, w)
    assert not bad, "%d plans break a bound, e.g.\n%s" % (len(bad), "\n".join(bad[:40]))


def all_configs():
    return [(b, c, nt, w) for b in BS for c in CS for nt, w in NTS]


def random_shapes():
    """200 k seeded (m, L), log-uniform over 1..40 000 targets and 1..5 M sources, each at both slot counts and a b, c
    drawn from the call sites' range"""
    rng = np.random.default_rng(20261016)
    n = 200_000
    ms = np.exp(rng.uniform(0, math.log(40000), n)).astype(np.int64).clip(1, 40000)
    Ls = np.exp(rng.uniform(0, math.log(5e6), n)).astype(np.int64).clip(1, 5_000_000)
    bs = rng.choice(BS, n)
    cs = rng.choice(CS, n)
    shapes = []
    for m, L, b, c in zip(ms.tolist(), Ls.tolist(), bs.tolist(), cs.tolist()):
        for nt, w in NTS:
            shapes.append((b, c, m, L, nt, w))
    return shapes


def test_random_shapes(lib):
    shapes = random_shapes()
    sweep(lib, shapes)
    forms = {plan(lib, b, c, m, L, nt, w)[0] for b, c, m, L, nt, w in shapes[:20000]}
    assert forms == {TILES, CSR, CL}          # the sweep reaches every form


def grid(x, r=16, lo=1):
    return range(max(lo, x - r), x + r + 1)


def test_switch_points(lib):
    """dense grids of +-16 around every switch: m = 32768, L = 36864, L * c = 65536, L * nt = 12 m and q crossing
    1024 (found with the query)"""
    shapes = []
    for b, c, nt, w in all_configs():
        for L in (1, 7, 5000, 24000, 36864, 200000, 1_500_000):
            shapes += [(b, c, m, L, nt, w) for m in grid(TS_MAX_M)]
        for m in (1, 512, 8192, 20000, 40000):
            shapes += [(b, c, m, L, nt, w) for L in grid(TLDS_FLOATS)]
            shapes += [(b, c, m, L, nt, w) for L in grid(-(-65536 // c))]
        for L in (240, 6000, 24000, 36864, 100000):
            shapes += [(b, c, m, L, nt, w) for m in grid(L * nt // 12)]
        for m in (1, 600, 5524, 8192, 11385, 20000, 32768):
            tiles = lambda L: plan(lib, b, c, m, L, nt, w)[0] == TILES     # noqa: E731
            top = switch(tiles, 40000, 1 << 23)    # the longest rows the tile form takes at m targets
            if m <= 11385:                         # (more targets: the LDS of the sums ends them first)
                assert plan(lib, b, c, m, top, nt, w)[1]["q"] == TS_MAX_Q, (b, c, m, nt, top)
            shapes += [(b, c, m, L, nt, w) for L in grid(top)]
            if c >= 4:                             # four channels per workgroup give way to two at q = 1024 tiles as well
                four = lambda L: (plan(lib, b, c, m, L, nt, w)[1] or {}).get("ch") == 4     # noqa: E731
                if four(40000) and not four(1 << 23):
                    shapes += [(b, c, m, L, nt, w) for L in grid(switch(four, 40000, 1 << 23))]
    sweep(lib, shapes)


def test_switches_go_where_they_should(lib):
    """each switch moves the shape to the form the planner documents"""
    for b, c, nt, w in all_configs():
        # more than 32768 targets: no tile plan
        assert plan(lib, b, c, TS_MAX_M, 200000, nt, w)[0] == TILES
        assert plan(lib, b, c, TS_MAX_M + 1, 200000, nt, w)[0] == CL
        # the list walk needs L * c >= 65536, and it is preferred with whole rows in one part and L * nt >= 12 m
        L = -(-65536 // c)
        if L <= TLDS_FLOATS:
            m = max(1, L * nt // 12)
            one_part = c < 4 or TLDS_FLOATS // L >= 4
            assert plan(lib, b, c, m, L, nt, w)[0] == (CSR if one_part else TILES)
            assert plan(lib, b, c, m, L - 1, nt, w)[0] == TILES
            if one_part:
                assert plan(lib, b, c, m + 1, L, nt, w)[0] == TILES
        # beyond the tile form's targets, rows longer than 36864 sources leave only the channels-last form
        assert plan(lib, b, c, 40000, TLDS_FLOATS, nt, w)[0] in ((CSR, CL) if TLDS_FLOATS * c >= 65536 else (CL,))
        assert plan(lib, b, c, 40000, TLDS_FLOATS + 1, nt, w)[0] == CL
    assert plan(lib, 8, 384, 40000, TLDS_FLOATS, 3)[0] == CSR


@pytest.mark.parametrize("entry", sorted(REGRESSION))
def test_regression_shapes(lib, entry):
    """the shapes whose plans used to exceed the LDS limit after the tile retune (the launch was refused on the host)"""
    c, m, L, nt = REGRESSION[entry]
    w = nt == 3
    for b in BS:
        for cc in sorted({c, min(c, 4), 5 if c >= 4 else c}):
            assert plan(lib, b, cc, m, L, nt, w)[0] == TILES
            assert not violations(lib, b, cc, m, L, nt, w)
    # ts_plan reads c only as min(c, 4): the wide shapes' plans at c = 5 are theirs
    assert plan(lib, 8, 5, m, L, nt, w) == plan(lib, 8, c, m, L, nt, w) or c < 4


def test_model_plans_are_pinned(lib):
    """the model's gradient shapes keep the plans bench.py measured"""
    assert plan(lib, 8, 384, 8192, 24000, 3) == (TILES, dict(ch=4, tl=960, q=25, ppp=2880, cap=4160, lds=163392,
                                                              lds_build=44292, ints=1667208))
    assert plan(lib, 8, 64, 24000, 6000 * 32, 1) == (TILES, dict(ch=1, tl=4028, q=48, ppp=4028, cap=5312, lds=131296,
                                                                 lds_build=112116, ints=2045960))
    for c in (64, 128, 256, 384, 512):          # the decoder's stages that interpolate from 512 group centres
        for n in (2048, 6000, 8192):
            assert plan(lib, 8, c, 512, n, 3)[0] == CSR, (c, n)
        assert plan(lib, 8, c, 512, 24000, 3) == (TILES, dict(ch=4, tl=1000, q=24, ppp=3000, cap=4288, lds=41728,
                                                               lds_build=14052, ints=1649672)), c


def test_degenerate_and_forced(lib, monkeypatch):
    for args in ((0, 4, 10, 10), (1, 0, 10, 10), (1, 4, 0, 10), (1, 4, 10, 0)):
        assert plan(lib, *args, 3)[0] == NONE
    monkeypatch.setenv("GEOT_GATHER_IMPL", "plain")      # the atomic kernels: neither sorted form
    assert plan(lib, 8, 384, 8192, 24000, 3)[0] == CL
    monkeypatch.setenv("GEOT_GATHER_IMPL", "csr")
    assert plan(lib, 8, 64, 8192, 24000, 3)[0] == CSR
    assert plan(lib, 8, 64, 24000, 6000 * 32, 1)[0] == CL
    monkeypatch.setenv("GEOT_GATHER_IMPL", "tiles")
    assert plan(lib, 8, 64, 512, 24000, 3)[0] == TILES


def test_workspace_size_is_the_largest_of_its_three_users(lib, monkeypatch):
    """geot_scatter_grad_ws_floats over the seeded shapes of test_random_shapes: the channels-last accumulator, the tile
    plan's workspace, or the one-part reverse index where the list walk's shape condition holds (_scatter_ref)"""
    shapes = random_shapes()
    monkeypatch.setenv("GEOT_GATHER_IMPL", "tiles")      # the tile plan of every shape that has one, preferred or not
    tiles = [(plan(lib, *s)[1] or {}).get("ints", 0) for s in shapes]
    monkeypatch.delenv("GEOT_GATHER_IMPL")
    bad = [(s, got, want) for s, t in zip(shapes, tiles)
           for got, want in [(lib.geot_scatter_grad_ws_floats(*s[:5], int(s[5])), ws_floats_ref(*s[:5], t))] if got != want]
    assert not bad, "%d sizes differ (shape, library, restated), e.g.\n%s" % (len(bad), "\n".join(map(str, bad[:20])))
    assert any(t == 0 for t in tiles) and any(ws_floats_ref(*s[:5], 0) > s[0] * s[1] * s[2] for s in shapes)


def test_list_walk_grid_limit_is_planned(lib, monkeypatch):
    """the list walk's per-part launch puts b * Q on the grid's z axis (at most 65535): a shape beyond it is planned as
    the channels-last form, whose workspace the caller clears, and not refused by the launch after the plan said csr"""
    monkeypatch.setenv("GEOT_GATHER_IMPL", "csr")
    assert plan(lib, 32768, 8, 16385, 18432, 1)[0] == CL             # Q = 2 parts, too many targets to loop them inside
    assert lib.geot_grad_ws_needs_zero(32768, 8, 16385, 18432, 1) == 1
    assert plan(lib, 32767, 8, 16385, 18432, 1)[0] == CSR
    assert lib.geot_grad_ws_needs_zero(32767, 8, 16385, 18432, 1) == 0
    assert plan(lib, 32768, 8, 16384, 18432, 1)[0] == CSR            # parts looped inside the workgroup: b on the z axis
    assert lib.geot_grad_ws_needs_zero(32768, 8, 16384, 18432, 1) == 0
