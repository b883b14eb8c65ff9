"""The run-time-C NTM kernels' launch plan (csrc/ntm_generic.hip: gen_sig_plan, gen_blocks) and the references their GPU suite
uses, without a GPU.

geot_ntm_generic_plan reports what geot_ntm_sig_t_mean[_grad_raw] and geot_ntm_correct[_grad] launch for a shape -- the
wave-per-point, lane-per-point or matrix-core form and its geometry -- from the plan the launchers read.  Here the query is
held against the planner restated in Python (tests/_ntm_generic_ref.py) over a grid, over log-uniform shapes and at every
switch; the case table of tests/test_ntm_generic_kernels_gpu.py is held against a census of the kernel branches it has to
reach (at 256 CUs); the inputs of every case are held to the conditions that make the comparison mean something (every clamp
region populated, few edge entries, well-conditioned rows); and the op-by-op fp32 restatement of tests/_ntm_point_ref.py is
held to every bound the kernels will be held to, on the same inputs."""
import itertools

import numpy as np
import pytest

import _ntm_generic_ref as G
import _ntm_point_ref as R

CUS = (64, 104, 256, 304)
LAMS = [0.9, 0.0, 1.0]


@pytest.fixture(scope="module")
def lib():
    from geot_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def no_impl(monkeypatch):
    monkeypatch.delenv("GEOT_NTM_GENERIC", raising=False)


def same(lib, b, n, c, backward=0, cus=256, env=None):
    got, want = G.plan(lib, b, n, c, backward, cus), G.plan_ref(b, n, c, backward, cus, env)
    assert got == want, ((b, n, c, backward, cus, env), got, want)
    return got


def under(monkeypatch, env):
    if env is None:
        monkeypatch.delenv("GEOT_NTM_GENERIC", raising=False)
    else:
        monkeypatch.setenv("GEOT_NTM_GENERIC", env)


def test_query_equals_the_restated_planner_over_a_grid(lib, monkeypatch):
    seen = set()
    for env in (None, "m", "r", "w"):
        under(monkeypatch, env)
        for b, n, c, bw, cus in itertools.product((1, 2, 3, 8), (1, 3, 4, 31, 33, 1000, 4097, 24000, 70001, 524353), range(1, 33),
                                                  (0, 1), CUS):
            form, p = same(lib, b, n, c, bw, cus, env)
            seen.add((form, p["cp"], p["tails"], min(p["ksplit"], 5)))
        rng = np.random.default_rng(7)
        for _ in range(4000):                          # log-uniform shapes, 16 000 in all
            b, n, c = int(2 ** rng.uniform(0, 6)), int(2 ** rng.uniform(0, 24)), int(rng.integers(1, 33))
            same(lib, b, n, c, int(rng.integers(2)), int(rng.choice(CUS)), env)
    assert {s[0] for s in seen} == {G.WAVE, G.ROWS, G.MFMA, G.C17} and len(seen) > 25


def test_query_equals_the_restated_planner_at_every_switch(lib, monkeypatch):
    f = lambda *a, **k: same(lib, *a, **k)[0]
    P = lambda *a, **k: same(lib, *a, **k)[1]
    # the default form, CPAD and the specialised count
    assert f(2, 700, 5) == G.ROWS and f(2, 700, 6) == G.MFMA
    assert P(2, 700, 8)["cp"] == 8 and P(2, 700, 9)["cp"] == 16
    assert P(2, 700, 16)["cp"] == 16 and f(2, 700, 17) == G.C17 and P(2, 700, 18)["cp"] == 32
    assert same(lib, 2, 700, 17) == (G.C17, dict(form=4, cp=0, tails=0, ksplit=0, blocks=0, lds=0, correct_blocks=0))
    for c in range(6, 33):
        if c != 17:
            assert P(2, 700, c)["tails"] == int(c & 3 != 0)
    # B N C^2: 2^30 - 1 | 2^30 (mfma -> rows), 4 (2^31 - 1) (rows -> wave)
    assert 32 * 32 * (1 << 20) == 1 << 30
    assert f(1, (1 << 20) - 1, 32) == G.MFMA and f(1, 1 << 20, 32) == G.ROWS
    assert f(1, (1 << 22) - 1, 16) == G.MFMA and f(1, 1 << 22, 16) == G.ROWS
    lim = 0x7fffffff * 4
    n = lim // 1024                                    # c = 32: the largest n with n 1024 < lim is n itself unless it divides
    assert n * 1024 < lim <= (n + 1) * 1024
    assert f(1, n, 32) == G.ROWS and f(1, n + 1, 32) == G.WAVE
    assert 0x7fffffff * 4 == 1 * 0x7fffffff * 2 * 2 and f(1, 0x7fffffff - 1, 2) == G.ROWS and f(1, 0x7fffffff, 2) == G.WAVE
    # the forced forms; fewer than four output elements never reach the MFMA form
    under(monkeypatch, "mfma")
    for pts in (1, 2, 3):
        assert f(1, pts, 1, env="m") == G.ROWS
    assert f(1, 4, 1, env="m") == G.MFMA and f(1, 1, 2, env="m") == G.MFMA and f(2, 700, 5, env="m") == G.MFMA
    assert f(1, 1 << 20, 32, env="m") == G.ROWS
    under(monkeypatch, "rows")
    assert f(2, 700, 20, env="r") == G.ROWS and f(1, n + 1, 32, env="r") == G.WAVE
    for c, cp in ((8, 8), (9, 16), (16, 16), (18, 24), (24, 24), (25, 32), (32, 32)):     # CP steps 8|9, 16|17, 24|25
        assert P(2, 700, c, env="r")["cp"] == cp
    assert P(1, 256 * 8 * 256, 3, env="r")["blocks"] == 2048 and P(1, 256 * 8 * 256 + 1, 3, env="r")["blocks"] == 2048
    assert P(1, 256 * 8 * 104, 3, cus=104, env="r")["blocks"] == 832 and P(1, 255 * 256 + 1, 3, env="r")["blocks"] == 256
    under(monkeypatch, "wave")
    assert f(2, 700, 20, env="w") == G.WAVE
    # per-CU count of the wave form: 160 KB // (lds + 512), clamped 1..8
    for c, per_cu in ((32, 1), (27, 1), (26, 2), (23, 3), (21, 4), (18, 6), (16, 8), (3, 8), (1, 8)):
        p = P(1, 1 << 16, c, env="w")
        assert p["lds"] == 4 * (c + 1) * c * c and p["blocks"] == per_cu * 256 == min(8, max(1, 163840 // (p["lds"] + 512))) * 256, c
    assert P(1, 1057, 32, env="w")["blocks"] == 256 and P(1, 1024, 32, env="w")["blocks"] == 256 and P(1, 1021, 32, env="w")["blocks"] == 256
    assert P(1, 1020, 32, env="w")["blocks"] == 255
    under(monkeypatch, None)
    # the 160 KB gate: one range holds every row tile up to c = 24 (147 KB), ksplit starts at 2 from c = 25, where a row
    # tile's weights grow to four groups of K steps (175 KB)
    assert G.mfma_lds(24, 1) == 150528 <= G.LDS_MAX < G.mfma_lds(25, 1) == 179328 and G.mfma_lds(32, 2) <= G.LDS_MAX
    for c in range(18, 33):
        assert P(1, 64, c)["ksplit"] == (1 if c <= 24 else 2), c
    # the 85 % rule at 256 CUs, c = 9 (nkt = 5): 4096 tiles fill one round; 4097 .. 6963 leave the second round under 85 %
    # of 4096 waves, and ksplit = 2 (2048 waves) takes the first count whose last round is full enough
    assert P(1, 4096 * 32, 9)["ksplit"] == 1 and P(1, 4097 * 32, 9)["ksplit"] > 1
    assert P(1, 6964 * 32, 9)["ksplit"] == 1                         # 6964 * 100 >= 2 * 4096 * 85
    ks = {t: P(1, t * 32, 9)["ksplit"] for t in range(4097, 6964, 7)}
    assert set(ks.values()) == {2, 3, 4}
    assert P(1, 5000 * 32, 9) == dict(form=3, cp=16, tails=1, ksplit=3, blocks=255, lds=G.mfma_lds(9, 3), correct_blocks=2048)
    assert P(2, 70001, 13)["ksplit"] == 4                            # ksplit >= 4 ends the search
    # the loop runs out: ksplit = nkt (c = 6, 8: two row tiles)
    assert P(3, 43693, 6)["ksplit"] == 2 and P(3, 43693, 8)["ksplit"] == 2 and G.mfma_geometry(8)[2] == 2
    assert P(1, 4097 * 32, 4, env=None)["form"] == G.ROWS
    # nb: capped by the tiles
    assert P(1, 33, 9)["blocks"] == 1 and P(1, 16 * 32 + 1, 9)["blocks"] == 2
    # gen_blocks' cap
    for pts, blocks in ((1, 1), (4, 1), (5, 2), (8192, 2048), (8193, 2048), (8188, 2047), (1 << 22, 2048)):
        assert P(1, pts, 9)["correct_blocks"] == blocks
    # too few CUs for the split the LDS gate demands: the launch is refused, the plan says so
    assert same(lib, 1, 64, 32, 0, 1)[0] == G.REFUSED
    # nothing to launch, arguments out of range
    for args in ((0, 5, 9), (5, 0, 9), (1, 5, 0), (1, 5, 33), (-1, 5, 9)):
        assert same(lib, *args) == (0, None)


def test_cus_zero_asks_the_device(lib):
    form, p = G.plan(lib, 3, 43693, 9, 0, 0)            # without a GPU the library assumes 256 CUs
    assert form == G.MFMA and p["blocks"] >= 1


def test_the_compiled_dispatcher_forwards_the_query(lib):
    import ctypes
    from geot_amd import build_torch_ext
    disp = build_torch_ext.load("_geot_dispatch_cpp")
    out = (ctypes.c_longlong * 7)()
    assert disp.geot_ntm_generic_plan(1, 5000 * 32, 9, 1, 256, ctypes.addressof(out), 7) == 3
    assert list(out) == [3, 16, 1, 3, 255, G.mfma_lds(9, 3), 2048]
    assert disp.geot_ntm_generic_plan(1, 5, 33, 0, 256, None, 0) == 0


# ---- the case table ---------------------------------------------------------------------------------------------------------
def table_rows(cus=256):
    """(name, b, n, c, env) of every sig_t_mean case of the GPU suite at this CU count"""
    rows = []
    for c in G.CLASS_COUNTS:
        for env, _ in G.forms_of(c):
            for b, n in G.SMALL_SHAPES:
                rows.append(("small", b, n, c, env))
    for c in (6, 8, 9, 12):
        rows.append(("mfma second tile",) + G.large_mfma_second_tile(c, cus) + (c, None))
    if G.large_mfma_ksplit3(9, cus):
        rows.append(("mfma ksplit 3",) + G.large_mfma_ksplit3(9, cus) + (9, None))
    for c in (2, 3):
        rows.append(("rows second trip",) + G.large_rows_second_trip(c, cus) + (c, "rows"))
    rows.append(("wave second trip",) + G.large_wave_second_trip(32, cus, b=1) + (32, "wave"))
    for c in (3, 9):
        rows.append(("wave second trip",) + G.large_wave_second_trip(c, cus) + (c, "wave"))
    return rows


def test_census_of_the_case_table(lib, monkeypatch):
    reached = {}
    for name, b, n, c, env in table_rows():
        under(monkeypatch, env)
        form, p = same(lib, b, n, c, 0, 256, env)
        if name == "small":
            assert form == G.small_form(b, n, c, env), (b, n, c, env)
        for cls in G.classes(b, n, c, env):
            reached.setdefault(cls, []).append((name, b, n, c, env))
    missing = [c for c in G.REQUIRED_CLASSES if c not in reached]
    assert not missing, missing
    # what the rows were chosen for, at 256 CUs
    at = lambda cls: {(r[3], r[4]) for r in reached[cls]}
    assert {c for c, _ in at("mfma sh 1")} >= {11, 23, 31} and {c for c, _ in at("mfma sh 2")} == {18} and {c for c, _ in at("mfma sh 3")} >= {7, 9, 21, 25, 1, 3, 5}
    assert (14, None) in at("mfma sh 0") and (6, None) in at("mfma sh 0")
    assert {c for c, _ in at("mfma ng 3")} == {18, 20, 21, 23, 24} and {c for c, _ in at("mfma ng 4")} == {25, 31, 32}
    assert {c for c, _ in at("mfma fourth block skipped")} == {18, 20, 21, 23, 24}
    assert {c for c, _ in at("mfma ksplit from the LDS gate")} == {25, 31, 32} and (31, None) in at("mfma uneven ranges")
    assert {c for c, _ in at("mfma second point tile")} >= {6, 8, 9, 12} and {c for c, _ in at("mfma ksplit 3")} == {9}
    assert {c for c, _ in at("mfma ksplit = nkt")} >= {6, 8}
    assert {c for c, _ in at("rows dq 0")} >= {1, 2, 8, 16, 32} and {c for c, _ in at("rows second trip")} == {2, 3}
    assert {c for c, _ in at("wave second trip")} >= {3, 9, 32} and {c for c, _ in at("wave big lds")} >= {32}
    assert {c for c, _ in at("mfma cpad 8")} >= {1, 2, 3, 5, 6, 7, 8}            # the small counts under the forced form too
    # the shapes the searches find at 256 CUs
    assert G.large_mfma_second_tile(9, 256) == (3, 43691) and G.large_rows_second_trip(2, 256) == (1, 524353)
    b, n = G.large_mfma_ksplit3(9, 256)
    assert 4624 <= (b * n + 31) // 32 <= 5221
    assert G.large_wave_second_trip(32, 256, b=1) == (1, 1025) and G.large_wave_second_trip(3, 256)[1] <= 2741
    assert "correct second trip" in G.classes(*G.CORRECT_LARGE, 9) and G.gen_blocks(3 * 2741) == 2048
    assert "correct second trip" not in G.classes(2, 1001, 9)
    # the other CU counts of the fleet find their shapes too
    for cus in (64, 104, 304):
        for name, b, n, c, env in table_rows(cus):
            if name != "small":
                assert b * n * c * c * 4 <= 96 << 20, (cus, name, b, n, c)      # outputs of 96 MB at most


# ---- the references ----------------------------------------------------------------------------------------------------------
def sig_shapes(c):
    shapes = list(G.SMALL_SHAPES)
    if c in (3, 9):
        shapes.append(G.large_wave_second_trip(c, 256))
    if c == 32:
        shapes.append(G.large_wave_second_trip(32, 256, b=1))
    return shapes


_sig = {}


def sig_case(c, b, n):
    if (c, b, n) not in _sig:
        p, cm, W, g = R.sig_inputs(b, n, c, seed=G.seed_of(c, b, n), amp=2.0)
        _sig[(c, b, n)] = (p, cm, W, g, R.sig_t_mean(p, cm, W, g))
    return _sig[(c, b, n)]


def test_c_17_with_default_arguments_is_the_17_class_case():
    p, cm, W, g = R.sig_inputs(2, 50)
    q = R.sig_inputs(2, 50, 17)
    assert all(np.array_equal(a, b) for a, b in zip((p, cm, W, g), q)) and p.shape == (2, 17, 50)
    assert abs(np.abs(W).max() * np.sqrt(34) / 8 - 1) < 0.01 and (W[3] <= 0).all()
    r = R.sig_t_mean(p, cm, W, g)
    assert not r["derived"] and (r["raw_eps"] == R.RAW_EPS).all()
    assert np.array_equal(r["edge"], (np.abs(r["raw"] - R.LO) <= R.EDGE) | (np.abs(r["raw"] - R.HI) <= R.EDGE))
    a, b = R.correct_inputs(2, 50, zero_points=(3,)), R.correct_inputs(2, 50, 17, zero_points=(3,))
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not a[2][5].any() and not a[1][3, 5].any()
    assert R.all_low_head(17) == 3 and R.zero_row(17) == 5 and R.all_low_head(2) == 1 and R.zero_row(3) == 2 and R.zero_row(1) == 0


@pytest.mark.parametrize("c", [c for c in G.CLASS_COUNTS if c > 1])
def test_sig_inputs_meet_the_reference_conditions(c):
    for b, n in sig_shapes(c):
        p, cm, W, g, r = sig_case(c, b, n)
        below, inside, above, edge = R.region_shares(r)
        assert np.abs(W).max() <= 2.0 and (np.abs(W).max() > 1.9 or c < 6)
        assert edge <= 1e-4, (c, b, n, edge)
        head = R.all_low_head(c)
        assert r["below"][:, head].all() and not r["edge"][:, head].any() and (r["draw"][:, head] == 0).all()
        assert np.abs(r["out"][:, head] - 1.0 / c).max() <= 1e-15
        # the derived raw error: the first-order bound of the fp32 dot product, never below half an ulp of the value
        assert (r["raw_eps"] >= (c + 2) * R.U * np.abs(r["raw"]) * (1 - 1e-12)).all()
        if b * n >= 33:
            assert min(below, inside, above) >= 0.01, (c, b, n, below, inside, above)
            cond = (r["draw_bound"] <= 2e-4 * r["rowscale"])[r["inside"]].mean()
            print("ntm-generic-inputs | c %2d (%d, %d) seed %d | below %.4f inside %.4f above %.4f edge %.2e conditioned %.4f"
                  % (c, b, n, G.seed_of(c, b, n), below, inside, above, edge, cond))
            assert cond >= 0.95, (c, b, n, cond)


def c1_weights(kind):
    """c = 1: p = 1 and cm = 1, raw = W[0][0][0] + W[0][0][1] at every point: inside the clamp, or below it"""
    return np.array([[[0.25, 0.5]]], np.float32) if kind == "inside" else np.array([[[0.25, -0.5]]], np.float32)


@pytest.mark.parametrize("kind", ["inside", "below"])
def test_one_class(kind):
    p, cm, _, g = R.sig_inputs(1, 65, 1, amp=2.0)
    W = c1_weights(kind)
    assert (p == 1).all() and (cm == 1).all()
    r = R.sig_t_mean(p, cm, W, g)
    assert r[kind].all() and not r["edge"].any() and (r["out"] == 1).all() and (r["draw"] == 0).all()
    out, draw, gW = R.composite_sig_grad_W(p, cm, W, g)
    assert R.sig_forward_ratio(out, r) <= 1.0 and R.draw_ratio(draw, r) <= 1.0
    if kind == "below":
        assert not draw.any()


@pytest.mark.parametrize("c", [c for c in G.CLASS_COUNTS if c > 1])
def test_an_fp32_restatement_meets_every_sig_bound(c):
    for b, n in sig_shapes(c):
        p, cm, W, g, r = sig_case(c, b, n)
        out, draw, gW = R.composite_sig_grad_W(p, cm, W, g)
        ratios = R.sig_forward_ratio(out, r), R.draw_ratio(draw, r), R.grad_W_ratio(gW, r, b * n)
        print("ntm-generic-fp32 | sig c %2d (%d, %d) | forward %.4f d raw %.4f grad_W %.4f" % ((c, b, n) + ratios))
        assert max(ratios) <= 1.0, (c, b, n, ratios)
        assert not draw[r["above"] & ~r["edge"]].any() and not draw[:, R.all_low_head(c)].any()


@pytest.mark.parametrize("c", G.CLASS_COUNTS)
def test_an_fp32_restatement_meets_every_correct_bound(c):
    zero = (0, 1001, 2001)
    for (b, n), zp in [(s, ()) for s in G.SMALL_SHAPES] + [((2, 1001), zero), (G.CORRECT_LARGE, ())]:
        logits, insT, E, g = R.correct_inputs(b, n, c, zero_points=zp, threshold_points=(1,) if zp else ())
        groups = (np.arange(b * n) % (4 * G.gen_blocks(b * n))) // 4
        for lam in LAMS:
            r = R.correct_logits(logits, insT, E, lam, g, groups=groups)
            dead = ~r["live"]
            if zp:
                assert dead[list(zp) + [1], R.zero_row(c)].all() and dead.sum() == (b * n if lam == 1.0 else 4)
                if lam == 0.0:
                    assert np.float32(r["s"][1, R.zero_row(c)]) == np.float32(1e-12) and r["s"][1, R.zero_row(c)] < 1e-12
            else:
                assert r["live"].all()
            assert r["s"][r["live"]].min() > 1e-3 if r["live"].any() else c == 1
            assert (E < 0).any() and (E > 0).any() or c < 3
            if b * n >= 32:
                assert 0.4 < (insT < 0).mean() < 0.6
            out, gl, gi, gE = R.composite_correct(logits, insT, E, lam, g)
            ratios = (R.correct_forward_ratio(out, r),) + R.correct_grads_ratio(gl, gi, gE, r, b * n)
            assert max(ratios) <= 0.5, (c, b, n, lam, ratios)
            assert (r["grad_ema_t_tile_abs"] <= r["grad_ema_t_abs"] * (1 + 1e-12)).all()
            if lam == 0.0:
                assert not gE.any()
            if lam == 1.0:
                assert not gi.any()
    print("ntm-generic-fp32 | correct c %2d | last ratios %s" % (c, " ".join("%.4f" % x for x in ratios)))
