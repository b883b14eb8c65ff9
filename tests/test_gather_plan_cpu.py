"""The forward gathers' launch plan (csrc/gather_group.hip: tlds_plan) without a GPU.

geot_gather_plan reports what geot_gather_points, geot_group_points and geot_three_interpolate[_into] launch for a shape --
the plain register gather or the table-in-LDS gather and its geometry -- from the planner the four launchers call.  Here the
query is held against the planner restated in Python (tests/_gather_ref.py) over a grid of shapes and at every switch, the
case table of tests/test_gather_forward_gpu.py is held against the plans its rows claim and against a census of the kernel
branches it has to reach, and every fp32 restatement the GPU tests use as a referee is held against its own fp64 bound on
the inputs those tests use: the referee alone must satisfy what the kernels are held to."""
import ctypes
import itertools

import numpy as np
import pytest

import _gather_ref as R
from _fused_ref import gamma


@pytest.fixture(scope="module")
def lib():
    from geot_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def no_impl(monkeypatch):
    monkeypatch.delenv("GEOT_GATHER_IMPL", raising=False)


def same(lib, b, c, m, L, impl=None):
    got, want = R.plan(lib, b, c, m, L), R.plan_ref(b, c, m, L, impl)
    assert got == want, ((b, c, m, L), got, want)
    return got


def test_query_equals_the_restated_planner_over_a_grid(lib):
    seen = set()
    for b, c, m, L in itertools.product((1, 2, 3, 8, 16, 64, 600), (1, 2, 3, 8, 16, 17, 19, 64, 384, 4096),
                                        (0, 1, 5, 7, 100, 777, 2304, 2305, 2458, 8192, 18432, 18433, 36864, 36865, 100000),
                                        (1, 16, 255, 4095, 4096, 4097, 8191, 8192, 12289, 24000, 65536, 262149, 1 << 21)):
        form, p = same(lib, b, c, m, L)
        seen.add((form, p["ch"], min(p["slices"], 4)) if p else (form,))
    assert {s[0] for s in seen} == {R.PLAIN, R.LDS} and len(seen) > 20
    rng = np.random.default_rng(5)
    for _ in range(20000):                       # log-uniform shapes
        b, c = int(2 ** rng.uniform(0, 7)), int(2 ** rng.uniform(0, 12))
        m, L = int(2 ** rng.uniform(0, 16)), int(2 ** rng.uniform(0, 20))
        same(lib, b, c, m, L)


def test_query_equals_the_restated_planner_at_every_switch(lib):
    # the gate L * c >= 65536
    assert same(lib, 1, 16, 64, 4095)[0] == R.PLAIN and same(lib, 1, 16, 64, 4096)[0] == R.LDS
    assert same(lib, 1, 65535, 8, 1)[0] == R.PLAIN and same(lib, 1, 65536, 8, 1)[0] == R.LDS
    assert same(lib, 1, 1, 8, 65535)[0] == R.PLAIN and same(lib, 1, 1, 8, 65536)[0] == R.LDS
    # the table length
    assert same(lib, 1, 2, 36864, 32768) == (R.LDS, {"ch": 1, "chunks": 2, "slices": 8, "per": 4096, "lds": 147456})
    assert same(lib, 1, 2, 36865, 32768)[0] == R.PLAIN
    assert same(lib, 1, 2, 0, 32768)[0] == R.PLAIN and same(lib, 2, 32, 1, 2048)[0] == R.LDS
    # ch: 15 | 16 from the budget, then the caps by 16 and by c
    assert same(lib, 1, 16, 2305, 4096)[1]["ch"] == 15 and same(lib, 1, 16, 2304, 4096)[1]["ch"] == 16
    assert same(lib, 1, 64, 100, 4096)[1]["ch"] == 16 and same(lib, 2, 3, 100, 21846)[1]["ch"] == 3
    assert same(lib, 1, 2, 18432, 32768)[1]["ch"] == 2 and same(lib, 1, 2, 18433, 32768)[1]["ch"] == 1
    for m in range(1, 36865, 97):
        same(lib, 1, 64, m, 4096)
    # slices: 1, 2, 3, 64 and the L // 4096 steps between; want < maxs
    for L, slices in ((4096, 1), (8191, 1), (8192, 2), (8193, 2), (12287, 2), (12288, 3), (12289, 3), (262143, 63), (262144, 64),
                      (262149, 64), (1 << 20, 64)):
        assert same(lib, 1, 16, 7, L)[1]["slices"] == slices, L
    assert same(lib, 16, 8, 18432, 36864)[1] == {"ch": 2, "chunks": 4, "slices": 8, "per": 4608, "lds": 147456}
    assert same(lib, 600, 16, 100, 1 << 16)[1]["slices"] == 1          # want = 1: more workgroups than 512 already
    assert same(lib, 8, 384, 8192, 24000)[1] == {"ch": 4, "chunks": 96, "slices": 1, "per": 24000, "lds": 131072}


def test_both_answer_plain_under_the_switch_and_nothing_for_an_empty_call(lib, monkeypatch):
    shapes = [s for _, s, _, _ in R.LDS_CASES]
    monkeypatch.setenv("GEOT_GATHER_IMPL", "plain")
    for s in shapes:
        assert same(lib, *s, impl="plain") == (R.PLAIN, None), s
    monkeypatch.delenv("GEOT_GATHER_IMPL")
    for s in ((0, 16, 64, 4096), (1, 0, 64, 4096), (1, 16, 64, 0), (-1, 16, 64, 4096)):
        assert same(lib, *s) == (R.NONE, None)
    out = (ctypes.c_longlong * 5)(*([-7] * 5))                          # a prefix on request, nothing where the form is not 2
    assert lib.geot_gather_plan(1, 16, 64, 4096, out, 2) == 2 and list(out) == [16, 1, -7, -7, -7]
    assert lib.geot_gather_plan(1, 16, 64, 4096, None, 0) == 2
    out = (ctypes.c_longlong * 5)(*([-7] * 5))
    assert lib.geot_gather_plan(1, 16, 64, 4095, out, 5) == 1 and list(out) == [-7] * 5


def test_the_compiled_dispatcher_forwards_the_query(lib):
    from geot_amd import build_torch_ext
    disp = build_torch_ext.load("_geot_dispatch_cpp")
    out = (ctypes.c_longlong * 5)()
    assert disp.geot_gather_plan(16, 8, 18432, 36864, ctypes.addressof(out), 5) == 2 and list(out) == [2, 4, 8, 4608, 147456]
    assert disp.geot_gather_plan(1, 16, 64, 4095, None, 0) == 1


def test_case_table_plans_as_it_claims(lib):
    for name, shape, form, fields in R.LDS_CASES:
        got_form, p = same(lib, *shape)
        assert got_form == form, name
        for k, v in fields.items():
            assert p[k] == v, (name, k, p)
        b, c, m, L = shape
        assert b * c * L * 4 <= 19 << 20 and b * c * m < 2 ** 24, name          # output of 18 MB at most; ids stay exact
    for shape in R.PLAIN_CASES:
        assert same(lib, *shape)[0] == R.PLAIN
    last = {name: L - (p["slices"] - 1) * p["per"] for name, (b, c, m, L), f, _ in R.LDS_CASES if f == R.LDS
            for p in [R.plan_ref(b, c, m, L)[1]]}
    assert last["ch capped by c, short last slice"] == 4366 and last["slices, three"] == 4095
    assert last["slices, cap of 64"] == 4038 and last["slices, two uneven"] == 4096


def test_census_of_the_case_table():
    """every class of REQUIRED_CLASSES is reached by at least one row of the table, at storage offset 0"""
    reached = {}
    for name, shape, _, _ in R.LDS_CASES:
        for cls in R.classes(*shape):
            reached.setdefault(cls, []).append(name)
    missing = [c for c in R.REQUIRED_CLASSES if c not in reached]
    assert not missing, missing
    # what the rows were chosen for
    assert "loader second trip" in R.classes(*R.LDS_CASE["row loader's second trip"])
    odd = R.classes(*R.LDS_CASE["partial chunk, odd m"])
    assert {"loader 16-byte", "loader scalar", "loader count % 4 tail", "partial chunk"} <= odd
    assert R.classes(*R.LDS_CASE["shorter than one pass"]) >= {"short pass", "pass tail", "ch=16"}
    assert R.classes(*R.LDS_CASE["second pass of one element"]) >= {"second pass", "pass tail"}
    assert "pass tail" not in R.classes(*R.LDS_CASE["slices, exactly two"])
    assert not R.classes(*R.LDS_CASE["gate, below"]) and not R.classes(*R.LDS_CASE["LDS budget, one over"])
    # an aligned table moved 1, 2, 3 floats on goes through the scalar loader alone
    for off in (1, 2, 3):
        cls = R.classes(*R.LDS_CASE["ch 16"], table_off=off)
        assert "loader scalar" in cls and "loader 16-byte" not in cls


def test_index_and_table_generators():
    for name, (b, c, m, L), _, _ in R.LDS_CASES:
        idx = R.indices(R.rng_of(name), m, (b, L))
        assert idx.min() == 0 and idx.max() == m - 1 and idx.dtype == np.int32
        for bi in range(b):
            assert (idx[bi] == 0).any() and (idx[bi] == m - 1).any()
            if L >= 256:
                assert len(set(idx[bi, 64:192].tolist())) == 1          # one value across two whole waves
    t = R.position_table(3, 19, 777)
    assert t[2, 18, 776] == 3 * 19 * 777 - 1 and t[1, 0, 0] == 19 * 777 and len(np.unique(t)) == t.size


# ---- the fp32 restatements stay inside the bounds the kernels are held to --------------------------------------------------

@pytest.mark.parametrize("name", ["partial chunk, odd m", "ch 16", "slices, three", "one-element table"])
def test_three_interpolate_restatement_meets_its_bound(name):
    b, c, m, L = R.LDS_CASE[name]
    rng = R.rng_of(name)
    table, idx, w = R.position_table(b, c, m), R.indices(rng, m, (b, L, 3)), R.weights(rng, (b, L, 3))
    got = R.three_interpolate_ref32(table, idx, w)
    want, bound = R.three_interpolate_ref64(table, idx, w)
    assert got.dtype == np.float32 and (np.abs(got - want) <= bound).all()
    assert (bound > 0).mean() > 0.9 and np.abs(got - want).max() > 0               # the bound binds, the roundings are real


def cl_inputs(n, ns, c, w_c, name, hub=None):
    rng = R.rng_of("%s %d %d %d %d" % (name, n, ns, c, w_c))
    idx = R.indices(rng, n, (n, ns)) if n * ns else np.zeros((n, ns), np.int32)
    if hub is not None:
        idx[:] = hub
    return (rng, idx, rng.standard_normal((n, c)).astype(np.float32), rng.standard_normal((n, ns, c)).astype(np.float32),
            rng.standard_normal((n, ns, w_c)).astype(np.float32), rng.standard_normal((n, c)).astype(np.float32))


@pytest.mark.parametrize("n,ns,c,w_c", [(1, 1, 1, 1), (257, 3, 33, 11), (300, 8, 32, 8), (64, 16, 12, 1), (64, 5, 12, 12)])
def test_channels_last_restatements_meet_their_bounds(n, ns, c, w_c):
    rng, idx, inp, pos, w, out0 = cl_inputs(n, ns, c, w_c, "cl")
    got = R.aggregation_cl_ref32(inp, pos, w, idx, out0)
    want, bound = R.aggregation_cl_ref64(inp, pos, w, idx, out0)
    assert (np.abs(got - want) <= bound).all()
    wk = R.weights(rng, (n, ns))
    got = R.interpolation_cl_ref32(inp, idx, wk, out0)
    want, bound = R.interpolation_cl_ref64(inp, idx, wk, out0)
    assert (np.abs(got - want) <= bound).all()
    # the scatter referee against a plain loop, and an fp32 sequential sum against its bound
    g = rng.standard_normal((n, c)).astype(np.float32)
    rows, terms = R.interpolation_cl_grad_terms(g, idx, wk)
    s, bound = R.scatter_rows64(rows, terms, n)
    loop = np.zeros((n, c))
    acc32 = np.zeros((n, c), np.float32)
    for i in range(n):
        for t in range(ns):
            loop[idx[i, t]] += g[i].astype(np.float64) * float(wk[i, t])
            acc32[idx[i, t]] += g[i] * wk[i, t]
    assert np.allclose(s, loop, rtol=1e-13, atol=1e-13) and (np.abs(acc32 - s) <= bound).all()
    g_pos, (r_in, t_in), (r_w, t_w) = R.aggregation_cl_grad_ref(inp, pos, w, idx, g)
    gw, _ = R.scatter_rows64(r_w, t_w, n * ns * w_c)
    want_w = np.zeros((n, ns, w_c))
    for ch in range(c):
        want_w[:, :, ch % w_c] += g[:, None, ch].astype(np.float64) * (inp[idx, ch] + pos[:, :, ch]).astype(np.float32)
    assert np.allclose(gw.reshape(n, ns, w_c), want_w, rtol=1e-13, atol=1e-13) and g_pos.shape == (n, ns, c)


def test_channels_first_scatter_referee():
    rng = R.rng_of("cf")
    b, c, m, L = 2, 5, 7, 40
    g, idx, w = rng.standard_normal((b, c, L)).astype(np.float32), R.indices(rng, m, (b, L, 3)), R.weights(rng, (b, L, 3))
    out, bound = R.scatter_cf64(g, idx, w, m)
    loop = np.zeros((b, c, m))
    for bi, e, t in itertools.product(range(b), range(L), range(3)):
        loop[bi, :, idx[bi, e, t]] += g[bi, :, e].astype(np.float64) * float(w[bi, e, t])
    assert np.allclose(out, loop, rtol=1e-13, atol=1e-13) and (bound >= 0).all()
    out1, _ = R.scatter_cf64(g, idx[..., :1], None, m)
    loop = np.zeros((b, c, m))
    for bi, e in itertools.product(range(b), range(L)):
        loop[bi, :, idx[bi, e, 0]] += g[bi, :, e]
    assert np.allclose(out1, loop, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("k", [1, 3, 4, 5, 8, 12, 16, 20])
def test_graph_feature_restatements(k):
    rng = R.rng_of("gf %d" % k)
    b, c, nq, nk = 2, 9, 257, 77
    x_q, x_k = rng.standard_normal((b, c, nq)).astype(np.float32), rng.standard_normal((b, c, nk)).astype(np.float32)
    idx = R.indices(rng, nk, (b, nq, k))
    out = R.graph_feature_ref(x_q, x_k, idx)
    assert out.shape == (b, 2 * c, nq, k) and out.dtype == np.float32
    assert out[1, 3, 200, k - 1] == np.float32(x_k[1, 3, idx[1, 200, k - 1]] - x_q[1, 3, 200]) and out[1, c + 3, 200, 0] == x_q[1, 3, 200]
    g, old = rng.standard_normal(out.shape).astype(np.float32), rng.standard_normal(x_q.shape).astype(np.float32)
    got = R.graph_feature_grad_q_ref(g, old)
    d = g[:, c:].astype(np.float64) - g[:, :c]
    want = old + d.sum(-1)
    assert (np.abs(got - want) <= gamma(k + 2) * (np.abs(old) + np.abs(g[:, c:]).sum(-1) + np.abs(g[:, :c]).sum(-1))).all()


@pytest.mark.parametrize("rows", [1, 255, 256, 257])
def test_fp_weights_restatement_meets_gamma_9(rows):
    d2 = R.fp_weights_rows(rows)
    got, want = R.fp_weights_ref32(d2), R.fp_weights_ref64(d2)
    assert np.isfinite(got).all() and (got > 0).all()
    assert (np.abs(got - want) <= R.FP_WEIGHTS_BOUND * want).all()
    assert (np.abs(got.astype(np.float64).sum(1) - 1) <= gamma(3)).all()
    if rows >= 9:
        assert (d2 == 0).sum(1).tolist().count(1) >= 1 and ((d2 == 0).sum(1) == 3).any() and (d2 == 1e30).any()
        assert ((d2 > 0) & (d2 < np.finfo(np.float32).tiny)).any()
