"""GPU suite: the grid neighbour searches of csrc/knn_grid.hip, per in-kernel branch, against the CPU oracle.

knn_grid_kernel and ball_grid_kernel choose a branch per query from its data.  tests/_grid_ref.py names the branch of
every query (a NumPy restatement of the grid, used as a classifier only; tests/test_grid_search_cpu.py holds its census),
and every result here is compared with the oracle class by class, so that a failure names the entry point, the cloud, the
class and the first query that differs.  Indices and fp32 squared distances must be bit-equal.  The inputs are the smallest
the grid takes: 2048 reference points per cloud (GEOT_NN_IMPL=grid), ten clouds stacked as one batch so that each has its
own box, 241 queries per cloud.
"""
import numpy as np
import pytest
import torch

import _grid_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]      # each test under its own limit; each takes a second or so

DEV = "cuda:0"
INVALID = 1                 # hipErrorInvalidValue


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def lib():
    from geot_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def ext(lib):
    from geot_amd.ext import pointnet2_ext, pointnet2_batch_cuda

    class E:
        p2 = pointnet2_ext
        p2b = pointnet2_batch_cuda
    return E


@pytest.fixture()
def grid_env(monkeypatch):
    monkeypatch.setenv("GEOT_NN_IMPL", "grid")
    return monkeypatch


def _same(got, want):
    """bit-equal rows; NaN distances compare as NaN"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype.kind == "f":
        eq = (got.view(np.int32) == want.view(np.int32)) | (np.isnan(got) & np.isnan(want))
    else:
        eq = got == want
    return eq.reshape(eq.shape[0], -1).all(1)


def _check(entry, labels, pairs, clouds=R.CLOUDS):
    """pairs: (field, got, want) arrays of (cloud, query, ...); labels: per cloud the class of every query.  Compared class
    by class: the message names entry point, cloud, class and the first query that differs."""
    for c, name in enumerate(clouds):
        for cls in np.unique(labels[c]):
            rows = np.flatnonzero(labels[c] == cls)
            for field, got, want in pairs:
                ok = _same(got[c][rows], want[c][rows])
                if not ok.all():
                    j = int(rows[np.flatnonzero(~ok)[0]])
                    pytest.fail("%s: cloud %s, class %s, query %d (%d of the class's %d differ): %s\n got  %s\n want %s"
                                % (entry, name, cls, j, int((~ok).sum()), rows.size, field, got[c][j], want[c][j]))


def _knn_labels(case):
    out = []
    for f, r, m in zip(case["fast"], case["ring"], case["marginal"]):
        out.append(np.array([a + ("/" + b if b else "") + (" (marginal)" if mm else "") for a, b, mm in zip(f, r, m)]))
    return out


_ORACLE = {}


def _oracle_knn(oracle, nr, k):
    """computed once per (nr, k), shared, never written to"""
    if (nr, k) not in _ORACLE:
        ref, qry = R.inputs(nr)
        wi, wd = oracle.knn_sorted(qry, ref, k)
        wi.setflags(write=False)
        wd.setflags(write=False)
        _ORACLE[nr, k] = (wi, wd)
    return _ORACLE[nr, k]


# ---- knn_sorted -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nr,k", R.KNN_CASES)
def test_knn_sorted_per_class(lib, oracle, grid_env, nr, k):
    from geot_amd.knn_cuda import knn_sorted
    case = R.knn_case(lib, nr, k)
    ref, qry = dev(case["ref"]), dev(case["qry"])
    b = ref.shape[0]
    assert lib.geot_knn_grid_eligible(b, R.NQ, nr, k) == 1
    d_g, i_g = knn_sorted(qry, ref, k)
    wi, wd = _oracle_knn(oracle, nr, k)
    labels = _knn_labels(case)
    _check("knn_sorted (grid) k = %d, nr = %d" % (k, nr), labels, [("idx", host(i_g), wi), ("dist2", host(d_g), wd)])
    grid_env.setenv("GEOT_NN_IMPL", "wave")                            # the brute-force sibling: the same bits
    assert lib.geot_knn_grid_eligible(b, R.NQ, nr, k) == 0
    d_b, i_b = knn_sorted(qry, ref, k)
    _check("knn_sorted grid against wave, k = %d, nr = %d" % (k, nr), labels,
           [("idx", host(i_g), host(i_b)), ("dist2", host(d_g), host(d_b))])


def test_knn_ring_stop_keeps_its_slack(lib, oracle, grid_env):
    """A box a few extents off the origin, where a point is counted to the cell above the face it sits under: the nearest
    neighbour of query 0 lies outside its 3-cell block, inside the block's bound.  Only the h / 1000 slack of the ring
    stop sends the search on to ring 2 (tests/test_grid_search_cpu.py asserts the construction)."""
    from geot_amd.knn_cuda import knn_sorted
    case = R.make_face_rounding_case()
    assert lib.geot_knn_grid_eligible(1, 8, R.NR, R.FACE_K) == 1
    d_g, i_g = knn_sorted(dev(case["qry"]), dev(case["ref"]), R.FACE_K)
    wi, wd = oracle.knn_sorted(case["qry"], case["ref"], R.FACE_K)
    assert wi[0, 0, 0] == case["p_index"]
    labels = [np.array(["rings_only/r2_3_bound, neighbour outside the block"] + ["rings_only"] * 7)]
    _check("knn_sorted (grid) k = 1, face-rounding cloud", labels, [("idx", host(i_g), wi), ("dist2", host(d_g), wd)],
           clouds=("face_rounding",))


# ---- three_nn ---------------------------------------------------------------------------------------------------------
def _three_nn(ext, binding, unknown, known):
    if binding == "p2":
        d, i = ext.p2.three_nn(unknown, known)
        return d, i
    b, n, m = unknown.shape[0], unknown.shape[1], known.shape[1]
    d = torch.full((b, n, 3), -7.0, dtype=torch.float32, device=DEV)
    i = torch.full((b, n, 3), -7, dtype=torch.int32, device=DEV)
    ext.p2b.three_nn_wrapper(b, n, m, unknown, known, d, i)
    return d, i


@pytest.mark.parametrize("binding", ["p2", "p2b"])
def test_three_nn_grid_path_per_class(lib, ext, oracle, grid_env, binding):
    """2048 known points: the grid with k = 3, rings only"""
    case = R.knn_case(lib, R.NR, 3)
    assert lib.geot_knn_grid_eligible(len(R.CLOUDS), R.NQ, R.NR, 3) == 1
    d, i = _three_nn(ext, binding, dev(case["qry"]), dev(case["ref"]))
    wd, wi = oracle.three_nn(case["qry"], case["ref"])
    _check("three_nn (%s, grid, 2048 known)" % binding, _knn_labels(case), [("idx", host(i), wi), ("dist2", host(d), wd)])


@pytest.mark.parametrize("binding", ["p2", "p2b"])
def test_three_nn_every_third_reference_known(lib, ext, oracle, grid_env, binding):
    """683 known points, below the grid's floor even when it is forced: the linear scan, the same contract"""
    ref, _ = R.inputs(R.NR)
    known = np.ascontiguousarray(ref[:, ::3])
    assert known.shape[1] == 683 and lib.geot_knn_grid_eligible(len(R.CLOUDS), R.NR, 683, 3) == 0
    d, i = _three_nn(ext, binding, dev(ref), dev(known))
    wd, wi = oracle.three_nn(ref, known)
    labels = [np.array(["linear_scan"] * R.NR)] * len(R.CLOUDS)
    _check("three_nn (%s, 683 known)" % binding, labels, [("idx", host(i), wi), ("dist2", host(d), wd)])


# ---- ball_query -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binding", ["p2", "p2b"])
@pytest.mark.parametrize("radius,ns", R.BALL_CASES)
def test_ball_query_per_class(lib, ext, oracle, grid_env, radius, ns, binding):
    case = R.ball_case(lib, R.NR, radius, ns)
    ref, qry = dev(case["ref"]), dev(case["qry"])
    b = ref.shape[0]
    assert lib.geot_ball_grid_eligible(b, R.NR, R.NQ, radius, ns) == 1
    if binding == "p2":
        got = ext.p2.ball_query(qry, ref, radius, ns)
    else:
        got = torch.full((b, R.NQ, ns), -7, dtype=torch.int32, device=DEV)
        ext.p2b.ball_query_wrapper(b, R.NR, R.NQ, radius, ns, qry, ref, got)
    want = oracle.ball_query(case["qry"], case["ref"], radius, ns)
    _check("ball_query (%s, grid) radius = %g, nsample = %d" % (binding, radius, ns), case["cls"], [("idx", host(got), want)])
    if binding == "p2":                                                # the linear scan: the same bits
        grid_env.setenv("GEOT_NN_IMPL", "wave")
        assert lib.geot_ball_grid_eligible(b, R.NR, R.NQ, radius, ns) == 0
        scan = ext.p2.ball_query(qry, ref, radius, ns)
        _check("ball_query grid against the linear scan, radius = %g, nsample = %d" % (radius, ns), case["cls"],
               [("idx", host(got), host(scan))])


# ---- pointops.knn: the certified fast path ---------------------------------------------------------------------------
POINTOPS_CLOUDS = ("dups", "lattice", "volume")


def _uncertified(oracle, x, k):
    """queries whose k + 1 nearest squared distances are not strictly increasing (or reach the heap's 1e10 root): the ones
    the fast path hands to the literal heap"""
    _, d = oracle.knn_sorted(x, x, k + 1)
    strict = (d[..., :-1] < d[..., 1:]).all(-1) & (d[..., k] < np.float32(1e10))
    return (~strict).sum(1)


@pytest.mark.parametrize("k", [7, 8, 47, 48, 63])
def test_pointops_knn_certified_fast_path(lib, oracle, grid_env, k):
    """k + 1 crosses both ends of the select band, and 64 is the last list the grid takes.  Against the oracle's literal
    max-heap; the count of queries the certification hands on is read out of the workspace."""
    from geot_amd.pointops.functions import pointops
    ref, _ = R.inputs(R.NR)
    x = np.ascontiguousarray(ref[[R.CLOUDS.index(c) for c in POINTOPS_CLOUDS]])
    B, N = x.shape[0], x.shape[1]
    assert lib.geot_knn_grid_eligible(B, N, N, k + 1) == 1 and k < 64
    idx, dist = pointops.knn(dev(x), dev(x), k)
    off = (np.arange(B, dtype=np.int32) + 1) * N
    wi, wd = oracle.knnquery_heap(k, x.reshape(-1, 3), x.reshape(-1, 3), off, off)
    wi = wi.reshape(B, N, k).astype(np.int64) - (off - N)[:, None, None]
    labels = [np.array(["certified_or_heap"] * N)] * B
    want_dist = host(torch.sqrt(dev(wd))).reshape(B, N, k)              # the square root the product takes, of the oracle's d2
    _check("pointops.knn k = %d" % k, labels, [("idx", host(idx), wi), ("dist", host(dist), want_dist)], clouds=POINTOPS_CLOUDS)
    # this test's own call, one cloud at a time, so that the count can be taken out of the workspace
    want_q = _uncertified(oracle, x, k)
    for c, name in enumerate(POINTOPS_CLOUDS):
        pts = dev(x[c])
        o = dev(np.array([N], np.int32))
        nbytes = int(lib.geot_knnquery_heap_ws_bytes(1, N, N, k))
        gbytes = int(lib.geot_knn_grid_ws_bytes(1, N))
        assert nbytes >= gbytes + 4 * (2 * N * (k + 1) + N + 1)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        gi = torch.full((N, k), -7, dtype=torch.int32, device=DEV)
        gd = torch.full((N, k), -7.0, dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        rc = lib.geot_knnquery_heap_ws(1, N, N, k, pts.data_ptr(), pts.data_ptr(), o.data_ptr(), o.data_ptr(), gi.data_ptr(),
                                       gd.data_ptr(), ws.data_ptr(), nbytes, None)
        torch.cuda.synchronize()
        assert rc == 0
        qcount = int(ws[gbytes + 4 * (2 * N * (k + 1) + N):][:4].view(torch.int32).item())
        assert qcount == int(want_q[c]), "pointops.knn k = %d, cloud %s: %d queries handed to the heap, %d have ties" % (
            k, name, qcount, int(want_q[c]))
        assert (qcount > 0) if name != "volume" else (qcount == 0), (name, qcount)
        assert np.array_equal(host(gi).astype(np.int64), wi[c]), name


# ---- geot_spatial_order -----------------------------------------------------------------------------------------------
def test_spatial_order_is_the_morton_order_of_the_grid(lib, grid_env):
    from geot_amd.ntm import spatial_order
    names = ("volume", "clusters", "identical")
    ref, _ = R.inputs(R.NR)
    x = np.ascontiguousarray(ref[[R.CLOUDS.index(c) for c in names]])
    plan = R.knn_plan(lib, len(names), R.NR, R.NR, 8)
    order = host(spatial_order(dev(x))).reshape(len(names), R.NR)
    again = host(spatial_order(dev(x))).reshape(len(names), R.NR)
    for c, name in enumerate(names):
        local = order[c].astype(np.int64) - c * R.NR
        assert np.array_equal(np.sort(local), np.arange(R.NR)), "spatial_order: cloud %s is not a permutation" % name
        keys = R.morton_keys(x[c], plan["gmax"])[local]
        assert (np.diff(keys) >= 0).all(), "spatial_order: cloud %s, Morton keys descend at position %d" % (
            name, int(np.flatnonzero(np.diff(keys) < 0)[0]))
        assert np.bincount(keys).max() <= plan["sort_max"]
        inside = np.diff(keys) == 0                                     # neighbours in one cell: ascending index
        assert (np.diff(local)[inside] > 0).all(), "spatial_order: cloud %s, indices descend inside a cell" % name
        assert np.array_equal(order[c], again[c]), name
    assert np.array_equal(order[2] - 2 * R.NR, np.arange(R.NR))       # all points identical: one cell, the identity
    assert len(np.unique(R.morton_keys(x[0], plan["gmax"]))) > 1000   # the volume cloud does spread over the cells


# ---- the workspace contract of the _ws entry points, by ctypes --------------------------------------------------------
def _buffers(nbytes):
    """a workspace of nbytes + 16 filled with a pattern, and that pattern"""
    ws = torch.full((nbytes + 16,), 0x5A, dtype=torch.uint8, device=DEV)
    return ws, ws.clone()


@pytest.mark.parametrize("entry", ["knn_sorted_ws", "three_nn_ws", "ball_query_ws"])
def test_ws_contract(lib, oracle, grid_env, entry):
    """No workspace, or a short one: the brute-force kernel answers (the same result; the workspace is not written).
    A workspace at a 4-byte offset: hipErrorInvalidValue, outputs and workspace untouched.  A good one: the grid."""
    names = ("volume", "dups")
    ref_all, qry_all = R.inputs(R.NR)
    sel = [R.CLOUDS.index(c) for c in names]
    ref, qry = np.ascontiguousarray(ref_all[sel]), np.ascontiguousarray(qry_all[sel])
    b, k = len(names), {"knn_sorted_ws": 16, "three_nn_ws": 3, "ball_query_ws": 32}[entry]
    r, q = dev(ref), dev(qry)
    need = int(lib.geot_knn_grid_ws_bytes(b, R.NR))
    if entry == "ball_query_ws":
        assert lib.geot_ball_grid_eligible(b, R.NR, R.NQ, 0.1, k) == 1
        want = [("idx", oracle.ball_query(qry, ref, 0.1, k))]
    else:
        assert lib.geot_knn_grid_eligible(b, R.NQ, R.NR, k) == 1
        wi, wd = oracle.knn_sorted(qry, ref, k)
        if entry == "three_nn_ws":
            wd, wi = oracle.three_nn(qry, ref)
        want = [("idx", wi), ("dist2", wd)]

    def run(ws_ptr, ws_bytes):
        idx = torch.full((b, R.NQ, k), -7, dtype=torch.int32, device=DEV)
        d2 = torch.full((b, R.NQ, k), -7.0, dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        if entry == "knn_sorted_ws":
            rc = lib.geot_knn_sorted_ws(b, R.NQ, R.NR, k, q.data_ptr(), r.data_ptr(), idx.data_ptr(), d2.data_ptr(), ws_ptr,
                                        ws_bytes, None)
        elif entry == "three_nn_ws":
            rc = lib.geot_three_nn_ws(b, R.NQ, R.NR, q.data_ptr(), r.data_ptr(), d2.data_ptr(), idx.data_ptr(), ws_ptr,
                                      ws_bytes, None)
        else:
            rc = lib.geot_ball_query_ws(b, R.NR, R.NQ, 0.1, k, q.data_ptr(), r.data_ptr(), idx.data_ptr(), ws_ptr, ws_bytes, None)
        torch.cuda.synchronize()
        return rc, {"idx": host(idx), "dist2": host(d2)}

    labels = [np.array(["all"] * R.NQ)] * b
    ws, pattern = _buffers(need)
    assert ws.data_ptr() % 16 == 0
    for what, (ptr, nbytes) in (("no workspace", (None, 0)), ("no workspace but a size", (None, need)),
                                ("short workspace", (ws.data_ptr(), need - 16))):
        rc, out = run(ptr, nbytes)
        assert rc == 0, (entry, what, rc)
        _check("%s, %s" % (entry, what), labels, [(f, out[f], w) for f, w in want], clouds=names)
        assert torch.equal(ws, pattern), "%s, %s: the workspace was written" % (entry, what)
    rc, out = run(ws.data_ptr() + 4, need)
    assert rc == INVALID, "%s: a workspace at a 4-byte offset returned %d" % (entry, rc)
    assert (out["idx"] == -7).all() and (out["dist2"] == -7.0).all(), "%s: a refused call wrote its outputs" % entry
    assert torch.equal(ws, pattern), "%s: a refused call wrote the workspace" % entry
    rc, out = run(ws.data_ptr(), need)
    assert rc == 0
    _check("%s, full workspace" % entry, labels, [(f, out[f], w) for f, w in want], clouds=names)
    assert not torch.equal(ws[:need], pattern[:need]) and torch.equal(ws[need:], pattern[need:]), \
        "%s: the grid did not run in the workspace, or ran past it" % entry


def test_spatial_order_ws_contract(lib, grid_env):
    """geot_spatial_order has no other path: without a workspace of the full size, 16-byte aligned, it is refused"""
    ref, _ = R.inputs(R.NR)
    x = dev(ref[:2])
    need = int(lib.geot_knn_grid_ws_bytes(2, R.NR))
    ws, pattern = _buffers(need)
    for what, (ptr, nbytes) in (("no workspace", (None, need)), ("short workspace", (ws.data_ptr(), need - 16)),
                                ("4-byte offset", (ws.data_ptr() + 4, need))):
        order = torch.full((2 * R.NR,), -7, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        rc = lib.geot_spatial_order(2, R.NR, x.data_ptr(), order.data_ptr(), ptr, nbytes, None)
        torch.cuda.synchronize()
        assert rc == INVALID, (what, rc)
        assert (order == -7).all() and torch.equal(ws, pattern), what
    order = torch.full((2 * R.NR,), -7, dtype=torch.int32, device=DEV)
    assert lib.geot_spatial_order(2, R.NR, x.data_ptr(), order.data_ptr(), ws.data_ptr(), need, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(np.sort(host(order)), np.arange(2 * R.NR)) and torch.equal(ws[need:], pattern[need:])
