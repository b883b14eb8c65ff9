"""GPU suite: the forward half of csrc/gather_group.hip through its C entry points, per launch branch, against referees
that do not share code with it (tests/_gather_ref.py; tests/test_gather_plan_cpu.py holds the census of the case table).

* geot_gather_points, geot_group_points, geot_three_interpolate[_into]: every row of LDS_CASES once as planned and once
  under GEOT_GATHER_IMPL=plain, the form asserted from geot_gather_plan both times, both results compared with the referee
  and never with each other.  The table holds its own positions, so the copies must be exact and a wrong row, chunk, slice
  or batch offset names itself; the interpolation must equal the fp32 restatement fl(fl(fl(p0 w0) + fl(p1 w1)) + fl(p2 w2))
  to the bit, and its distance from the fp64 value is printed as a share of gamma(3) sum |p_t w_t|.
* outputs arrive filled with NaN between two margins of a sentinel, which must survive.
* the plain kernels' own edges (L around a block, c around GG_CCHUNK), their atomic gradients against an fp64 scatter-add
  with gamma(n + 1) sum |terms| per element (n counted from the indices) and on integer-valued inputs, exactly.
* geot_graph_feature[_grad]: the kernel each (k, alignment) pair selects is GF_KERNEL below; aligned and offset runs must
  give the same bits and both must equal the referee.
* geot_fp_weights against the fp64 value of its expression under gamma(9) relative (tests/_gather_ref.py says why 9).

Measured on an MI355X, worst share of the bound over all cases (each test prints its own with -s); no kernel bug was found:
* three_interpolate, both forms: equal to the fp32 restatement to the bit everywhere; 0.915 of gamma(3) sum |p_t w_t|
  ("want < maxs")
* plain atomic gradients: gather / group 0.393, three_interpolate 0.310 of gamma(n + 1) sum |terms|; integer cases exact
* graph feature: forward and grad_xq bit-equal for every k, aligned and offset; grad_xk 0.452 of gamma(n + 1) sum |terms|
  and 0.037 of the row rule of tests/_scatter_ref.py
* fp_weights: 0.412 of gamma(9); 2307 of 2307 results equal the numpy fp32 restatement to the bit (division and sqrt are
  correctly rounded in this build)

Value-only faults planted in a scratch build (arithmetic or a loop bound changed, never an address), and what caught them:
* the `count % 4` tail of the 16-byte row loader one element short: gather_points in "partial chunk, odd m" (the 6 outputs
  that read element m - 1 of the last channel), in "slices, cap of 64" and in the storage-offset runs of the odd-m case
* the 16-byte row loader without its second trip: gather_points in "LDS budget, largest table", "ch 15", "ch 16",
  "want < maxs" and "row loader's second trip"
* the LDS kernel's sum contracted to fma: three_interpolate in every LDS row of the table, _into and the wrappers (bits
  differ from the restatement; the fp64 bound alone would not have noticed)
* graph_feature_grad_q_kernel<K4> summing in pairs: grad_xq for k = 4, 8, 16 (the other five k pass)
* (r0 + r1) of fp_weights' norm scaled by 1 + 1e-6: test_fp_weights fails at all four row counts"""
import functools

import numpy as np
import pytest
import torch

import _gather_ref as R
from _fused_ref import at_offset, gamma
from _scatter_ref import rel, scatter64

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

DEV = torch.device("cuda:0")
SENT = -31337.0
MARGIN = 64                                       # floats: keeps the body 16-byte aligned
TOL = 1e-5                                        # tests/test_scatter_boundaries_gpu.py's rule for the *_grad_ws forms


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)        # a copy: the shared referee inputs are read-only


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def lib():
    from geot_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def abi():
    from geot_amd.ext._common import call, ptr
    return call, ptr


class Guarded:
    """numel floats of NaN (or `fill`) with MARGIN sentinels before and after, the body `off` floats past 16-byte alignment"""

    def __init__(self, numel, off=0, fill=float("nan")):
        self.buf = torch.full((2 * MARGIN + off + numel,), SENT, dtype=torch.float32, device=DEV)
        self.lo, self.hi = MARGIN + off, MARGIN + off + numel
        self.body = self.buf[self.lo:self.hi]
        self.body.fill_(fill)
        assert (self.body.data_ptr() - 4 * off) % 16 == 0

    def take(self, shape):
        torch.cuda.synchronize()
        a = host(self.buf)
        assert (a[:self.lo] == SENT).all() and (a[self.hi:] == SENT).all(), "a margin was written"
        return a[self.lo:self.hi].reshape(shape)


def modes(lib, monkeypatch, shape, want_form):
    """yields the mode's name after setting it and asserting the form the launch will take, as planned and under plain"""
    for impl in (None, "plain"):
        if impl:
            monkeypatch.setenv("GEOT_GATHER_IMPL", impl)
        else:
            monkeypatch.delenv("GEOT_GATHER_IMPL", raising=False)
        want = R.PLAIN if impl else want_form
        assert R.plan(lib, *shape)[0] == want == R.plan_ref(*shape, impl=impl)[0], (shape, impl)
        yield impl or "planned"
    monkeypatch.delenv("GEOT_GATHER_IMPL", raising=False)


def group_split(L):
    ns = next(s for s in (4, 3, 2, 1) if L % s == 0)
    return L // ns, ns


@functools.lru_cache(maxsize=2)
def case_inputs(name, shape):
    """host inputs and referees of one (b, c, m, L) case, computed once and never changed"""
    b, c, m, L = shape
    rng = R.rng_of(name)
    table = R.position_table(b, c, m)
    idx1, idx3, w3 = R.indices(rng, m, (b, L)), R.indices(rng, m, (b, L, 3)), R.weights(rng, (b, L, 3))
    want64, bound = R.three_interpolate_ref64(table, idx3, w3)
    ref = {"table": table, "idx1": idx1, "idx3": idx3, "w3": w3, "copy": R.gather_ref(table, idx1),
           "interp32": R.three_interpolate_ref32(table, idx3, w3), "interp64": want64, "bound": bound}
    for v in ref.values():
        v.setflags(write=False)
    return ref


def share_of_bound(got, want64, bound):
    """largest |got - want64| / bound; where the bound is 0 the value must be exact"""
    err = np.abs(got.astype(np.float64) - want64)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def first_diff(got, want):
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    return None if not len(bad) else (tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])], len(bad))


def run_three(abi, shape, t_table, t_idx1, t_idx3, t_w3, out_off=0):
    """gather, group and three_interpolate of one shape through the C entry points -> three host arrays (b, c, L)"""
    call, ptr = abi
    b, c, m, L = shape
    npoints, ns = group_split(L)
    outs = [Guarded(b * c * L, out_off) for _ in range(3)]
    call("geot_gather_points", DEV, b, c, m, L, ptr(t_table), ptr(t_idx1), ptr(outs[0].body))
    call("geot_group_points", DEV, b, c, m, npoints, ns, ptr(t_table), ptr(t_idx1), ptr(outs[1].body))
    call("geot_three_interpolate", DEV, b, c, m, L, ptr(t_table), ptr(t_idx3), ptr(t_w3), ptr(outs[2].body))
    return [o.take((b, c, L)) for o in outs]


def check_three(got, ref, label):
    for k, (op, want) in enumerate((("gather_points", ref["copy"]), ("group_points", ref["copy"]),
                                    ("three_interpolate", ref["interp32"]))):
        assert first_diff(got[k], want) is None, (label, op, "(index, got, want, count):", first_diff(got[k], want))
    return share_of_bound(got[2], ref["interp64"], ref["bound"])


@pytest.mark.parametrize("name,shape,form,fields", R.LDS_CASES, ids=[c[0] for c in R.LDS_CASES])
def test_lds_case_table(lib, abi, monkeypatch, name, shape, form, fields):
    ref = case_inputs(name, shape)
    t = [dev(ref[k]) for k in ("table", "idx1", "idx3", "w3")]
    monkeypatch.delenv("GEOT_GATHER_IMPL", raising=False)
    assert all((R.plan(lib, *shape)[1] or {}).get(k) == v for k, v in fields.items()), (name, R.plan(lib, *shape))
    for mode in modes(lib, monkeypatch, shape, form):
        share =check_three(run_three(abi, shape, *t), ref, (name, mode))
        assert share <= 1.0, (name, mode, share)
        print("three_interpolate %-34s %-8s |err| / (gamma(3) sum|p w|) = %.3f" % (name, mode, share))


@pytest.mark.parametrize("shape", R.PLAIN_CASES, ids=str)
def test_plain_kernels_own_edges(lib, abi, monkeypatch, shape):
    ref = case_inputs("plain %s" % (shape,), shape)
    t = [dev(ref[k]) for k in ("table", "idx1", "idx3", "w3")]
    for mode in modes(lib, monkeypatch, shape, R.PLAIN):
        assert check_three(run_three(abi, shape, *t), ref, (shape, mode)) <= 1.0


@pytest.mark.parametrize("name", R.OFFSET_CASES)
def test_storage_offsets(lib, abi, monkeypatch, name):
    """table, index and weight 1, 2 and 3 floats past fresh storage, and the output too: the row loader's alignment test
    then takes the scalar branch where it took the 16-byte one"""
    shape = R.LDS_CASE[name]
    ref = case_inputs(name, shape)
    base = [dev(ref[k]) for k in ("table", "idx1", "idx3", "w3")]
    for k in (1, 2, 3):
        for which in ("table", "index", "weight", "out"):
            t = list(base)
            if which == "table":
                t[0] = at_offset(base[0], k)
            elif which == "index":
                t[1], t[2] = at_offset(base[1], k), at_offset(base[2], k)
            elif which == "weight":
                t[3] = at_offset(base[3], k)
            for mode in modes(lib, monkeypatch, shape, R.LDS):
                got = run_three(abi, shape, *t, out_off=k if which == "out" else 0)
                assert check_three(got, ref, (name, which, k, mode)) <= 1.0


@pytest.mark.parametrize("name,shape,form", [("partial chunk, odd m", R.LDS_CASE["partial chunk, odd m"], R.LDS),
                                             ("plain", (3, 9, 50, 257), R.PLAIN)])
def test_three_interpolate_into(lib, abi, monkeypatch, name, shape, form):
    """the written block of a wider (b, before + c + after, n) buffer equals geot_three_interpolate to the bit; the channels
    before and after it, in every batch, and the margins keep their sentinel"""
    call, ptr = abi
    b, c, m, n = shape
    before, after = 2, 3
    wide = before + c + after
    ref = case_inputs(name if form == R.LDS else "plain %s" % (shape,), shape)
    t_table, t_idx3, t_w3 = dev(ref["table"]), dev(ref["idx3"]), dev(ref["w3"])
    for mode in modes(lib, monkeypatch, shape, form):
        sep, into = Guarded(b * c * n), Guarded(b * wide * n, fill=SENT)
        call("geot_three_interpolate", DEV, b, c, m, n, ptr(t_table), ptr(t_idx3), ptr(t_w3), ptr(sep.body))
        call("geot_three_interpolate_into", DEV, b, c, m, n, ptr(t_table), ptr(t_idx3), ptr(t_w3),
             ptr(into.body) + 4 * before * n, wide * n)
        a, w = sep.take((b, c, n)), into.take((b, wide, n))
        assert first_diff(a, ref["interp32"]) is None, (mode, first_diff(a, ref["interp32"]))
        assert first_diff(w[:, before:before + c], a) is None, (mode, first_diff(w[:, before:before + c], a))
        assert (w[:, :before] == SENT).all() and (w[:, before + c:] == SENT).all(), mode


@pytest.mark.parametrize("name,shape,form", [("ch 15", R.LDS_CASE["ch 15"], R.LDS), ("plain", (3, 9, 50, 257), R.PLAIN)])
def test_python_wrappers(lib, monkeypatch, name, shape, form):
    """pointnet2_ext allocates its outputs with torch.empty: every element must be written by the launch"""
    from geot_amd.ext import pointnet2_ext as p2
    b, c, m, L = shape
    npoints, ns = group_split(L)
    ref = case_inputs(name if form == R.LDS else "plain %s" % (shape,), shape)
    table, idx1, idx3, w3 = [dev(ref[k]) for k in ("table", "idx1", "idx3", "w3")]
    for mode in modes(lib, monkeypatch, shape, form):
        wide = torch.full((b, c + 4, L), SENT, device=DEV)
        p2.three_interpolate_into(table, idx3, w3, wide, ch_offset=1)
        got = [host(p2.gather_points(table, idx1)), host(p2.group_points(table, idx1.view(b, npoints, ns))).reshape(b, c, L),
               host(p2.three_interpolate(table, idx3, w3))]
        assert check_three(got, ref, (name, mode)) <= 1.0
        w = host(wide)
        assert first_diff(w[:, 1:1 + c], ref["interp32"]) is None and (w[:, :1] == SENT).all() and (w[:, 1 + c:] == SENT).all()


def test_empty_calls_write_nothing(lib, abi):
    call, ptr = abi
    src = dev(R.position_table(2, 4, 8))
    idx = dev(np.zeros((2, 6), np.int32))
    w = dev(np.ones((2, 6), np.float32))
    for b, c, L in ((2, 4, 0), (0, 4, 2), (2, 0, 2)):
        assert R.plan(lib, b, c, 8, L)[0] == R.NONE
        out = Guarded(64)
        call("geot_gather_points", DEV, b, c, 8, L, ptr(src), ptr(idx), ptr(out.body))
        call("geot_group_points", DEV, b, c, 8, L, 1, ptr(src), ptr(idx), ptr(out.body))
        call("geot_group_points", DEV, b, c, 8, 1, L, ptr(src), ptr(idx), ptr(out.body))
        call("geot_three_interpolate", DEV, b, c, 8, L, ptr(src), ptr(idx), ptr(w), ptr(out.body))
        call("geot_three_interpolate_into", DEV, b, c, 8, L, ptr(src), ptr(idx), ptr(w), ptr(out.body), c * L + 5)
        assert np.isnan(out.take((64,))).all()


# ---- the plain atomic gradients -------------------------------------------------------------------------------------------

def atomic_grads(abi, shape, g, idx1, idx3, w3):
    """geot_gather_points_grad, geot_group_points_grad, geot_three_interpolate_grad into zero-filled, guarded buffers"""
    call, ptr = abi
    b, c, m, L = shape
    npoints, ns = group_split(L)
    outs = [Guarded(b * c * m, fill=0.0) for _ in range(3)]
    tg, t1, t3, tw = dev(g), dev(idx1), dev(idx3), dev(w3)
    call("geot_gather_points_grad", DEV, b, c, m, L, ptr(tg), ptr(t1), ptr(outs[0].body))
    call("geot_group_points_grad", DEV, b, c, m, npoints, ns, ptr(tg), ptr(t1), ptr(outs[1].body))
    call("geot_three_interpolate_grad", DEV, b, c, L, m, ptr(tg), ptr(t3), ptr(tw), ptr(outs[2].body))
    return [o.take((b, c, m)) for o in outs]


@pytest.mark.parametrize("shape", R.PLAIN_CASES + [(2, 9, 1, 300)], ids=str)
def test_plain_atomic_gradients(abi, shape):
    """(2, 9, 1, 300): every index is the one hub"""
    b, c, m, L = shape
    rng = R.rng_of("grad %s" % (shape,))
    idx1, idx3, w3 = R.indices(rng, m, (b, L)), R.indices(rng, m, (b, L, 3)), R.weights(rng, (b, L, 3))
    g = rng.standard_normal((b, c, L)).astype(np.float32)
    got = atomic_grads(abi, shape, g, idx1, idx3, w3)
    want1, bound1 = R.scatter_cf64(g, idx1[..., None], None, m)
    want3, bound3 = R.scatter_cf64(g, idx3, w3, m)
    shares = [share_of_bound(got[0], want1, bound1), share_of_bound(got[1], want1, bound1), share_of_bound(got[2], want3, bound3)]
    print("atomic gradients %-18s |err| / (gamma(n + 1) sum|terms|): gather %.3f group %.3f three_interpolate %.3f"
          % ((shape,) + tuple(shares)))
    assert max(shares) <= 1.0, shares
    # integer-valued: |g| <= 8, w in {-2 .. 2}, at most 3 L terms of at most 16 on an element: exact in any order
    gi = rng.integers(-8, 9, (b, c, L)).astype(np.float32)
    wi = rng.integers(-2, 3, (b, L, 3)).astype(np.float32)
    got = atomic_grads(abi, shape, gi, idx1, idx3, wi)
    want1, want3 = R.scatter_cf64(gi, idx1[..., None], None, m)[0], R.scatter_cf64(gi, idx3, wi, m)[0]
    assert np.abs(want3).max() < 2 ** 24
    for k, want in enumerate((want1, want1, want3)):
        assert first_diff(got[k], want.astype(np.float32)) is None, (k, first_diff(got[k], want.astype(np.float32)))


# ---- graph feature ---------------------------------------------------------------------------------------------------------

# the kernel geot_graph_feature / geot_graph_feature_grad select: (k, every pointer they test is 16-byte aligned) -> K4
# (forward tests idx and out, the gradient tests grad_out; K4 = 0 is the generic kernel)
GF_KERNEL = {(k, al): (k // 4 if al and k in (4, 8, 16) else 0) for k in (1, 3, 4, 5, 8, 12, 16, 20) for al in (True, False)}
GF_OFFSETS = ((0, 0), (1, 1), (2, 2), (3, 3), (1, 0), (0, 1))     # (idx, out / grad_out) floats off; the last two: one of the pair


def graph_feature_run(abi, lib, x_q, x_k, idx, g, old, off_idx, off_out):
    call, ptr = abi
    b, c, nq = x_q.shape
    nk, k = x_k.shape[2], idx.shape[2]
    out = Guarded(b * 2 * c * nq * k, off_out)
    t_idx = at_offset(dev(idx), off_idx) if off_idx else dev(idx)
    t_q, t_k = dev(x_q), dev(x_k)                 # named: a temporary's storage is handed to the next allocation
    call("geot_graph_feature", DEV, b, c, nq, nk, k, ptr(t_q), ptr(t_k), ptr(t_idx), ptr(out.body))
    gq, gk = Guarded(b * c * nq), Guarded(b * c * nk, fill=0.0)
    gq.body.copy_(dev(old).reshape(-1))
    t_g = at_offset(dev(g), off_out) if off_out else dev(g)
    floats = int(lib.geot_scatter_grad_ws_floats(b, c, nk, nq * k, 1, 0))
    ws = torch.zeros(max(floats, 1), dtype=torch.float32, device=DEV)
    call("geot_graph_feature_grad", DEV, b, c, nq, nk, k, ptr(t_g), ptr(t_idx), ptr(gq.body), ptr(gk.body), ptr(ws))
    return out.take((b, 2 * c, nq, k)), gq.take((b, c, nq)), gk.take((b, c, nk))


@pytest.mark.parametrize("k", [1, 3, 4, 5, 8, 12, 16, 20])
def test_graph_feature(abi, lib, k):
    b, worst = 2, [0.0, 0.0]
    for nq in (1, 255, 256, 257):
        for c in (1, 8, 9):
            for nk in (1, 77):
                rng = R.rng_of("gf %d %d %d %d" % (k, nq, c, nk))
                x_q, x_k = rng.standard_normal((b, c, nq)).astype(np.float32), rng.standard_normal((b, c, nk)).astype(np.float32)
                idx = R.indices(rng, nk, (b, nq, k))
                g = rng.standard_normal((b, 2 * c, nq, k)).astype(np.float32)
                if nk == 1:
                    # a row of grad_xk is one element, the sum of all nq k values: _scatter_ref.rel takes the error relative
                    # to the row's largest |sum|, which a sum of signed values can bring as near to 0 as it likes (k = 5,
                    # nq = 255, c = 8: a sum of 0.0225 over 1275 unit normals, off by 2e-6).  One sign makes that scale the sum
                    # of |terms|; the rule in any order, gamma(n + 1) sum |terms|, is applied to every case as well
                    g[:, :c] = np.abs(g[:, :c])
                old = rng.standard_normal((b, c, nq)).astype(np.float32)            # grad_xq arrives non-zero
                want_out, want_q = R.graph_feature_ref(x_q, x_k, idx), R.graph_feature_grad_q_ref(g, old)
                g1 = np.ascontiguousarray(g[:, :c].reshape(b, c, nq * k))
                want_k = scatter64(torch.from_numpy(g1), torch.from_numpy(idx.reshape(b, nq * k, 1)), None, nk)
                want_k64, bound_k = R.scatter_cf64(g1, idx.reshape(b, nq * k, 1), None, nk)
                offsets = GF_OFFSETS if (k in (4, 8, 16) and (nq, c, nk) in ((257, 9, 77), (256, 8, 77), (1, 1, 1))) else GF_OFFSETS[:1]
                for off_idx, off_out in offsets:
                    label = (k, nq, c, nk, "idx +%d, out +%d" % (off_idx, off_out), "K4 forward = %d, gradient = %d"
                             % (GF_KERNEL[(k, off_idx == 0 and off_out == 0)], GF_KERNEL[(k, off_out == 0)]))
                    out, gq, gk = graph_feature_run(abi, lib, x_q, x_k, idx, g, old, off_idx, off_out)
                    assert first_diff(out, want_out) is None, (label, first_diff(out, want_out))
                    assert first_diff(gq, want_q) is None, (label, first_diff(gq, want_q))
                    err = rel(torch.from_numpy(gk), want_k)
                    worst[0], worst[1] = max(worst[0], err / (TOL * (30 if nk == 1 else 1))), max(worst[1], share_of_bound(gk, want_k64, bound_k))
                    assert err <= TOL * (30 if nk == 1 else 1), (label, err)      # that file's rule: x 30 for a hub
                    assert worst[1] <= 1.0, (label, worst[1])
    print("graph_feature k = %-2d grad_xk: worst share of the row rule %.3f, of gamma(n + 1) sum|terms| %.3f" % (k, worst[0], worst[1]))


# ---- fp_weights ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b,n", [(1, 1), (1, 255), (2, 128), (1, 257)])
def test_fp_weights(abi, b, n):
    """Held to gamma(9) relative against the fp64 value of the same expression on the same fp32 inputs, and a row's weights
    sum to 1 within gamma(3).  The share of results that equal the numpy fp32 restatement to the bit is printed."""
    call, ptr = abi
    rows = b * n
    d2 = R.fp_weights_rows(rows)
    out, t_d2 = Guarded(rows * 3), dev(d2)
    call("geot_fp_weights", DEV, b, n, ptr(t_d2), ptr(out.body))
    got = out.take((rows, 3))
    want, ref32 = R.fp_weights_ref64(d2), R.fp_weights_ref32(d2)
    err = np.abs(got.astype(np.float64) - want) / want
    print("fp_weights rows = %-4d worst relative error / gamma(9) = %.3f, bit-equal to the fp32 restatement: %d of %d"
          % (rows, err.max() / R.FP_WEIGHTS_BOUND, int((got == ref32).sum()), got.size))
    assert np.isfinite(got).all() and (err <= R.FP_WEIGHTS_BOUND).all(), (err.max(), np.argwhere(err > R.FP_WEIGHTS_BOUND)[:3])
    assert (np.abs(got.astype(np.float64).sum(1) - 1) <= gamma(3)).all()
