"""The scatter-add gradients on both sides of every switch of their planner, and at its edges, against fp64.

three_interpolate_grad (3 weighted slots), group_points_grad / gather_points_grad and the kNN graph feature's neighbour
gradient (1 slot) take one of three forms per call (geot_scatter_grad_plan): the sorted pair stream of
csrc/tile_scatter.hip, the whole-row list walk or the channels-last float-atomic scatter.  Every case first asserts, through
that query, the form it means to test, so a retune of the planner fails here instead of silently testing another form;
switch points are found with the query (bisection), only the regression shapes are literal.  Untouched targets must come
out exactly 0 from memory that arrives NaN-poisoned, and the two atomic-free forms must repeat bit for bit."""
import numpy as np
import pytest
import torch

from _scatter_ref import CL, CSR, FORM_NAMES, TILES, plan, rel, scatter64, switch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5


@pytest.fixture(scope="module")
def lib():
    from geot_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def default_forms(monkeypatch):
    monkeypatch.delenv("GEOT_GATHER_IMPL", raising=False)


def make(b, c, L, nt, m, seed, hubs=False):
    """grad_out (b, c, L), idx (b, L, nt) over m targets with the last one untouched (m > 1), weights (b, L, nt)"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, m, (b, L, nt))
    if hubs:                                   # a few targets collect half the pairs
        idx[:, : L // 2] = rng.integers(0, min(3, m), (b, L // 2, nt))
    if m > 1:
        idx[idx == m - 1] = 0
    w = rng.random((b, L, nt)).astype(np.float32)
    w /= w.sum(-1, keepdims=True)
    g = rng.standard_normal((b, c, L)).astype(np.float32)
    return (torch.from_numpy(g).to(DEV), torch.from_numpy(idx.astype(np.int32)).to(DEV), torch.from_numpy(w).to(DEV))


def poison(*shape):
    """a NaN-filled block of the output's size goes back to the caching allocator: the next buffer of that size is it"""
    t = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    del t


def untouched(idx, m):
    b = idx.shape[0]
    flat = idx.reshape(b, -1).long().cpu()
    hit = torch.zeros(b, m, dtype=torch.bool)
    hit.scatter_(1, flat, True)
    return ~hit


def run(fn, want, idx, m, form, hubs=False):
    """fn() -> (b, c, m) gradient; checks it against want and the form's reproducibility"""
    b, c = want.shape[:2]
    poison(b, c, m)
    got = fn()
    torch.cuda.synchronize()
    assert got.shape == (b, c, m)
    err = rel(got, want)
    assert err <= TOL * (30 if hubs else 1), (FORM_NAMES[form], err)       # a hub sums thousands of fp32 terms
    cold = untouched(idx, m)
    assert torch.equal(got.cpu()[cold.unsqueeze(1).expand(b, c, m)], torch.zeros(int(cold.sum()) * c))
    if form in (TILES, CSR):                  # one writer per element, one summation order
        poison(b, c, m)
        assert torch.equal(fn(), got)
    return got


def interp(lib, b, c, m, L, form, seed=0, hubs=False, binding=None):
    from geot_amd.ext import pointnet2_ext as p2
    mod = binding or p2
    assert plan(lib, b, c, m, L, 3)[0] == form, (b, c, m, L, plan(lib, b, c, m, L, 3))
    g, idx, w = make(b, c, L, 3, m, seed, hubs)
    return run(lambda: mod.three_interpolate_grad(g, idx, w, m), scatter64(g, idx, w, m), idx, m, form, hubs), (g, idx, w)


def gather(lib, b, c, m, L, form, seed=0, binding=None):
    from geot_amd.ext import pointnet2_ext as p2
    mod = binding or p2
    assert plan(lib, b, c, m, L, 1)[0] == form, (b, c, m, L, plan(lib, b, c, m, L, 1))
    g, idx, _ = make(b, c, L, 1, m, seed)
    return run(lambda: mod.gather_points_grad(g, idx.reshape(b, L), m), scatter64(g, idx, None, m), idx, m, form)


def group(lib, b, c, m, npoint, ns, form, seed=0, binding=None):
    from geot_amd.ext import pointnet2_ext as p2
    mod = binding or p2
    L = npoint * ns
    assert plan(lib, b, c, m, L, 1)[0] == form, (b, c, m, L, plan(lib, b, c, m, L, 1))
    g, idx, _ = make(b, c, L, 1, m, seed)
    return run(lambda: mod.group_points_grad(g.reshape(b, c, npoint, ns), idx.reshape(b, npoint, ns), m),
               scatter64(g, idx, None, m), idx, m, form)


def neighbour(lib, b, c, nk, nq, k, form, seed=0):
    """the kNN graph feature's gradient into x_k: the first c of its 2c output channels, scattered over nq * k pairs"""
    from geot_amd.openpoints.models.backbone.transformer_ops import graph_feature
    L = nq * k
    assert plan(lib, b, c, nk, L, 1)[0] == form, (b, c, nk, L, plan(lib, b, c, nk, L, 1))
    rng = np.random.default_rng(seed)
    _, idx, _ = make(b, 1, L, 1, nk, seed)
    go = torch.from_numpy(rng.standard_normal((b, 2 * c, nq, k)).astype(np.float32)).to(DEV)
    xq = torch.zeros(b, c, nq, device=DEV, requires_grad=True)
    xk = torch.zeros(b, c, nk, device=DEV, requires_grad=True)

    def fn():
        xk.grad = None
        graph_feature(xq, xk, idx.reshape(b, nq, k)).backward(go)
        return xk.grad
    return run(fn, scatter64(go[:, :c].reshape(b, c, L), idx, None, nk), idx, nk, form)


# ---- the shapes whose plans used to exceed the LDS limit: a RuntimeError (hipErrorInvalidValue on the host) before ------

def test_regression_three_interpolate_grad(lib):
    interp(lib, 1, 4, 5524, 679433, TILES, seed=1)


def test_regression_three_interpolate_grad_wide(lib):
    # ts_plan reads c only as min(c, 4): c = 5 takes c = 64's plan at a fraction of the reference's cost
    assert plan(lib, 1, 5, 8587, 1989578, 3) == plan(lib, 1, 64, 8587, 1989578, 3)
    interp(lib, 1, 5, 8587, 1989578, TILES, seed=2)


@pytest.mark.parametrize("c,m,L,c_table,k", [(2, 11385, 1275160, 2, 8), (5, 30000, 729160, 16, 8), (1, 24000, 2243858, 1, 2)])
def test_regression_one_slot(lib, c, m, L, c_table, k):
    assert plan(lib, 1, c, m, L, 1) == plan(lib, 1, c_table, m, L, 1)
    gather(lib, 1, c, m, L, TILES, seed=3)
    group(lib, 1, c, m, L // k, k, TILES, seed=4)
    neighbour(lib, 1, c, m, L // k, k, TILES, seed=5)


# ---- both sides of every switch --------------------------------------------------------------------------------------

def test_channels_per_workgroup_switches(lib):
    """4 -> 2 -> 1 channels per workgroup as the targets' sums grow, at the model's 24000 sources (b = 8, c = 5)"""
    ch = lambda m: (plan(lib, 8, 5, m, 24000, 3)[1] or {}).get("ch")      # noqa: E731
    m1 = switch(lambda m: ch(m) == 4, 1000, 32768)
    m2 = switch(lambda m: ch(m) >= 2, m1 + 1, 32768)
    pockets = [m for m in range(m1 + 2, m2 + 1) if ch(m) == 4][:1]       # ch = 4 coming back with shorter tiles, if any
    for m in sorted({m1, m1 + 1, m2, m2 + 1} | set(pockets) | {p - 1 for p in pockets}):
        interp(lib, 8, 5, m, 24000, TILES, seed=m)
    assert (ch(m1), ch(m1 + 1), ch(m2), ch(m2 + 1)) == (4, 2, 2, 1)


def test_target_limit(lib):
    interp(lib, 1, 5, 32768, 200000, TILES, seed=6)
    interp(lib, 1, 5, 32769, 200000, CL, seed=7)          # c < 16: the direct atomic kernel
    gather(lib, 1, 16, 32768, 200000, TILES, seed=8)
    gather(lib, 1, 16, 32769, 200000, CL, seed=9)


@pytest.mark.parametrize("nt", [1, 3])
def test_tile_count_limit(lib, nt):
    """the longest rows the tile form takes (q = 1024 tiles) and one source more"""
    b, c, m = 1, 3, 600
    top = switch(lambda L: plan(lib, b, c, m, L, nt)[0] == TILES, 40000, 1 << 23)
    assert plan(lib, b, c, m, top, nt)[1]["q"] == 1024
    for L in (top, top + 1):
        form = plan(lib, b, c, m, L, nt)[0]
        if nt == 3:
            interp(lib, b, c, m, L, form, seed=L)
        else:
            gather(lib, b, c, m, L, form, seed=L)
    assert plan(lib, b, c, m, top + 1, nt)[0] == CL


def test_whole_row_limit(lib):
    """the list walk holds at most 36864 sources of a row in LDS (b = 2, c = 3: one part, list walk preferred)"""
    b, c, m = 2, 3, 4000
    L = switch(lambda L: plan(lib, b, c, m, L, 3)[0] == CSR, 30000, 40000)
    assert L == 36864
    interp(lib, b, c, m, L, CSR, seed=10)
    interp(lib, b, c, m, L + 1, TILES, seed=11)


def test_row_payload_limit(lib):
    """the list walk needs L * c >= 65536"""
    b, c, m = 2, 16, 300
    L = switch(lambda L: plan(lib, b, c, m, L, 1)[0] == CSR, 1000, 8000)
    assert (L * c, (L + 1) * c) == (65520, 65536)
    gather(lib, b, c, m, L, TILES, seed=12)
    gather(lib, b, c, m, L + 1, CSR, seed=13)


def test_few_targets_long_lists(lib):
    """the list walk is preferred from L * nt >= 12 m on"""
    b, c, L = 2, 16, 6000
    m = switch(lambda m: plan(lib, b, c, m, L, 1)[0] == CSR, 1, 5000)
    assert L == 12 * m
    gather(lib, b, c, m, L, CSR, seed=14)
    gather(lib, b, c, m + 1, L, TILES, seed=15)
    gather(lib, b, c, m, L - 1, TILES, seed=16)           # L * nt = 12 m - 1


@pytest.mark.parametrize("c", [5, 16])
def test_reference_smoke_cloud(lib, c):
    """40960 targets (the reference's smoke cloud) with rows beyond the list walk: the channels-last form"""
    interp(lib, 1, c, 40960, 50000, CL, seed=c)


# ---- ragged inputs ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 2, 3, 5])
def test_tiny_rows(lib, L):
    interp(lib, 2, 5, 7, L, TILES, seed=L)
    gather(lib, 2, 5, 7, L, TILES, seed=L)


@pytest.mark.parametrize("tail", [1, 2, 3])
def test_last_tile_of_one_to_three_sources(lib, tail):
    """L % 4 != 0 and the last tile holds 1-3 sources (scalar staging loads)"""
    b, c, m = 2, 6, 3000
    for L in range(50000, 60000):
        p = plan(lib, b, c, m, L, 3)[1]
        if p and L - (p["q"] - 1) * p["tl"] == tail:
            break
    else:
        raise AssertionError("no shape with a last tile of %d sources" % tail)
    interp(lib, b, c, m, L, TILES, seed=L)


def test_unaligned_rows_of_a_wider_gradient(lib):
    """three_interpolate_grad_from at an odd channel offset: rows that do not start on 16 bytes"""
    from geot_amd.ext import pointnet2_ext as p2
    b, c, skip, m, L = 2, 5, 3, 2500, 20000
    assert plan(lib, b, c, m, L, 3)[0] == TILES
    g, idx, w = make(b, c + skip, L, 3, m, 18)
    run(lambda: p2.three_interpolate_grad_from(g, c, idx, w, m, ch_offset=skip), scatter64(g[:, skip:], idx, w, m), idx, m,
        TILES)


@pytest.mark.parametrize("L", [5, 4099, 100000])
def test_one_target(lib, L):
    interp(lib, 2, 5, 1, L, plan(lib, 2, 5, 1, L, 3)[0], seed=L)


@pytest.mark.parametrize("m,L", [(300, 8192), (20000, 100000)])
def test_hubs(lib, m, L):
    interp(lib, 2, 5, m, L, TILES, seed=m, hubs=True)


# ---- the accumulate form and the compiled binding, for a subset --------------------------------------------------------

ACC = [(1, 4, 5524, 679433, TILES), (2, 3, 4000, 36864, CSR), (1, 5, 32769, 200000, CL), (1, 16, 40960, 50000, CL), (2, 5, 7, 3, TILES)]


@pytest.mark.parametrize("b,c,m,L,form", ACC)
def test_batch_wrapper_accumulates(lib, b, c, m, L, form):
    """pointnet2_batch_cuda: *_grad outputs arrive pre-filled and are added to"""
    from geot_amd.ext import pointnet2_batch_cuda as pb
    assert plan(lib, b, c, m, L, 3)[0] == form
    g, idx, w = make(b, c, L, 3, m, 19)
    base = torch.randn(b, c, m, device=DEV)
    want = scatter64(g, idx, w, m) + base.double().cpu()
    out = base.clone()
    pb.three_interpolate_grad_wrapper(b, c, L, m, g, idx, w, out)
    scale = (want.abs() + base.double().cpu().abs()).amax(dim=-1, keepdim=True).clamp_min(1e-30)
    assert float(((out.double().cpu() - want).abs() / scale).max()) <= TOL
    again = base.clone()
    pb.three_interpolate_grad_wrapper(b, c, L, m, g, idx, w, again)
    if form != CL:
        assert torch.equal(out, again)
    if form == TILES:                         # nt = 1 through the group form as well
        assert plan(lib, b, c, m, L, 1)[0] == TILES
        gi = idx[..., :1].contiguous()
        out1 = base.clone()
        pb.group_points_grad_wrapper(b, c, m, L, 1, g, gi, out1)
        want1 = scatter64(g, gi, None, m) + base.double().cpu()
        scale1 = (want1.abs() + base.double().cpu().abs()).amax(dim=-1, keepdim=True).clamp_min(1e-30)
        assert float(((out1.double().cpu() - want1).abs() / scale1).max()) <= TOL


@pytest.mark.parametrize("b,c,m,L,form", ACC)
def test_compiled_binding(lib, b, c, m, L, form):
    """the compiled torch binding (its own c < 16 branch to the direct atomic kernel) against fp64"""
    from geot_amd import build_torch_ext
    cpp = build_torch_ext.load()
    interp(lib, b, c, m, L, form, seed=20, binding=cpp)
    if plan(lib, b, c, m, L, 1)[0] in (TILES, CSR):
        gather(lib, b, c, m, L, plan(lib, b, c, m, L, 1)[0], seed=21, binding=cpp)


# ---- the bare C ABI with a workspace the tile form refuses; the list order switch --------------------------------------

@pytest.mark.parametrize("entry", ["geot_three_interpolate_grad_ws", "geot_group_points_grad_ws"])
@pytest.mark.parametrize("misalign", [0, 4])
def test_workspace_at_four_bytes(lib, entry, misalign):
    """a workspace that is not 8-byte aligned (the tile form refuses it, the list walk does not apply): the call takes the
    channels-last accumulator and clears it itself, although the plan had promised a form that needs no clearing"""
    b, c, m, L = 2, 5, 300, 1000
    nt = 3 if "interpolate" in entry else 1
    assert plan(lib, b, c, m, L, nt)[0] == TILES and lib.geot_grad_ws_needs_zero(b, c, m, L, nt) == 0
    assert L * c < 65536                                  # (the list walk's payload limit)
    g, idx, w = make(b, c, L, nt, m, 22)
    ws = torch.full((lib.geot_scatter_grad_ws_floats(b, c, m, L, nt, int(nt == 3)) + 2,), 1e30, device=DEV)
    out = torch.zeros(b, c, m, device=DEV)
    args = (b, c, L, m, g.data_ptr(), idx.data_ptr(), w.data_ptr()) if nt == 3 else (b, c, m, L, 1, g.data_ptr(), idx.data_ptr())
    assert ws.data_ptr() % 8 == 0
    err = getattr(lib, entry)(*args, out.data_ptr(), ws.data_ptr() + misalign, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert err == 0
    assert rel(out, scatter64(g, idx, w if nt == 3 else None, m)) <= TOL


def exact_case(b, c, L, nt, m, seed):
    """small-integer gradients and power-of-two weights: every summation order gives the same fp32 sum"""
    rng = np.random.default_rng(seed)
    g = rng.integers(-8, 9, (b, c, L)).astype(np.float32)
    idx = rng.integers(0, m, (b, L, nt)).astype(np.int32)
    w = (2.0 ** rng.integers(-2, 2, (b, L, nt))).astype(np.float32)
    return torch.from_numpy(g).to(DEV), torch.from_numpy(idx).to(DEV), torch.from_numpy(w).to(DEV)


def test_arrival_order_lists(lib, monkeypatch):
    """GEOT_REPRODUCIBLE=0 keeps the lists of the list walk in the order the pairs arrived: the same pairs, so sums that
    do not depend on the order are exactly the fp64 ones -- one part per row, then three parts looped in the workgroup"""
    from geot_amd.ext import pointnet2_ext as p2
    monkeypatch.setenv("GEOT_REPRODUCIBLE", "0")
    b, c, m, L = 2, 64, 64, 1024
    assert plan(lib, b, c, m, L, 3)[0] == CSR
    g, idx, w = exact_case(b, c, L, 3, m, 23)
    assert torch.equal(p2.three_interpolate_grad(g, idx, w, m).double().cpu(), scatter64(g, idx, w, m))
    monkeypatch.setenv("GEOT_GATHER_IMPL", "csr")
    # L = 20000 sources are cut into 3 parts.  At c = 8 the workspace the size query grants (b m c floats: no tile plan under
    # this switch) does not hold the index, so the plan is the channels-last form; c = 128 has the room and walks the parts
    for c, form in ((8, CL), (128, CSR)):
        b, m, L = 1, 700, 20000
        assert plan(lib, b, c, m, L, 1)[0] == form and -(-4 * L // 36864) == 3
        g, idx, _ = exact_case(b, c, L, 1, m, 24)
        assert torch.equal(p2.gather_points_grad(g, idx.reshape(b, L), m).double().cpu(), scatter64(g, idx, None, m))
