"""GPU suite: the 17-class per-point NTM kernels (csrc/ntm.hip: sig_t_mean_mfma_kernel forward and backward with its weight-
gradient reduce, sig_t_mean_kernel<C, true>, ntm_correct_fwd / bwd_kernel, ntm_partial_reduce_kernel) at every in-kernel
branch, EVERY element against the fp64 helper tests/_ntm_point_ref.py, whose bounds tests/test_ntm_point_ref_cpu.py holds an
fp32 restatement to.

What the inputs add to tests/test_ntm_gpu.py: weights 8 x nn.Linear's init, so about half the raw values clamp low, 3 % clamp
HIGH (the `raw <= 1 - 1e-5` half of the mask decides) and one head clamps low as a whole; correct_logits operands of both
signs (the fabsf of the L1 norm, the sign term of the backward), lam in {0.9, 0, 1}, rows that are exactly zero (s <= 1e-12).
Shapes: one point (fetch clamp, one block, one partial to reduce), five batches inside a tile, exactly one tile, one tile plus
a point, a batch boundary inside a tile, and (3, 10931) = 1024 full tiles + 25 points, more tiles than any launch has blocks:
block 0 of the backward of sig_t_mean walks tiles 0, 512 (both prefetched) and the partial 1024 (copied directly), block 0 of
its forward, of the d raw kernel and of both ntm_correct kernels walks tile 0 and the partial tile 1024 (eacc carried over).
The block counts come from the library's workspace queries; the forward cap of sig_t_mean (4 x 256 blocks = 1024 < 1025
tiles) has no query.

Buffers passed to the C entry points carry guard words on both sides that must come back untouched; outputs are pre-filled
with NaN, the accumulate-contract gradients (grad_W, grad_ema_t) with non-zero values.

The two long sums at 32 793 points are held to 4 x the error of the op-by-op fp32 composite (see _ntm_point_ref.py):
grad_W 6.2e-7, grad_ema_t 9.8e-7 of the array's scale (composite: 1.56e-7 and 2.45e-7).  The atomic form of the
ntm_correct backward rounds grad_ema_t once per block in arrival order and gets the any-order bound of those additions on top.

Largest error / bound per family (each test prints its own figures, pytest -s), MI355X, 2026-10-19: sig_t_mean forward 0.28
(the row sums; elements 0.02), d raw 0.0075, grad_W 0.0016 at the small shapes and 0.245 at 32 793 points (1.53e-7 of the
scale), grad_W += 0.23, correct_logits out 0.0065, grad_logits 0.0061, grad_ins_T 0.0013, grad_ema_t 0.0003 at the small shapes
and 0.28 at 32 793 points (2.76e-7 of the scale), zero rows 0.0098.  The atomic form measured 9.5e-7 and 8.3e-7 of the scale in
two runs.  No kernel exceeded its bound.  (3, 10931): 1025 tiles, 512 blocks in the backward of sig_t_mean, 1024 in the
others.  Wall time of the slowest case 0.7 s."""
import numpy as np
import pytest
import torch

import _ntm_point_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = R.C
SHAPES = [(1, 1), (5, 7), (1, 32), (1, 33), (2, 1001), (3, 10931)]
LARGE = (3, 10931)
LAMS = [0.9, 0.0, 1.0]
ZERO_SHAPE, ZERO_POINTS = (2, 1001), (0, 1001, 2001)
GUARD, SENTINEL = 64, -7.25            # 256 bytes: the body stays 16-byte aligned


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def guarded(shape, values=None):
    """A buffer between two runs of guard words: NaN-filled, or holding `values`."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    body = whole[GUARD:GUARD + n].view(*shape)
    if values is None:
        body.fill_(float("nan"))
    else:
        body.copy_(dev(values))
    assert body.data_ptr() % 16 == 0
    return body, whole


def intact(*wholes):
    for w in wholes:
        assert bool((w[:GUARD] == SENTINEL).all()) and bool((w[-GUARD:] == SENTINEL).all()), "guard words overwritten"
        assert not bool(torch.isnan(w).any()), "NaN left in a buffer"


def note(what, shape, *ratios):
    print("ntm-point-ratio | %s | (%d, %d) | %s" % (what, shape[0], shape[1], " ".join("%.4f" % r for r in ratios)))


def call(name, *args):
    from geot_amd.ext._common import call as _call
    _call(name, torch.device(DEV), *args)


def launch_geometry(b, n):
    """(tiles, blocks of the sig_t_mean backward, blocks of the 32-point-tile kernels), from the library."""
    from geot_amd import _lib
    lib = _lib.load()
    sig_ws, cor_ws = int(lib.geot_ntm_sig_t_mean_ws_floats(b, n)), int(lib.geot_ntm_correct_ws_floats(b, n))
    assert sig_ws % ((C + 1) * C * C) == 0 and cor_ws % (C * C) == 0
    return (b * n + 31) // 32, sig_ws // ((C + 1) * C * C), cor_ws // (C * C), sig_ws, cor_ws


def need_every_multi_tile_branch(b, n):
    """A later change of a cap fails here instead of silently removing coverage."""
    tiles, sig_blocks, ntm_blocks, _, _ = launch_geometry(b, n)
    assert (b * n) % 32 != 0 and tiles > ntm_blocks, (tiles, ntm_blocks)            # block 0: tile 0, then the partial tile
    assert tiles > 2 * sig_blocks and (tiles - 1) % sig_blocks == 0, (tiles, sig_blocks)   # block 0: two full tiles, then the partial one
    assert tiles > 4 * 256                                                          # the forward cap of sig_t_mean (no query)
    return tiles, sig_blocks, ntm_blocks


class SigCase:
    def __init__(self, b, n):
        self.b, self.n, self.t = b, n, b * n
        self.p, self.cm, self.W, self.g = R.sig_inputs(b, n)
        self.ref = R.sig_t_mean(self.p, self.cm, self.W, self.g)
        below, inside, above, edge = R.region_shares(self.ref)
        assert min(below, inside, above) >= 0.01 and edge <= 1e-4                   # the inputs reach every region
        assert self.ref["below"][:, R.ALL_LOW_HEAD].all()
        self.d_p, self.d_cm, self.d_W, self.d_g = dev(self.p), dev(self.cm), dev(self.W), dev(self.g)

    def module(self):
        from geot_amd import ntm
        mod = ntm.sig_t_mean(C).to(DEV)
        with torch.no_grad():
            for kk, l in enumerate(mod.fc):
                l.weight.copy_(self.d_W[kk])
        return mod


class CorrectCase:
    def __init__(self, b, n, zero=()):
        self.b, self.n, self.t = b, n, b * n
        self.logits, self.insT, self.E, self.g = R.correct_inputs(b, n, zero_points=zero)
        self.d_l, self.d_T, self.d_E, self.d_g = dev(self.logits), dev(self.insT), dev(self.E), dev(self.g)
        self._refs = {}

    def ref(self, lam):
        if lam not in self._refs:
            r = R.correct_logits(self.logits, self.insT, self.E, lam, self.g)
            assert r["s"][r["live"]].min() > 1e-3                                   # well conditioned
            assert 0.4 < (self.E < 0).mean() < 0.6 and (self.insT < 0).any() and (self.insT > 0).any()
            self._refs[lam] = r
        return self._refs[lam]


_cases = {}


def sig_case(b, n):
    if ("sig", b, n) not in _cases:
        _cases[("sig", b, n)] = SigCase(b, n)
    return _cases[("sig", b, n)]


def correct_case(b, n, zero=()):
    if ("cor", b, n, zero) not in _cases:
        _cases[("cor", b, n, zero)] = CorrectCase(b, n, zero)
    return _cases[("cor", b, n, zero)]


def test_the_large_shape_exceeds_every_block_cap():
    tiles, sig_blocks, ntm_blocks = need_every_multi_tile_branch(*LARGE)
    print("ntm-point-geometry | (%d, %d) | tiles %d, sig_t_mean backward blocks %d, ntm blocks %d" % (LARGE + (tiles, sig_blocks, ntm_blocks)))
    for b, n in SHAPES[:-1]:                          # one tile per block everywhere else
        tiles, sig_blocks, ntm_blocks, _, _ = launch_geometry(b, n)
        assert tiles == sig_blocks == ntm_blocks
    r = sig_case(*LARGE).ref
    print("ntm-point-inputs | (%d, %d) | below %.4f inside %.4f above %.4f edge %.2e" % (LARGE + R.region_shares(r)))


# ---- sig_t_mean -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,n", SHAPES)
def test_sig_t_mean_forward(b, n):
    c = sig_case(b, n)
    if (b, n) == LARGE:
        need_every_multi_tile_branch(b, n)
    out, whole = guarded((c.t, C, C))
    call("geot_ntm_sig_t_mean", b, n, C, c.d_p.data_ptr(), c.d_W.data_ptr(), c.d_cm.data_ptr(), out.data_ptr())
    intact(whole)
    ratio = R.sig_forward_ratio(host(out), c.ref)
    note("sig_t_mean forward", (b, n), ratio)
    assert ratio <= 1.0
    with torch.no_grad():
        assert torch.equal(c.module()(c.d_p, c.d_cm), out)          # the module runs this kernel


@pytest.mark.parametrize("b,n", SHAPES)
def test_sig_t_mean_grad_raw(b, n):
    c = sig_case(b, n)
    if (b, n) == LARGE:
        need_every_multi_tile_branch(b, n)
    draw, whole = guarded((c.t, C, C))
    call("geot_ntm_sig_t_mean_grad_raw", b, n, C, c.d_p.data_ptr(), c.d_W.data_ptr(), c.d_cm.data_ptr(), c.d_g.data_ptr(),
         draw.data_ptr())
    intact(whole)
    got = host(draw)
    ratio = R.draw_ratio(got, c.ref)                  # non-edge entries; an exact zero outside the clamp
    note("d raw", (b, n), ratio)
    assert ratio <= 1.0
    assert not got[c.ref["above"] & ~c.ref["edge"]].any() and c.ref["above"].any()
    assert not got[:, R.ALL_LOW_HEAD].any()
    # an edge entry is one of the two legitimate values: off, or its inside value
    e = c.ref["edge"]
    if e.any():
        on = (c.g.astype(np.float64) - (c.g * c.ref["out"]).sum(2, keepdims=True)) / c.ref["den"]
        assert np.all((got[e] == 0) | (np.abs(got[e] - on[e]) <= c.ref["draw_bound"][e]))


@pytest.mark.parametrize("b,n", SHAPES)
def test_sig_t_mean_grad_W_through_autograd(b, n):
    c = sig_case(b, n)
    if (b, n) == LARGE:
        need_every_multi_tile_branch(b, n)
    mod = c.module()
    (mod(c.d_p, c.d_cm) * c.d_g).sum().backward()
    got = host(torch.stack([l.weight.grad for l in mod.fc]))
    ratio = R.grad_W_ratio(got, c.ref, c.t)
    note("grad_W", (b, n), ratio)
    assert ratio <= 1.0
    assert not got[R.ALL_LOW_HEAD].any()


@pytest.mark.parametrize("b,n", [(1, 1), (1, 33), LARGE])
def test_sig_t_mean_grad_W_adds_to_the_buffer_with_the_same_bits_every_run(b, n):
    c = sig_case(b, n)
    if (b, n) == LARGE:
        need_every_multi_tile_branch(b, n)
    _, _, _, ws_floats, _ = launch_geometry(b, n)
    base = np.random.default_rng(11).standard_normal((C, C, 2 * C)).astype(np.float32)
    runs = []
    for _ in range(2):
        gw, whole = guarded((C, C, 2 * C), base)
        ws, ws_whole = guarded((ws_floats,))
        call("geot_ntm_sig_t_mean_grad_w", b, n, C, c.d_p.data_ptr(), c.d_W.data_ptr(), c.d_cm.data_ptr(), c.d_g.data_ptr(),
             gw.data_ptr(), ws.data_ptr())
        intact(whole, ws_whole)                       # every block partial written, nothing beyond
        runs.append(gw.clone())
    assert torch.equal(runs[0], runs[1])
    ratio = R.grad_W_ratio(host(runs[0]), c.ref, c.t, base=base)
    note("grad_W += ", (b, n), ratio)
    assert ratio <= 1.0
    assert np.array_equal(host(runs[0])[R.ALL_LOW_HEAD], base[R.ALL_LOW_HEAD])       # + 0


# ---- correct_logits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("b,n", SHAPES)
def test_correct_logits_through_autograd(b, n, lam):
    from geot_amd import ntm
    c = correct_case(b, n)
    if (b, n) == LARGE:
        need_every_multi_tile_branch(b, n)
    ref = c.ref(lam)
    tl, ti, tE = (t.clone().requires_grad_(True) for t in (c.d_l, c.d_T, c.d_E))
    out = ntm.correct_logits(tl, ti, tE, lam)
    r_out = R.correct_forward_ratio(host(out), ref)
    (out * c.d_g).sum().backward()
    ratios = R.correct_grads_ratio(host(tl.grad), host(ti.grad), host(tE.grad), ref, c.t)
    note("correct_logits lam %.1f: out, grad_logits, grad_ins_T, grad_ema_t" % lam, (b, n), r_out, *ratios)
    assert max((r_out,) + ratios) <= 1.0
    if lam == 0.0:
        assert not bool(tE.grad.any())
    if lam == 1.0:
        assert not bool(ti.grad.any())


@pytest.mark.parametrize("lam", LAMS)
def test_correct_logits_rows_of_exact_zeros(lam):
    """v = 0 in row 5 of three points (every point at lam = 1): nothing from that row in the forward, l g / 1e-12 in the backward,
    each of those entries -- and the grad_ema_t row they are summed into -- held to 1e-5 of its own magnitude."""
    from geot_amd import ntm
    b, n = ZERO_SHAPE
    c = correct_case(b, n, ZERO_POINTS)
    ref = c.ref(lam)
    dead = ~ref["live"]
    assert dead[list(ZERO_POINTS), R.ZERO_ROW].all() and dead.sum() == (c.t if lam == 1.0 else 3)
    assert ZERO_POINTS[-1] >= c.t // 32 * 32 and c.t % 32
    tl, ti, tE = (t.clone().requires_grad_(True) for t in (c.d_l, c.d_T, c.d_E))
    out = ntm.correct_logits(tl, ti, tE, lam)
    r_out = R.correct_forward_ratio(host(out), ref)
    (out * c.d_g).sum().backward()
    assert bool(torch.isfinite(ti.grad).all()) and bool(torch.isfinite(tE.grad).all())
    ratios = R.correct_grads_ratio(host(tl.grad), host(ti.grad), host(tE.grad), ref, c.t)
    note("zero rows lam %.1f: out, grad_logits, grad_ins_T, grad_ema_t" % lam, (b, n), r_out, *ratios)
    assert max((r_out,) + ratios) <= 1.0
    if lam != 1.0:
        assert np.abs(host(ti.grad)[list(ZERO_POINTS), R.ZERO_ROW]).min() > 1e6     # the huge values are there


@pytest.mark.parametrize("b,n", [(1, 1), (5, 7), (1, 33), LARGE])
def test_correct_logits_entry_points(b, n):
    """The C entry points with guarded buffers: forward; the workspace form into a non-zero grad_ema_t (+=, the same bits on
    every run); the atomic form (exported, not reachable from Python at 17 classes; no bit equality claimed); and the workspace
    form without a workspace, which must fall back to the atomic form."""
    lam = 0.9
    c = correct_case(b, n)
    if (b, n) == LARGE:
        need_every_multi_tile_branch(b, n)
    ref = c.ref(lam)
    _, _, ntm_blocks, _, ws_floats = launch_geometry(b, n)
    ins = (c.d_l.data_ptr(), c.d_T.data_ptr(), c.d_E.data_ptr())
    out, whole = guarded((b, C, n))
    call("geot_ntm_correct", b, n, C, lam, *ins, out.data_ptr())
    intact(whole)
    assert R.correct_forward_ratio(host(out), ref) <= 1.0
    base = np.random.default_rng(12).standard_normal((C, C)).astype(np.float32)

    def backward(form):
        gl, w1 = guarded((b, C, n))
        gi, w2 = guarded((c.t, C, C))
        gE, w3 = guarded((C, C), base)
        ws, w4 = guarded((ws_floats,))
        if form == "atomic":
            call("geot_ntm_correct_grad", b, n, C, lam, *ins, c.d_g.data_ptr(), gl.data_ptr(), gi.data_ptr(), gE.data_ptr())
        else:
            call("geot_ntm_correct_grad_ws", b, n, C, lam, *ins, c.d_g.data_ptr(), gl.data_ptr(), gi.data_ptr(), gE.data_ptr(),
                 ws.data_ptr() if form == "ws" else None)
        if form == "ws":
            intact(w4)                                # every block partial written, nothing beyond
        else:
            assert bool(torch.isnan(ws).all())        # untouched
        intact(w1, w2, w3)
        ratios = R.correct_grads_ratio(host(gl), host(gi), host(gE), ref, c.t, base_E=base,
                                       atomic_adds=0 if form == "ws" else ntm_blocks)
        note("correct_logits %s: grad_logits, grad_ins_T, grad_ema_t" % form, (b, n), *ratios)
        assert max(ratios) <= 1.0
        return gl, gi, gE

    first, second = backward("ws"), backward("ws")
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    for form in ("atomic", "no workspace"):
        gl, gi, _ = backward(form)
        assert torch.equal(gl, first[0]) and torch.equal(gi, first[1])              # the same kernel; only grad_ema_t's sum differs
