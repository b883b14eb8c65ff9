"""GPU suite: the run-time-C per-point NTM kernels (csrc/ntm_generic.hip: gen_sig_t_mean_kernel, gen_sig_t_mean_rows_kernel<CP>,
gen_sig_t_mean_mfma_kernel<CPAD, BACKWARD, TAILS>, gen_correct_fwd / bwd_kernel) at every form and in-kernel branch, EVERY
element against the fp64 helper tests/_ntm_point_ref.py, whose bounds tests/test_ntm_generic_plan_cpu.py holds an fp32
restatement to.  The class counts, shapes and forms are the table of tests/_ntm_generic_ref.py; the CPU test holds a census of
the branches that table reaches.

Every case first asserts, from geot_ntm_generic_plan at this device's CU count, that the form and plan it means to test is the
one that runs (a retune of the dispatcher or of a cap fails loudly).  The large shapes are searched from the restated planner
at the device's CU count and assert from the query that a second trip of the grid-stride loop happens.

Buffers passed to the C entry points carry guard words on both sides; outputs are pre-filled with NaN, grad_ema_t with
non-zero values (the backward adds with atomics).  Inputs sit in exactly-sized bodies between NaN guard words: the MFMA form
reads p and grad_out with deliberately clamped addresses, and a read that leaks past an end shows as NaN in a result.

W is uniform in +-2, so every clamp region holds its share of the entries and some rows are badly conditioned (den of a
few 1e-4); the bounds carry the conditioning terms derived in _ntm_point_ref.py.  correct_logits operands have both signs, lam
is 0.9, 0 and 1, rows of exact zeros sit at the first, a middle and the last point, and one row has s = 1e-12f exactly (at
lam = 0: the `s > 1e-12` comparison itself).

Largest error / bound per family (each test prints its own figures, pytest -s), MI355X (256 CUs), 2026-10-20: sig_t_mean
forward 0.67 at the small shapes and 0.69 at the large ones (the row sums of c = 2 and 3: a bound of 3 and 4 roundings;
elements far below), d raw 0.0094 small and 0.027 large, grad_W through autograd 0.0012 below 32 768 points and 0.51 at
(3, 10931) (c = 6: 3.3e-4 of the scale against the fp32 composite's 1.6e-4; c = 5: 5.1e-5 against 3.8e-4; c = 13: 3.6e-6
against 1.6e-5 -- with W in +-2 both are the conditioning of a few rows, not the length of the sum), correct_logits out
0.0087, grad_logits 0.0096, grad_ins_T 0.013 (0.34 at c = 1, where d v is nothing but the cancellation term), grad_ema_t
0.0052 (0.024 at c = 1).  No kernel exceeded its bound.  The plans at 256 CUs:
(3, 43691) = 4097 tiles on 256 workgroups for the MFMA second tile (ksplit 2 at c = 6 and 8, 4 at c = 9 and 12), (3, 49313)
for ksplit 3, (1, 524353) on 2048 workgroups for the rows form, (1, 1025) on 256 and (3, 2731) on 2048 for the wave form,
(3, 2741) on 2048 for gen_correct_*.  Wall time of the slowest case 1.2 s (MFMA second tile, c = 12: 19 M elements against
fp64); the whole file 17 s.

With one fault planted at a time in a scratch build of csrc/ntm_generic.hip (never committed), these cases failed:
the sh == 1 rotation reading g4[i][e]: every small shape of c = 11 and 23 and four of c = 31; the gv mask dropped: c = 1, 2,
3, 5 under the forced MFMA form and the large c = 6 and c = 9 (ksplit 3) cases; the row sum's TAILS mask dropped: 106 cases,
every count with c % 4 != 0; inside taken from the clamped value: 133 of 147 small cases; the rows form's wrap applied to o
only (the mirror of `pt only`, which would move addresses past the tile): 90 cases; kk < c dropped from the wave form's
live: 77 cases (every odd c); the sg term dropped: all 60 entry-point cases; s >= 1e-12f: lam = 0 at every count (the
threshold row); each family's grid-stride loop cut to its first trip: all ten large sig_t_mean cases and the (3, 2741)
case of c = 2, 9, 32 at every lam (NaN left in the outputs).
"""
import time

import numpy as np
import pytest
import torch

import _ntm_generic_ref as G
import _ntm_point_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAMS = [0.9, 0.0, 1.0]
ZERO_SHAPE, ZERO_POINTS = (2, 1001), (0, 1001, 2001)
THRESHOLD_POINTS = (1,)                # s = 1e-12f exactly at lam = 0: not above the threshold
GUARD, SENTINEL = 64, -7.25            # 256 bytes: the body stays 16-byte aligned
CHUNK = 8192                           # points per evaluation of the fp64 reference at the large shapes
SIG_CASES = [(c, kind) for c in G.CLASS_COUNTS for kind in (("inside", "below") if c == 1 else ("random",))]
AUTOGRAD_COUNTS = [1, 5, 6, 13, 32]
AUTOGRAD_SHAPES = [(1, 1), (5, 7), (1, 33), (2, 1001)]
AUTOGRAD_LARGE = (3, 10931)            # 32 793 points: the long sums


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def guarded(shape, values=None, guard=SENTINEL):
    """A buffer between two runs of guard words: NaN-filled, or holding `values`."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), guard, dtype=torch.float32, device=DEV)
    body = whole[GUARD:GUARD + n].view(*shape)
    if values is None:
        body.fill_(float("nan"))
    else:
        body.copy_(dev(values))
    assert body.data_ptr() % 16 == 0
    return body, whole


def operand(values):
    """An input in an exactly-sized body between NaN guard words (the whole buffer is kept alive by the view)."""
    return guarded(values.shape, values, guard=float("nan"))[0]


def intact(*wholes):
    for w in wholes:
        assert bool((w[:GUARD] == SENTINEL).all()) and bool((w[-GUARD:] == SENTINEL).all()), "guard words overwritten"
        assert not bool(torch.isnan(w).any()), "NaN left in a buffer"


def note(what, c, shape, *ratios):
    print("ntm-generic-ratio | %s | c %d (%d, %d) | %s" % (what, c, shape[0], shape[1], " ".join("%.4f" % r for r in ratios)))


def call(name, *args):
    from geot_amd.ext._common import call as _call
    _call(name, torch.device(DEV), *args)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def lib():
    from geot_amd import _lib
    return _lib.load()


def use(monkeypatch, env):
    if env is None:
        monkeypatch.delenv("GEOT_NTM_GENERIC", raising=False)
    else:
        monkeypatch.setenv("GEOT_NTM_GENERIC", env)


def need_plan(monkeypatch, b, n, c, env, form, backward=0):
    """Sets the form switch and asserts, from the library's query on this device, what the next launch will be."""
    use(monkeypatch, env)
    got = G.plan(lib(), b, n, c, backward, 0)
    assert got == G.plan_ref(b, n, c, backward, cus(), env), (b, n, c, env, got)
    assert got[0] == form, (b, n, c, env, got)
    return got[1]


# ---- cases ------------------------------------------------------------------------------------------------------------------
class SigCase:
    """inputs of one (c, shape); the fp64 reference of the small shapes whole, of the large ones chunk by chunk"""

    def __init__(self, c, b, n, kind="random", whole=True):
        self.c, self.b, self.n, self.t = c, b, n, b * n
        self.p, self.cm, self.W, self.g = R.sig_inputs(b, n, c, seed=G.seed_of(c, b, n), amp=2.0)
        if c == 1:
            self.W = np.array([[[0.25, 0.5 if kind == "inside" else -0.5]]], np.float32)
        self.x = np.ascontiguousarray(self.p.transpose(0, 2, 1).reshape(self.t, c))
        self.ref = R.sig_t_mean(self.p, self.cm, self.W, self.g) if whole else None
        if whole:
            self.check_inputs(self.ref, self.t)
        self.d_p, self.d_cm, self.d_W, self.d_g = operand(self.p), operand(self.cm), operand(self.W), operand(self.g)

    def check_inputs(self, ref, pts):
        below, inside, above, edge = R.region_shares(ref)
        assert edge <= 1e-4
        if self.c > 1:
            assert ref["below"][:, R.all_low_head(self.c)].all()
            if pts >= 33:
                assert min(below, inside, above) >= 0.01, (below, inside, above)     # the inputs reach every region

    def chunks(self):
        """(lo, hi, reference) over the points"""
        if self.ref is not None:
            yield 0, self.t, self.ref
            return
        for lo in range(0, self.t, CHUNK):
            hi = min(self.t, lo + CHUNK)
            ref = R.sig_t_mean(self.x[lo:hi].T[None], self.cm, self.W, self.g[lo:hi], want_grad_W=False)
            self.check_inputs(ref, hi - lo)
            yield lo, hi, ref

    def forward(self):
        out, whole = guarded((self.t, self.c, self.c))
        call("geot_ntm_sig_t_mean", self.b, self.n, self.c, self.d_p.data_ptr(), self.d_W.data_ptr(), self.d_cm.data_ptr(), out.data_ptr())
        intact(whole)
        return out

    def grad_raw(self):
        draw, whole = guarded((self.t, self.c, self.c))
        call("geot_ntm_sig_t_mean_grad_raw", self.b, self.n, self.c, self.d_p.data_ptr(), self.d_W.data_ptr(), self.d_cm.data_ptr(),
             self.d_g.data_ptr(), draw.data_ptr())
        intact(whole)
        return draw

    def ratios(self, out, draw):
        """(forward, d raw) ratios of two results, every element, and the exact statements about d raw"""
        out, draw = host(out), host(draw)
        r_f = r_d = 0.0
        head = R.all_low_head(self.c)
        for lo, hi, ref in self.chunks():
            r_f = max(r_f, R.sig_forward_ratio(out[lo:hi], ref))
            got = draw[lo:hi]
            r_d = max(r_d, R.draw_ratio(got, ref))                    # non-edge entries; an exact zero outside the clamp
            assert not got[(ref["above"] | ref["below"]) & ~ref["edge"]].any()
            if self.c > 1:
                assert not got[:, head].any()
            e = ref["edge"]                                           # an edge entry is one of the two legitimate values
            if e.any():
                on = (self.g[lo:hi].astype(np.float64) - (self.g[lo:hi] * ref["out"]).sum(2, keepdims=True)) / ref["den"]
                assert np.all((got[e] == 0) | (np.abs(got[e] - on[e]) <= ref["draw_bound"][e]))
        return r_f, r_d

    def module(self):
        from geot_amd import ntm
        mod = ntm.sig_t_mean(self.c).to(DEV)
        with torch.no_grad():
            for kk, l in enumerate(mod.fc):
                l.weight.copy_(self.d_W[kk])
        return mod


class CorrectCase:
    def __init__(self, c, b, n, zero=()):
        self.c, self.b, self.n, self.t = c, b, n, b * n
        self.logits, self.insT, self.E, self.g = R.correct_inputs(b, n, c, zero_points=zero, threshold_points=THRESHOLD_POINTS if zero else ())
        self.d_l, self.d_T, self.d_E, self.d_g = operand(self.logits), operand(self.insT), operand(self.E), operand(self.g)
        self.blocks = G.gen_blocks(self.t)
        self.groups = (np.arange(self.t) % (4 * self.blocks)) // 4      # the workgroup a point's wave belongs to
        self._refs = {}

    def ref(self, lam):
        if lam not in self._refs:
            r = R.correct_logits(self.logits, self.insT, self.E, lam, self.g, groups=self.groups)
            assert not r["live"].any() or r["s"][r["live"]].min() > 1e-3                # well conditioned
            assert (self.insT < 0).any() and (self.insT > 0).any() or self.t * self.c < 4
            self._refs[lam] = r
        return self._refs[lam]


_cases = {}


def sig_case(c, b, n, kind="random"):
    key = ("sig", c, b, n, kind)
    if key not in _cases:
        _cases[key] = SigCase(c, b, n, kind)
    return _cases[key]


# ---- sig_t_mean, small shapes: every form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,n", G.SMALL_SHAPES)
@pytest.mark.parametrize("c,kind", SIG_CASES)
def test_sig_t_mean_every_form_at_the_small_shapes(c, kind, b, n, monkeypatch):
    case = sig_case(c, b, n, kind)
    ref = case.ref
    if c == 1:
        assert ref[kind].all()
    results = {}
    for env, _ in G.forms_of(c):
        form = G.small_form(b, n, c, env)
        need_plan(monkeypatch, b, n, c, env, form)
        out = case.forward()
        need_plan(monkeypatch, b, n, c, env, form, backward=1)
        draw = case.grad_raw()
        r_f, r_d = case.ratios(out, draw)
        note("sig_t_mean %s (form %d): forward, d raw" % (env or "default", form), c, (b, n), r_f, r_d)
        assert max(r_f, r_d) <= 1.0
        results[env] = (host(out).astype(np.float64), host(draw).astype(np.float64))
    # the same operation under two forms, held to each other at the bound
    ne = ~ref["edge"]
    envs = list(results)
    for i, a in enumerate(envs):
        for b_ in envs[i + 1:]:
            r_f = R.worst(np.abs(results[a][0] - results[b_][0]), R.sig_forward_bound(ref))
            r_d = R.worst(np.abs(results[a][1] - results[b_][1])[ne], (ref["draw_bound"] * ref["inside"])[ne])
            assert max(r_f, r_d) <= 1.0, (a, b_, r_f, r_d)


@pytest.mark.parametrize("pts", [1, 2, 3])
def test_forced_mfma_with_fewer_than_four_output_elements_runs_the_rows_form(pts, monkeypatch):
    """c = 1, 1..3 points: the MFMA kernel clamps its gradient loads to the buffer's last four elements and needs four"""
    case = SigCase(1, 1, pts, "inside")
    need_plan(monkeypatch, 1, pts, 1, "mfma", G.ROWS, backward=1)
    r_f, r_d = case.ratios(case.forward(), case.grad_raw())
    note("sig_t_mean mfma -> rows: forward, d raw", 1, (1, pts), r_f, r_d)
    assert max(r_f, r_d) <= 1.0
    need_plan(monkeypatch, 1, 4, 1, "mfma", G.MFMA, backward=1)


# ---- sig_t_mean, large shapes: the second trips -----------------------------------------------------------------------------------
def large_cases():
    return ([("mfma second tile", c) for c in (6, 8, 9, 12)] + [("mfma ksplit 3", 9)] + [("rows second trip", c) for c in (2, 3)]
            + [("wave second trip", c) for c in (32, 3, 9)])


@pytest.mark.parametrize("what,c", large_cases())
def test_sig_t_mean_at_the_large_shapes(what, c, monkeypatch):
    t0 = time.time()
    n_cu = cus()
    if what == "mfma second tile":
        (b, n), env, form = G.large_mfma_second_tile(c, n_cu), None, G.MFMA
    elif what == "mfma ksplit 3":
        shape = G.large_mfma_ksplit3(c, n_cu)
        assert shape is not None, "the planner picks ksplit = 3 at no shape on %d CUs" % n_cu
        (b, n), env, form = shape, None, G.MFMA
    elif what == "rows second trip":
        (b, n), env, form = G.large_rows_second_trip(c, n_cu), None, G.ROWS
    else:
        (b, n), env, form = G.large_wave_second_trip(c, n_cu, b=1 if c == 32 else 3), "wave", G.WAVE
    pts = b * n
    p = need_plan(monkeypatch, b, n, c, env, form)
    assert need_plan(monkeypatch, b, n, c, env, form, backward=1) == p
    # from the query: a second trip happens on this device, and the last tile is partial
    if form == G.MFMA:
        tiles, nb = (pts + 31) // 32, p["blocks"] // p["ksplit"]
        assert tiles > nb * G.GEN_MW and pts % 32
        if what == "mfma ksplit 3":
            assert p["ksplit"] == 3 and G.mfma_geometry(c)[2] % 3
        elif c in (6, 8):
            assert p["ksplit"] == G.mfma_geometry(c)[2] == 2
    elif form == G.ROWS:
        assert pts > p["blocks"] * 256 and pts % 64
    else:
        assert pts > p["blocks"] * 4 and pts % 4
        assert c != 32 or p["lds"] > 64 * 1024                        # the launch that asks for more than 64 KB
    assert pts * c * c * 4 <= 96 << 20
    case = SigCase(c, b, n, whole=False)
    r_f, r_d = case.ratios(case.forward(), case.grad_raw())
    note("sig_t_mean %s, %d blocks, ksplit %d: forward, d raw" % (what, p["blocks"], p["ksplit"]), c, (b, n), r_f, r_d)
    print("ntm-generic-time | %s c %d | %.2f s" % (what, c, time.time() - t0))
    assert max(r_f, r_d) <= 1.0


# ---- correct_logits -------------------------------------------------------------------------------------------------------------
def correct_shapes(c):
    shapes = [(s, ()) for s in G.SMALL_SHAPES] + [(ZERO_SHAPE, ZERO_POINTS)]
    if c in (2, 9, 32):
        shapes.append((G.CORRECT_LARGE, ()))
    return shapes


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("c", G.CLASS_COUNTS)
def test_correct_logits_entry_points(c, lam, monkeypatch):
    """geot_ntm_correct, geot_ntm_correct_grad into a non-zero grad_ema_t (base + sum, any order of the workgroups' atomics),
    and geot_ntm_correct_grad_ws, which forwards to it at c != 17 and leaves the workspace alone."""
    worst = np.zeros(4)
    for (b, n), zero in correct_shapes(c):
        case = CorrectCase(c, b, n, zero)
        ref = case.ref(lam)
        p = need_plan(monkeypatch, b, n, c, None, G.MFMA if c >= 6 else G.ROWS)
        assert p["correct_blocks"] == case.blocks
        if (b, n) == G.CORRECT_LARGE:
            assert case.t > 4 * p["correct_blocks"] and case.t % 4        # the grid-stride loop's second trip, from the query
        dead = ~ref["live"]
        if zero:
            assert dead[list(zero + THRESHOLD_POINTS), R.zero_row(c)].all() and dead.sum() == (case.t if lam == 1.0 else 4) and zero[-1] == case.t - 1
            assert lam != 0.0 or np.float32(ref["s"][1, R.zero_row(c)]) == np.float32(1e-12)
        else:
            assert not dead.any()
        ins = (case.d_l.data_ptr(), case.d_T.data_ptr(), case.d_E.data_ptr())
        out, whole = guarded((b, c, n))
        call("geot_ntm_correct", b, n, c, lam, *ins, out.data_ptr())
        intact(whole)
        r_out = R.correct_forward_ratio(host(out), ref)
        base = np.random.default_rng(12).standard_normal((c, c)).astype(np.float32)

        def backward(ws_form):
            gl, w1 = guarded((b, c, n))
            gi, w2 = guarded((case.t, c, c))
            gE, w3 = guarded((c, c), base)
            ws, _ = guarded((c * c * case.blocks,))
            if ws_form:
                call("geot_ntm_correct_grad_ws", b, n, c, lam, *ins, case.d_g.data_ptr(), gl.data_ptr(), gi.data_ptr(), gE.data_ptr(),
                     ws.data_ptr())
            else:
                call("geot_ntm_correct_grad", b, n, c, lam, *ins, case.d_g.data_ptr(), gl.data_ptr(), gi.data_ptr(), gE.data_ptr())
            assert bool(torch.isnan(ws).all())                            # untouched
            intact(w1, w2, w3)
            ratios = R.correct_grads_ratio(host(gl), host(gi), host(gE), ref, case.t, base_E=base, atomic_adds=case.blocks)
            assert max(ratios) <= 1.0, (b, n, zero, ratios)
            return gl, gi, gE, ratios

        gl, gi, gE, ratios = backward(False)
        gl2, gi2, gE2, _ = backward(True)
        assert torch.equal(gl, gl2) and torch.equal(gi, gi2)              # the same kernel; grad_ema_t's atomics arrive in any order
        if case.blocks == 1:
            assert torch.equal(gE, gE2)
        if lam == 0.0:
            assert np.array_equal(host(gE), base + np.float32(0))
        if lam == 1.0:
            assert not bool(gi.any())
        if zero and lam != 1.0:
            assert np.abs(host(gi)[list(zero), R.zero_row(c)]).min() > 1e6 or c == 1   # the huge values are there
            assert bool(torch.isfinite(gi).all()) and bool(torch.isfinite(gE).all())
        assert r_out <= 1.0, (b, n, zero, r_out)
        worst = np.maximum(worst, (r_out,) + ratios)
    note("correct_logits lam %.1f: out, grad_logits, grad_ins_T, grad_ema_t (worst of %d shapes)" % (lam, len(correct_shapes(c))), c,
         (0, 0), *worst)


# ---- through autograd -------------------------------------------------------------------------------------------------------------
# the long sums at c = 5, 6, 13 (c = 1: grad_W is zero up to roundings, nothing to scale a bound by; c = 32: the fp64 reference
# of 32 793 points with its weight-shaped sums takes 4 GB)
@pytest.mark.parametrize("c,b,n", [(c,) + s for c in AUTOGRAD_COUNTS for s in AUTOGRAD_SHAPES] + [(c,) + AUTOGRAD_LARGE for c in (5, 6, 13)])
def test_sig_t_mean_through_autograd(c, b, n, monkeypatch):
    """The module's forward is the entry point's; grad_W comes from d raw and the torch.mm of _SigTMeanFn.backward."""
    use(monkeypatch, None)
    key = ("auto", c, b, n)
    if key not in _cases:
        _cases[key] = SigCase(c, b, n, "inside")
    case = _cases[key]
    mod = case.module()
    out = mod(case.d_p, case.d_cm)
    assert torch.equal(out.detach(), case.forward())
    (out * case.d_g).sum().backward()
    got = host(torch.stack([l.weight.grad for l in mod.fc]))
    large_tol = None
    if case.t >= R.LARGE_PTS:
        # another summation tree than the composite's: 4 x the fp32 composite's own error against fp64, on the same inputs
        gW = R.composite_sig_grad_W(case.p, case.cm, case.W, case.g)[2]
        comp = np.maximum(np.abs(gW - case.ref["grad_W"]) - case.ref["grad_W_edge"], 0).max() / np.abs(case.ref["grad_W"]).max()
        mine = np.maximum(np.abs(got - case.ref["grad_W"]) - case.ref["grad_W_edge"], 0).max() / np.abs(case.ref["grad_W"]).max()
        print("ntm-generic-long-sum | grad_W c %d (%d, %d) | composite %.3e kernel %.3e of the scale" % (c, b, n, comp, mine))
        large_tol = 4 * comp
    ratio = R.grad_W_ratio(got, case.ref, case.t, large_tol=large_tol)
    note("grad_W through autograd", c, (b, n), ratio)
    assert ratio <= 1.0
    if c > 1:
        assert not got[R.all_low_head(c)].any()


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("c", AUTOGRAD_COUNTS)
def test_correct_logits_through_autograd(c, lam):
    from geot_amd import ntm
    for (b, n), zero in [(s, ()) for s in AUTOGRAD_SHAPES] + [(ZERO_SHAPE, ZERO_POINTS)]:
        case = CorrectCase(c, b, n, zero)
        ref = case.ref(lam)
        tl, ti, tE = (t.clone().requires_grad_(True) for t in (case.d_l, case.d_T, case.d_E))
        out = ntm.correct_logits(tl, ti, tE, lam)
        r_out = R.correct_forward_ratio(host(out), ref)
        (out * case.d_g).sum().backward()
        ratios = R.correct_grads_ratio(host(tl.grad), host(ti.grad), host(tE.grad), ref, case.t, atomic_adds=case.blocks)
        note("correct_logits through autograd lam %.1f%s: out, grad_logits, grad_ins_T, grad_ema_t" % (lam, " zero rows" if zero else ""),
             c, (b, n), r_out, *ratios)
        assert max((r_out,) + ratios) <= 1.0
        if lam == 0.0:
            assert not bool(tE.grad.any())
        if lam == 1.0:
            assert not bool(ti.grad.any())


# ---- arguments --------------------------------------------------------------------------------------------------------------------
def test_arguments(monkeypatch):
    use(monkeypatch, None)
    case = SigCase(2, 1, 5)
    cor = CorrectCase(2, 1, 5)
    out, whole = guarded((5, 2, 2))
    for c in (0, 33, -1):
        for name, args in (("geot_ntm_sig_t_mean", (case.d_p.data_ptr(), case.d_W.data_ptr(), case.d_cm.data_ptr(), out.data_ptr())),
                           ("geot_ntm_sig_t_mean_grad_raw", (case.d_p.data_ptr(), case.d_W.data_ptr(), case.d_cm.data_ptr(), case.d_g.data_ptr(),
                                                             out.data_ptr()))):
            with pytest.raises(RuntimeError, match="invalid"):
                call(name, 1, 5, c, *args)
        with pytest.raises(RuntimeError, match="invalid"):
            call("geot_ntm_correct", 1, 5, c, 0.9, cor.d_l.data_ptr(), cor.d_T.data_ptr(), cor.d_E.data_ptr(), out.data_ptr())
        with pytest.raises(RuntimeError, match="invalid"):
            call("geot_ntm_correct_grad", 1, 5, c, 0.9, cor.d_l.data_ptr(), cor.d_T.data_ptr(), cor.d_E.data_ptr(), cor.d_g.data_ptr(),
                 out.data_ptr(), out.data_ptr(), out.data_ptr())
        assert G.plan(lib(), 1, 5, c, 0, 0) == (0, None)
    # b * n = 0: success, nothing touched
    for b, n in ((0, 5), (5, 0)):
        call("geot_ntm_sig_t_mean", b, n, 2, case.d_p.data_ptr(), case.d_W.data_ptr(), case.d_cm.data_ptr(), out.data_ptr())
        call("geot_ntm_sig_t_mean_grad_raw", b, n, 2, case.d_p.data_ptr(), case.d_W.data_ptr(), case.d_cm.data_ptr(), case.d_g.data_ptr(),
             out.data_ptr())
        call("geot_ntm_correct", b, n, 2, 0.9, cor.d_l.data_ptr(), cor.d_T.data_ptr(), cor.d_E.data_ptr(), out.data_ptr())
        call("geot_ntm_correct_grad", b, n, 2, 0.9, cor.d_l.data_ptr(), cor.d_T.data_ptr(), cor.d_E.data_ptr(), cor.d_g.data_ptr(),
             out.data_ptr(), out.data_ptr(), out.data_ptr())
        assert G.plan(lib(), b, n, 2, 0, 0) == (0, None)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())
