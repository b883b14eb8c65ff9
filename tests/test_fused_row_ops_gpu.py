"""The small autograd ops of geot_amd/fused_norm.py on both sides of every dispatch switch of their kernels, against fp64.

Kernels: csrc/bnrelu.hip (segment_max / _grad, segment_sum, bn_pool / _grad, rowdot_small, colsum, rowsum_f64, the
BatchNorm passes) and csrc/layernorm.hip (res_ln / _grad, qkv_split / _grad, softmax_grad).  Each case asserts the entry
points it launched, so a shape that falls back to torch cannot pass as a kernel test.

Tolerances:
  * exact ops (max and its one-hot gradient, the head split, copies) must be bit-equal;
  * sums are bounded by gamma_k * sum|terms| (tests/_fused_ref.py), k the depth of the kernel's summation tree -- the
    roundings one term can meet -- read off the kernel's loop structure; integer-valued inputs whose partial sums all fit
    in 24 bits must come out exact in any order, which catches a dropped or doubled element regardless of its size;
  * normalisations (BatchNorm, LayerNorm, soft-max) keep the rules of their tests in tests/test_model_gpu.py.
Storage at a 4-, 8- and 12-byte offset, for inputs and for the gradients a backward receives, must give the aligned result."""
import math
import zlib

import pytest
import torch

from _fused_ref import Launches, at_offset, backward_at_offset, first_argmax, gamma

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NS = (4, 8, 12, 16, 28, 32, 36, 252, 256)    # lanes per row 1 | 2, 2 | 4, 4 | 8, 8, 8, 8: both ends of every LPR band
ROW_SHAPES = ((1,), (31,), (257,), (3, 1000), (2, 3, 5))   # partial last blocks; ranks 2, 3 and 4 with the n axis
GRID_CAP4 = 65536 * 256                      # float4s the capped grids of segment_max_grad / bn_pool_grad cover in one sweep


@pytest.fixture
def launches(monkeypatch):
    return Launches(monkeypatch)


@pytest.fixture(scope="module")
def lib():
    from geot_amd import _lib
    return _lib.load()


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _bits(t):
    return t.detach().float().cpu().contiguous().view(torch.int32)


def _assert_rule(name, ref, got, rel, atol=0.0):
    """|got - ref| <= rel * max|ref| + atol (the normalisation rules of tests/test_model_gpu.py)"""
    ref = torch.zeros(()) if ref is None else ref.detach().double().cpu()
    got = torch.zeros(()) if got is None else got.detach().double().cpu()
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((ref - got).abs().max()) if ref.numel() else 0.0
    assert err <= rel * scale + atol, (name, err, scale)


def _assert_sum_bound(got, ref64, abs64, k):
    """fp32 sums of depth k against their fp64 value: |got - ref| <= gamma_k * sum|terms| + the final rounding"""
    got, ref64, abs64 = got.double().cpu(), ref64.double().cpu(), abs64.double().cpu()
    bound = gamma(k) * abs64 + 2.0 ** -24 * ref64.abs()
    excess = (got - ref64).abs() - bound
    assert float(excess.max()) <= 0.0, (k, float((got - ref64).abs().max()), float(bound.max()))


# ---- max_last: geot_segment_max / _grad ---------------------------------------------------------------------------------
def _planted(rows, n, gen):
    """(rows, n) float32, row r of kind r % 10: random; a tie inside one float4; a tie across adjacent float4s (adjacent
    lanes when LPR > 1); a tie at slots 0 and n-1; a lone maximum at n-1; -0.0 before +0.0 and the reverse as the maxima;
    all -inf; NaNs (two, after a +inf); -inf but one finite slot"""
    x = torch.randn(rows, n, generator=gen)
    big = x.abs().amax(-1) + 1.0
    v4 = n // 4
    for r in range(min(rows, 10 * 40)):         # the kinds repeat; 40 of each are plenty, the rest stay random
        kind, s = r % 10, r // 10
        if kind == 1:
            j = 4 * (s % v4) + 1
            x[r, j] = x[r, j + 1] = big[r]
        elif kind == 2:
            if v4 > 1:
                j = 4 * (s % (v4 - 1)) + 3
                x[r, j] = x[r, j + 1] = big[r]
            else:
                x[r, 0] = x[r, 3] = big[r]
        elif kind == 3:
            x[r, 0] = x[r, n - 1] = big[r]
        elif kind == 4:
            x[r, n - 1] = big[r]
        elif kind in (5, 6):
            x[r] = -x[r].abs() - 1.0
            j, j2 = s % (n // 2), n // 2 + (s * 7) % (n // 2)
            x[r, j], x[r, j2] = (-0.0, 0.0) if kind == 5 else (0.0, -0.0)
        elif kind == 7:
            x[r] = -math.inf
        elif kind == 8:
            x[r, 0] = math.inf
            x[r, 1 + s % (n - 1)] = math.nan
            x[r, n - 1] = math.nan
        elif kind == 9:
            x[r] = -math.inf
            x[r, (s * 5) % n] = 1.5
    return x


def check_max_last(shape, launches, seed=0):
    from geot_amd.fused_norm import max_last
    n = shape[-1]
    gen = _gen("max", shape, seed)
    rows = math.prod(shape[:-1])
    x0 = _planted(rows, n, gen).view(shape)
    up = torch.randn(shape[:-1], generator=gen)
    x = x0.to(DEV, copy=True).requires_grad_(True)
    y = max_last(x)
    (y * up.to(DEV)).sum().backward()
    assert launches.take() == ["geot_segment_max", "geot_segment_max_grad"], shape
    idx = first_argmax(x0)
    want = x0.gather(-1, idx.unsqueeze(-1)).squeeze(-1)
    assert torch.equal(_bits(y), want.view(torch.int32)), shape              # the element itself: sign of zero, NaN
    torch.testing.assert_close(y.detach().cpu(), x0.max(dim=-1)[0], rtol=0, atol=0, equal_nan=True)
    want_dx = torch.zeros(shape).scatter_(-1, idx.unsqueeze(-1), up.unsqueeze(-1))
    assert torch.equal(x.grad.cpu(), want_dx), shape                          # one-hot at the first maximum


@pytest.mark.parametrize("rows", ROW_SHAPES)
@pytest.mark.parametrize("n", NS)
def test_max_last_every_lane_count(n, rows, launches):
    check_max_last(rows + (n,), launches)


def test_max_last_grad_past_the_grid_cap(launches):
    """rows * n / 4 > 65536 * 256: the capped gradient grid strides; n = 256 puts the maximum at every slot up to 255"""
    from geot_amd.fused_norm import max_last
    n, rows = 256, GRID_CAP4 // 64 + 3001
    assert rows * n // 4 > GRID_CAP4
    r = torch.arange(rows, device=DEV).view(-1, 1)
    j = torch.arange(n, device=DEV).view(1, -1)
    x = ((j * 37 + r) % n).float().requires_grad_(True)     # a permutation of 0..255 per row: no ties, torch's index is unique
    up = torch.randn(rows, device=DEV)
    y = max_last(x)
    (y * up).sum().backward()
    assert launches.take() == ["geot_segment_max", "geot_segment_max_grad"]
    xr = x.detach().clone().requires_grad_(True)
    yr = xr.max(dim=-1)[0]
    (yr * up).sum().backward()
    assert torch.equal(y.detach(), yr.detach())
    assert torch.equal(x.grad, xr.grad)
    del x, xr, y, yr
    torch.cuda.empty_cache()


# ---- add_last_broadcast: geot_segment_sum ----------------------------------------------------------------------------------
def check_add_last_broadcast(shape, launches, seed=0):
    from geot_amd.fused_norm import add_last_broadcast
    n = shape[-1]
    gen = _gen("alb", shape, seed)
    a0, p0 = torch.randn(shape, generator=gen), torch.randn(shape[:-1], generator=gen)
    up_r = torch.randn(shape, generator=gen).view(-1, n)
    half = up_r[::3, : n // 2]                           # every third row cancels: (h, -h) in a shuffled order
    up_r[::3] = torch.cat([half, -half], 1)[:, torch.randperm(n, generator=gen)]
    up_i = torch.randint(-8, 9, shape, generator=gen).float()                     # |partial sums| < 2^24: exact
    for up, exact in ((up_r.view(shape), False), (up_i, True)):
        a, p = a0.to(DEV, copy=True).requires_grad_(True), p0.to(DEV, copy=True).requires_grad_(True)
        y = add_last_broadcast(a, p)
        (y * up.to(DEV)).sum().backward()
        assert launches.take() == ["geot_segment_sum"], shape
        assert torch.equal(y.detach().cpu(), a0 + p0.unsqueeze(-1)) and torch.equal(a.grad.cpu(), up)
        want = up.double().sum(-1)
        if exact:
            assert torch.equal(p.grad.double().cpu(), want), shape
        else:    # lane sub-sums, then a butterfly over the LPR lanes: each element meets at most n - 1 additions
            _assert_sum_bound(p.grad, want, up.double().abs().sum(-1), n - 1)


@pytest.mark.parametrize("rows", ((1,), (257,), (3, 1000)))
@pytest.mark.parametrize("n", NS)
def test_add_last_broadcast_every_lane_count(n, rows, launches):
    check_add_last_broadcast(rows + (n,), launches)


# ---- bn_relu_max: geot_bn_pool / _grad ----------------------------------------------------------------------------------
def _bn_pair(c, gen, gammas=None):
    ours = torch.nn.BatchNorm1d(c)
    with torch.no_grad():
        ours.weight.copy_(gammas if gammas is not None else torch.randn(c, generator=gen))
        ours.bias.copy_(torch.randn(c, generator=gen))
        ours.running_mean.uniform_(-0.5, 0.5, generator=gen)
        ours.running_var.uniform_(0.5, 2.0, generator=gen)
    ref = torch.nn.BatchNorm1d(c).double()
    ref.load_state_dict(ours.state_dict())
    return ref, ours


def check_bn_relu_max(b, c, groups, n, launches, y0=None, gammas=None, ref_dev="cpu", seed=0):
    """vs fp64 BatchNorm -> ReLU -> max over the last n (torch.max: the first extremum), at the rule of
    test_bn_relu_max_equals_batchnorm_relu_maxpool (3e-5 of the largest reference value + 1e-6)"""
    from geot_amd.fused_norm import bn_relu_max
    gen = _gen("bnpool", b, c, groups, n, seed)
    if y0 is None:
        y0 = torch.randn(b, c, groups, n, generator=gen) * 2 + 0.3
        # ties at the extremum the kernel picks: the maximum copied one slot on (wrapping to slot 0), the minimum half a row on
        imax, imin = y0.argmax(-1, keepdim=True), y0.argmin(-1, keepdim=True)
        tie_max = y0.gather(-1, imax).expand_as(y0).clone()
        tie_min = y0.gather(-1, imin).expand_as(y0).clone()
        sel = torch.arange(groups) % 3
        y0[:, :, sel == 0] = y0[:, :, sel == 0].scatter(-1, (imax[:, :, sel == 0] + 1) % n, tie_max[:, :, sel == 0])
        y0[:, :, sel == 1] = y0[:, :, sel == 1].scatter(-1, (imin[:, :, sel == 1] + n // 2) % n, tie_min[:, :, sel == 1])
        y0 = y0.reshape(b, c, groups * n)
    if gammas is None:                                      # > 0, < 0 and == 0 on different channels
        gammas = torch.tensor([0.8, -1.3, 0.0, 1.1, -0.4, 0.0, 2.0, -2.0][:c] + [0.5] * max(0, c - 8))
    ref, ours = _bn_pair(c, gen, gammas)
    with torch.no_grad():                                   # gamma == 0: out = relu(beta), a tie over the whole row
        ours.bias[gammas == 0] = torch.tensor([0.7, -0.2, 0.3, 0.1][: int((gammas == 0).sum())])
        ref.bias.copy_(ours.bias)
    up = torch.randn(b, c, groups, generator=gen)
    ref.to(ref_dev); ours.to(DEV)
    res = []
    for mod, fused in ((ref, False), (ours, True)):
        dev = DEV if fused else torch.device(ref_dev)
        y = (y0.to(dev) if fused else y0.to(dev).double()).requires_grad_(True)
        out = bn_relu_max(mod, y, n) if fused else torch.relu(mod(y)).view(b, c, groups, n).max(-1)[0]
        (out * up.to(dev, out.dtype)).sum().backward()
        res.append([t.detach() for t in (out, y.grad, mod.weight.grad, mod.bias.grad, mod.running_mean, mod.running_var)])
        del y, out
    assert launches.take()[-2:] == ["geot_bn_pool", "geot_bn_pool_grad"], (b, c, groups, n)
    for name, a, f in zip(("out", "dy", "dgamma", "dbeta", "running_mean", "running_var"), *res):
        _assert_rule(name, a, f, 3e-5, 1e-6)


@pytest.mark.parametrize("n", NS)
def test_bn_relu_max_every_lane_count(n, launches):
    check_bn_relu_max(2, 6, 13, n, launches)


def test_bn_relu_max_grad_past_the_grid_cap(launches):
    """b * c * groups * n / 4 > 65536 * 256: the capped backward grid strides.  Every group holds distinct values (a
    permutation of 32 levels plus a per-group offset), so the GPU reference's arg-max is unique."""
    b, c, n = 1, 8, 32
    groups = GRID_CAP4 // (c * n // 4) + 1001
    gen = _gen("bnpool-cap")
    j = torch.arange(n).view(1, 1, n)
    gi = torch.arange(groups).view(1, groups, 1)
    y0 = torch.empty(b, c, groups, n)
    for ch in range(c):
        off = torch.randn(1, groups, 1, generator=gen) * 0.5
        y0[0, ch] = (((j * 13 + gi + 5 * ch) % n).float() * 0.1 + off)[0]
    y0 = y0.view(b, c, groups * n)
    check_bn_relu_max(b, c, groups, n, launches, y0=y0, gammas=torch.tensor([0.8, -1.3, 1.1, -0.4, 2.0, -2.0, 0.3, -0.9]),
                      ref_dev="cuda")
    torch.cuda.empty_cache()


# ---- thin_mm: geot_rowdot_small ----------------------------------------------------------------------------------------
THIN_SHAPES = (          # (C, l): slices 64 (the cap, just past 63 * 2048), 17, 1, 2 (just past one slice), l < 4, l % 4 != 0, C = 1, C = 65535
    (8, 63 * 2048 + 1), (8, 16 * 2048 + 1), (8, 2048), (8, 2049), (5, 3), (5, 1), (37, 4099), (1, 5001), (65535, 6))


@pytest.mark.parametrize("c,l", THIN_SHAPES)
@pytest.mark.parametrize("j", range(1, 9))
def test_thin_mm_weight_gradient_every_j_and_slice_count(j, c, l, lib, launches):
    if (c, l) == THIN_SHAPES[0]:
        assert lib.geot_rowdot_small_slices(c, l) == 64
    check_thin_mm(j, c, l, lib, launches)


def check_thin_mm(j, c, l, lib, launches):
    from geot_amd.fused_norm import thin_mm
    s = int(lib.geot_rowdot_small_slices(c, l))
    per = ((l + s - 1) // s + 3) & ~3
    # an element's product meets ceil(per / 256) fmas in its thread, 6 + 2 block additions, <= s - 1 in the slice sum
    depth = -(-per // 256) + 8 + s
    gen = _gen("thin", j, c, l)
    w0 = torch.randn(c, j, generator=gen)
    for exact in (False, True):
        if exact:   # |products| <= 9, l * 9 < 2^24: every partial sum is an integer the fp32 format holds
            x0, up = torch.randint(-3, 4, (j, l), generator=gen).float(), torch.randint(-3, 4, (c, l), generator=gen).float()
        else:
            x0, up = torch.randn(j, l, generator=gen), torch.randn(c, l, generator=gen)
        w = w0.to(DEV, copy=True).requires_grad_(True)
        x = x0.to(DEV, copy=True).requires_grad_(True)
        y = thin_mm(w, x)
        (y * up.to(DEV)).sum().backward()
        assert launches.take() == ["geot_rowdot_small"]
        assert torch.equal(y.detach(), torch.mm(w0.to(DEV), x0.to(DEV)))
        assert torch.equal(x.grad, torch.mm(w0.to(DEV).t(), up.to(DEV)))
        want = up.double() @ x0.double().t()
        if exact:
            assert torch.equal(w.grad.double().cpu(), want)
        else:
            _assert_sum_bound(w.grad, want, up.double().abs() @ x0.double().abs().t(), depth)


# ---- linear: geot_colsum ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", (1, 63, 64, 65, 1536))
@pytest.mark.parametrize("shape", ((1,), (3,), (31,), (32,), (33,), (4096 + 5,), (2, 50)))
def test_linear_bias_gradient_every_slice_count(shape, cols, lib, launches):
    if shape == (4101,) and cols <= 1024:
        assert lib.geot_colsum_ws_floats(4101, cols) == 16 * cols      # the most slices the finish pass reads
    check_linear(shape, 8, cols, lib, launches)


def check_linear(shape, cin, cols, lib, launches):
    from geot_amd.fused_norm import linear
    rows = math.prod(shape)
    s = int(lib.geot_colsum_ws_floats(rows, cols)) // cols
    per = -(-rows // s)
    depth = -(-per // 4) + 2 + s      # a wave's rows of the slice one after the other, 2 block additions, s in the finish
    gen = _gen("colsum", shape, cols)
    lin = torch.nn.Linear(cin, cols).to(DEV)
    x0 = torch.randn(*shape, cin, generator=gen).to(DEV)
    for exact in (False, True):
        up = (torch.randint(-8, 9, (*shape, cols), generator=gen).float() if exact else torch.randn(*shape, cols, generator=gen))
        lin.zero_grad()
        y = linear(lin, x0)
        (y * up.to(DEV)).sum().backward()
        assert launches.take() == ["geot_colsum"]
        want = up.double().reshape(-1, cols).sum(0)
        if exact:
            assert torch.equal(lin.bias.grad.double().cpu(), want)
        else:
            _assert_sum_bound(lin.bias.grad, want, up.double().abs().reshape(-1, cols).sum(0), depth)


# ---- add_channel_bias: geot_rowsum_f64 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("l", (1, 255, 256, 257, 100000))
@pytest.mark.parametrize("lead", ((5,), (3, 4)))
def test_add_channel_bias_every_row_length(lead, l, launches):
    from geot_amd.fused_norm import add_channel_bias
    c = lead[-1]
    gen = _gen("acb", lead, l)
    y0, b0 = torch.randn(*lead, l, generator=gen), torch.randn(c, generator=gen)
    for exact in (False, True):
        up = torch.randint(-8, 9, (*lead, l), generator=gen).float() if exact else torch.randn(*lead, l, generator=gen)
        y, bias = y0.to(DEV, copy=True).requires_grad_(True), b0.to(DEV, copy=True).requires_grad_(True)
        out = add_channel_bias(y, bias)
        (out * up.to(DEV)).sum().backward()
        assert launches.take() == ["geot_rowsum_f64"]
        assert torch.equal(out.detach().cpu(), y0 + b0.view(-1, 1)) and torch.equal(y.grad.cpu(), up)
        dims = (0, 2) if len(lead) == 2 else (1,)
        want = up.double().sum(dims)
        if exact:
            assert torch.equal(bias.grad.double().cpu(), want)
        else:   # fp64 sums (depth <= l + b, unit 2^-53), then one rounding to fp32
            got = bias.grad.double().cpu()
            bound = 2.0 ** -24 * want.abs() + 2.0 ** -52 * (l + 8) * up.double().abs().sum(dims)
            assert bool(((got - want).abs() <= bound).all())


# ---- res_ln: geot_res_ln / _grad ----------------------------------------------------------------------------------------
def check_res_ln(b, n, c, use_y, use_s, use_e, use, launches, seed=0):
    """vs the torch composition in fp64 at the rule of test_res_ln_equals_add_then_layernorm (2e-5 of the largest reference
    value); use: which outputs the loss reads -- "t" (gz NULL), "z" (gt NULL) or "both" """
    from geot_amd.fused_norm import res_ln
    gen = _gen("resln", b, n, c, use_y, use_s, use_e, use, seed)
    x0, y0, e0 = (torch.randn(b, n, c, generator=gen) for _ in range(3))
    s0 = torch.tensor([0.0, 1.0 / 0.7, 1.3, 0.5])[torch.arange(b) % 4].view(b, 1, 1)   # per sample; a dropped one included
    up_t, up_z = torch.randn(b, n, c, generator=gen), torch.randn(b, n, c, generator=gen)
    res = []
    for fused in (False, True):
        dt = torch.float32 if fused else torch.float64
        ln = torch.nn.LayerNorm(c).to(DEV).to(dt)
        with torch.no_grad():
            ln.weight.copy_(torch.linspace(0.5, 1.5, c)); ln.bias.copy_(torch.linspace(-1, 1, c))
        x = x0.to(DEV, dt).requires_grad_(True)
        y = y0.to(DEV, dt).requires_grad_(True) if use_y else None
        e = e0.to(DEV, dt).requires_grad_(True) if use_e else None
        s = s0.to(DEV, dt) if use_s else None
        if fused:
            t, z = res_ln(x, y, s, e, ln)
        else:
            t = x
            if y is not None:
                t = t + (y if s is None else y * s)
            if e is not None:
                t = t + e
            z = ln(t)
        loss = 0.0
        if use in ("t", "both"):
            loss = loss + (t * up_t.to(DEV, dt)).sum()
        if use in ("z", "both"):
            loss = loss + (z * up_z.to(DEV, dt)).sum()
        loss.backward()
        res.append([t.detach(), z.detach(), x.grad, ln.weight.grad, ln.bias.grad] + ([y.grad] if use_y else [])
                   + ([e.grad] if use_e else []))
    names = launches.take()
    assert names[0] == "geot_res_ln" and (use == "t" and not (use_y or use_e) or "geot_res_ln_grad" in names), names
    for i, (a, f) in enumerate(zip(*res)):
        _assert_rule((b, n, c, use_y, use_s, use_e, use, i), a, f, 2e-5, 2e-5 * 1e-9)


RES_LN_ROWS = ((1, 1), (3, 1), (1, 7), (3, 3), (3, 500))     # rows 1, 3, 7, 9 (fwd: not a multiple of 4; bwd: of 8), 1500


@pytest.mark.parametrize("bn", RES_LN_ROWS)
@pytest.mark.parametrize("c", (128, 256, 384, 512, 768, 1024))
def test_res_ln_every_width_and_row_count(c, bn, lib, launches):
    assert lib.geot_res_ln_supported(c)
    if bn == (3, 500):
        assert -(-1500 // 8) > 128                           # the finish kernel's unrolled loop runs
    check_res_ln(bn[0], bn[1], c, True, True, True, "both", launches)


@pytest.mark.parametrize("use", ("t", "z", "both"))
@pytest.mark.parametrize("use_y,use_s,use_e", ((True, True, True), (True, True, False), (True, False, True), (True, False, False),
                                               (False, False, True), (False, False, False)))
@pytest.mark.parametrize("bn", ((3, 3), (3, 500)))
def test_res_ln_inputs_and_outputs_used(bn, use_y, use_s, use_e, use, launches):
    check_res_ln(bn[0], bn[1], 256, use_y, use_s, use_e, use, launches)


# ---- qkv_split: geot_qkv_split / _grad ----------------------------------------------------------------------------------
SUBSETS = ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2))


def _qkv_restated(x, b, n, h, d, scale):
    q, k, v = x.view(b, n, 3, h, d).permute(2, 0, 3, 1, 4).contiguous().view(3, b * h, n, d).unbind(0)
    return q * scale, k, v


def check_qkv_split(b, n, h, d, used, launches, seed=0):
    """bit-equal to the permute + contiguous restatement, forward and backward (unused outputs: zero gradient)"""
    from geot_amd.fused_norm import qkv_split
    gen = _gen("qkv", b, n, h, d, used, seed)
    scale = d ** -0.5
    x0 = torch.randn(b, n, 3 * h * d, generator=gen).to(DEV)
    ups = [torch.randn(b * h, n, d, generator=gen).to(DEV) for _ in range(3)]
    res = []
    for fused in (False, True):
        x = x0.clone().requires_grad_(True)
        outs = qkv_split(x, h, scale) if fused else _qkv_restated(x, b, n, h, d, scale)
        sum((outs[i] * ups[i]).sum() for i in used).backward()
        res.append([o.detach() for o in outs] + [x.grad])
    assert launches.take() == ["geot_qkv_split", "geot_qkv_split_grad"]
    for a, f in zip(*res):
        assert torch.equal(a, f), (b, n, h, d, used)


@pytest.mark.parametrize("used", SUBSETS)
@pytest.mark.parametrize("h", (1, 6))
@pytest.mark.parametrize("d", (4, 12, 64))
def test_qkv_split_every_subset(d, h, used, launches):
    check_qkv_split(2, 37, h, d, used, launches)


def test_qkv_split_past_the_grid_cap(launches):
    b, n, h, d = 16, 1024, 8, 64
    assert 3 * b * n * h * d // 4 > 16384 * 256                # the 16 384-block grid strides
    check_qkv_split(b, n, h, d, (0, 1, 2), launches)
    torch.cuda.empty_cache()


# ---- softmax_last: geot_softmax_grad -------------------------------------------------------------------------------------
def check_softmax_last(shape, launches, seed=0):
    """the rule of test_softmax_last_gradient: forward within 1e-6 (torch's fp32 soft-max), gradient within 2e-6 of its
    largest value + 1e-7"""
    from geot_amd.fused_norm import softmax_last
    gen = _gen("softmax", shape, seed)
    x0, up = torch.randn(*shape, generator=gen) * 3, torch.randn(*shape, generator=gen)
    res = []
    for fused in (False, True):
        x = (x0.to(DEV) if fused else x0.to(DEV).double()).requires_grad_(True)
        y = softmax_last(x) if fused else x.softmax(dim=-1)
        (y * up.to(DEV, y.dtype)).sum().backward()
        res.append((y.detach(), x.grad))
    assert launches.take() == ["geot_softmax_grad"]
    assert float((res[0][0] - res[1][0].double()).abs().max()) <= 1e-6, shape
    _assert_rule("dx", res[0][1], res[1][1], 2e-6, 1e-7)


@pytest.mark.parametrize("rows", ((1,), (5,), (3, 7)))
@pytest.mark.parametrize("n", (64, 128, 256, 512, 1024))
def test_softmax_last_every_row_length(n, rows, launches):
    check_softmax_last(rows + (n,), launches)


# ---- bn_act: geot_bn_stats / apply / bwd_reduce / bwd_apply --------------------------------------------------------------
def check_bn_act(b, c, l, relu, training, launches, seed=0):
    """vs fp64 nn.BatchNorm1d (+ ReLU) over two steps, at the rule of test_bn_act_equals_torch_batchnorm_relu"""
    from geot_amd.fused_norm import bn_act
    gen = _gen("bnact", b, c, l, relu, training, seed)
    x0 = torch.randn(b, c, l, generator=gen) * 2 + 0.5
    up = torch.randn(b, c, l, generator=gen)
    ref, ours = _bn_pair(c, gen)
    ref.to(DEV).train(training); ours.to(DEV).train(training)
    res = []
    for mod, fused in ((ref, False), (ours, True)):
        x = (x0.to(DEV) if fused else x0.to(DEV).double()).requires_grad_(True)
        for _ in range(2):                                   # two steps: the running statistics move twice
            y = bn_act(mod, x, relu=relu) if fused else (torch.relu(mod(x)) if relu else mod(x))
        (y * up.to(DEV, y.dtype)).sum().backward()
        res.append([y.detach(), x.grad, mod.weight.grad, mod.bias.grad, mod.running_mean, mod.running_var])
    names = launches.take()
    assert "geot_bn_apply" in names and "geot_bn_bwd_apply" in names and ("geot_bn_stats" in names) == training, names
    for name, a, f in zip(("out", "dx", "dgamma", "dbeta", "running_mean", "running_var"), *res):
        _assert_rule(name, a, f, 2e-5, 1e-6)


@pytest.mark.parametrize("relu", (True, False))
@pytest.mark.parametrize("training", (True, False))
@pytest.mark.parametrize("b,c,l", ((1, 2, 262147), (2, 3, 262144), (3, 5, 1001)))
def test_bn_act_slice_and_grid_caps(b, c, l, training, relu, lib, launches):
    """(1, 2, 262147) and (2, 3, 262144): BN_MAX_SLICES = 32 statistics slices and bn_gx = 64 blocks per row; odd l: every
    row after the first starts off the 16-byte boundary and takes the scalar path"""
    if l >= 262144:
        assert lib.geot_bn_slices(b, c, l) == 32 and min(64, -(-(l // 4) // 1024)) == 64
    check_bn_act(b, c, l, relu, training, launches)


# ---- storage at an offset -------------------------------------------------------------------------------------------------
def _run(fn, inputs, ups, k_in, k_grad):
    """fn(*inputs) -> outputs; inputs placed k_in elements off the 16-byte boundary, the outputs' gradients handed over
    k_grad elements off it -> (outputs, input gradients)"""
    ins = [(at_offset(t, k_in) if k_in else t.clone()).requires_grad_(t.is_floating_point()) for t in inputs]
    for t in ins:
        assert t.is_contiguous() and t.data_ptr() % 16 == 4 * k_in
    outs = fn(*ins)
    if outs is None:
        return None, None
    backward_at_offset(list(outs), ups, k_grad) if k_grad else sum((o * u).sum() for o, u in zip(outs, ups)).backward()
    return [o.detach() for o in outs], [t.grad for t in ins]


def _misaligned_cases():
    from geot_amd import fused_norm as fn
    gen = _gen("misaligned")
    r = lambda *s: torch.randn(*s, generator=gen).to(DEV)                                          # noqa: E731
    bn_state = _bn_pair(6, gen)[1].state_dict()

    def with_bn(f):
        def g(*a):
            bn = torch.nn.BatchNorm1d(6).to(DEV)
            bn.load_state_dict(bn_state)
            return f(bn, *a)
        return g
    # name -> (fn, inputs, upstream gradients, indices of outputs + input gradients that must be bit-equal with misaligned
    # inputs).  The others pass through a torch kernel (GEMM, soft-max) or a BatchNorm pass whose vector / scalar path may
    # follow the address, or through the torch fallback of bn_relu_max: they are held to the op's rule.
    ALL = tuple(range(8))
    return {
        "max_last": (lambda x: (fn.max_last(x),), [r(40, 3, 32)], [r(40, 3)], ALL),
        "max_last_n4": (lambda x: (fn.max_last(x),), [r(77, 4)], [r(77)], ALL),
        "add_last_broadcast": (lambda a, p: (fn.add_last_broadcast(a, p),), [r(33, 5, 16), r(33, 5)], [r(33, 5, 16)], ALL),
        "bn_relu_max": (with_bn(lambda bn, y: (fn.bn_relu_max(bn, y, 8),)), [r(2, 6, 11 * 8)], [r(2, 6, 11)], ()),
        "bn_act": (with_bn(lambda bn, x: (fn.bn_act(bn, x, relu=True),)), [r(2, 6, 999)], [r(2, 6, 999)], ()),
        "qkv_split": (lambda x: fn.qkv_split(x, 2, 0.25), [r(2, 9, 3 * 2 * 12)], [r(4, 9, 12) for _ in range(3)], ALL),
        "thin_mm": (lambda w, x: (fn.thin_mm(w, x),), [r(7, 3), r(3, 5001)], [r(7, 5001)], (1,)),       # d w: rowdot_small
        "linear": (lambda x, w, b: (fn._LinearFn.apply(x, w, b),), [r(3, 11, 16), r(40, 16), r(40)], [r(3, 11, 40)],
                   (3,)),                                                                             # d b: colsum
        "add_channel_bias": (lambda y, b: (fn.add_channel_bias(y, b),), [r(2, 6, 301), r(6)], [r(2, 6, 301)], ALL),
        "res_ln": (lambda x, y, e, w, b: fn._ResLnFn.apply(x, y, None, e, w, b, 1e-5),
                   [r(2, 9, 128), r(2, 9, 128), r(2, 9, 128), r(128), r(128)], [r(2, 9, 128), r(2, 9, 128)], ALL),
        "layer_norm": (lambda x, w, b: (fn._LnFn.apply(x, w, b, 1e-5),), [r(2, 9, 128), r(128), r(128)], [r(2, 9, 128)], ALL),
        "softmax_last": (lambda x: (fn.softmax_last(x),), [r(6, 64)], [r(6, 64)], ()),
    }


@pytest.mark.parametrize("where", ("inputs", "gradients"))
@pytest.mark.parametrize("k", (1, 2, 3))
@pytest.mark.parametrize("op", ("max_last", "max_last_n4", "add_last_broadcast", "bn_relu_max", "bn_act", "qkv_split", "thin_mm",
                                "linear", "add_channel_bias", "res_ln", "layer_norm", "softmax_last"))
def test_storage_off_the_16_byte_boundary(op, k, where):
    """a contiguous tensor at a 4-, 8- or 12-byte offset (inputs), and a backward handed such a gradient (a slice of the
    gradient of a torch.cat): the call succeeds and matches the aligned run.  A misaligned gradient must give the aligned
    result bit for bit (the float4 kernels take a copy; the others read it element by element) except in bn_act, whose
    reduction pass sums in another order on the scalar path; misaligned inputs: see _misaligned_cases."""
    fn, inputs, ups, exact_in = _misaligned_cases()[op]
    k_in, k_grad = (k, 0) if where == "inputs" else (0, k)
    outs, grads = _run(fn, inputs, ups, 0, 0)
    outs_k, grads_k = _run(fn, inputs, ups, k_in, k_grad)
    if op == "qkv_split" and k_in:
        assert outs_k is None                                # not covered: the caller takes its torch composition
        return
    for i, (a, f) in enumerate(zip(outs + grads, outs_k + grads_k)):
        if (i in exact_in) if k_in else op != "bn_act":
            assert torch.equal(a, f), (op, k, where, i)
        else:
            _assert_rule((op, k, where, i), a, f, 3e-5, 1e-6)


# ---- the model's own shapes ---------------------------------------------------------------------------------------------
def test_model_shapes_run_the_tested_kernels(lib, launches):
    """The shapes the model passes (TOOTH_SEG_CFG: width 384, 4 heads, 512 groups of 32 points, Encoder 256; the SA modules'
    nsample 32 and 16), each compared as above and asserted to launch its kernel: a retune that moved one of them off the
    tested branches, or to a torch fallback, fails here."""
    from geot_amd.openpoints.models.backbone.transformer import TOOTH_SEG_CFG as cfg
    c, heads, g, n, enc = cfg["trans_dim"], cfg["num_heads"], cfg["num_group"], cfg["group_size"], cfg["encoder_dims"]
    bs = 2
    assert (c, heads, g, n, enc) == (384, 4, 512, 32, 256)
    check_thin_mm(3, 128, bs * g * n, lib, launches)                   # Encoder first conv (3 -> 128): weight gradient
    check_max_last((enc, bs * g, n), launches)                         # Encoder: max over a group's points (LPR 8)
    check_add_last_broadcast((2 * enc, g, n), launches)                # Encoder: the pooled half broadcast over the group
    check_linear((bs, g), c, 4 * c, lib, launches)                     # transformer blocks: Linear bias gradients
    check_res_ln(bs, g, c, True, True, True, "both", launches)        # transformer blocks
    check_res_ln(bs, g, c, False, False, True, "both", launches)
    check_qkv_split(bs, g, heads, c // heads, (0, 1, 2), launches)     # d = 96
    check_softmax_last((bs * heads, g, g), launches)
    check_bn_act(1, 128, bs * g * n, True, True, launches)             # Encoder's BatchNorms on (1, C, L)
    for ns in (32, 16):                                                # SA modules: BatchNorm -> ReLU -> max over nsample
        check_bn_relu_max(2, 8, 64, ns, launches)
        check_max_last((2, 64, 128, ns), launches)
