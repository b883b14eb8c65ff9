"""GPU tests of the Encoder's folds (csrc/bnrelu.hip geot_bn_*_seg, geot_thin_*; fused_norm.bn_act(seg=), thin_bn_act):
the BatchNorm passes over x + a per-(channel, segment) addend that is never added in memory, the thin first stage
relu(bn(W x)) that never stores W x, and the Encoder with them against GEOT_ENCODER_FOLD=0 and the reference op order.

References are fp64 restatements in torch (_bn_ref: written out, so that a single column per channel -- which
nn.BatchNorm1d refuses in training mode -- has one too; the unbiased factor is n / max(n - 1, 1) there, as in
geot_bn_finalize).  The bound of every kernel-level comparison is the one the bn_act tests use (test_model_gpu.py:
2e-5 * max|reference| + 1e-6): the arithmetic is theirs plus one add, or a dot product of <= 8 terms.

The upstream gradients have mean 1, not 0.  The bound is relative to the largest entry of the reference, and the cases with
one or two channels leave d beta = sum g as the only entries: with a zero-mean gradient that sum over ~10^4 terms of both
signs comes out near zero by chance, and a bound relative to it then measures the conditioning of the draw, not the kernel.
Measured with zero-mean gradients at (B, C, G, n) = (1, 1, 1025, 12), ReLU, eval mode, pre_bias: d beta = -0.4736, the
unfolded path (add_last_broadcast -> bn_act, fp32 partial sums) 2.27e-5 from fp64, the folded one (fp64 partial sums) within
the bound of fp64 and therefore 2.27e-5 from the unfolded one, against a bound of 1.05e-5 -- no kernel can be within it of
both.  With mean 1 the sums are as well conditioned as the many-channel cases' largest entries are."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 1e-5, 0.1


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a comparison that fails is one failed case; a device error ends the session: nothing more is launched after it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error, stopping: %s" % e, returncode=3)


def _close(name, ref, got):
    ref, got = ref.double(), got.double()
    assert ref.shape == got.shape, (name, ref.shape, got.shape)
    scale = float(ref.abs().max()) + 1e-12
    err = float((ref - got).abs().max())
    assert err <= 2e-5 * scale + 1e-6, (name, err, scale)
    return err


def _bn_ref(z, gamma, beta, rm, rv, training, relu, pre_bias):
    """fp64: act(bn(z + pre_bias)) for z (C, N) -> (out, running_mean, running_var after the call)"""
    if pre_bias is not None:
        z = z + pre_bias.view(-1, 1)
    n = z.shape[1]
    if training:
        mean = z.mean(1)
        var = ((z - mean.view(-1, 1)) ** 2).mean(1)
        with torch.no_grad():
            rm = (1 - MOMENTUM) * rm + MOMENTUM * mean
            rv = (1 - MOMENTUM) * rv + MOMENTUM * var * (n / max(n - 1, 1))
    else:
        mean, var = rm, rv
    out = (z - mean.view(-1, 1)) * torch.rsqrt(var + EPS).view(-1, 1) * gamma.view(-1, 1) + beta.view(-1, 1)
    return (torch.relu(out) if relu else out), rm, rv


def _module(c, params, training, dev):
    gamma, beta, rm, rv = params
    bn = torch.nn.BatchNorm1d(c, eps=EPS, momentum=MOMENTUM).to(dev)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    return bn.train(training)


def _params(c, g):
    return (torch.randn(c, generator=g), torch.randn(c, generator=g), torch.rand(c, generator=g) - 0.5,
            torch.rand(c, generator=g) * 1.5 + 0.5)


# ---- the segment-addend passes -------------------------------------------------------------------------------------------
SEG_SHAPES = [(1, 1, 1025, 12),     # L = 12 300: 3 slices of 4 100 columns, boundaries inside a segment
              (2, 5, 3, 4),         # smallest n
              (1, 67, 129, 32),     # the bench's n, odd channel count
              (3, 8, 33, 36),       # n not a power of two
              (1, 2, 40, 256)]      # largest n


@pytest.mark.parametrize("pre_bias", [False, True])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("B,C,G,n", SEG_SHAPES)
def test_segment_addend_passes(B, C, G, n, relu, training, pre_bias):
    from geot_amd import _lib
    from geot_amd.fused_norm import add_last_broadcast, bn_act
    dev = torch.device("cuda:0")
    L = G * n
    if (B, C, G, n) == SEG_SHAPES[0]:
        assert _lib.load().geot_bn_slices(B, C, L) == 3 and 4100 % n != 0
    g = torch.Generator().manual_seed(1000 * B + 10 * C + n)
    a0 = torch.randn(B, C, L, generator=g) * 2 + 0.5
    p0 = torch.randn(B, C, G, generator=g) * 1.5
    up = torch.randn(B, C, L, generator=g) + 1.0       # mean 1: see the module docstring
    params = _params(C, g)
    bias0 = torch.randn(C, generator=g) if pre_bias else None

    # fp64 reference
    a, p = a0.double().requires_grad_(True), p0.double().requires_grad_(True)
    gamma, beta = params[0].double().requires_grad_(True), params[1].double().requires_grad_(True)
    z = (a.view(B, C, G, n) + p.unsqueeze(-1)).view(B, C, L).transpose(0, 1).reshape(C, B * L)
    out, rm, rv = _bn_ref(z, gamma, beta, params[2].double(), params[3].double(), training, relu,
                          None if bias0 is None else bias0.double())
    out = out.view(C, B, L).transpose(0, 1)
    (out * up.double()).sum().backward()
    want = dict(out=out.detach(), dx=a.grad, dseg=p.grad, dgamma=gamma.grad, dbeta=beta.grad, running_mean=rm, running_var=rv)

    def run(fold):
        bn = _module(C, params, training, dev)
        x, s = a0.to(dev).requires_grad_(True), p0.to(dev).requires_grad_(True)
        bias = None if bias0 is None else bias0.to(dev).requires_grad_(True)
        if fold:
            y = bn_act(bn, x, relu=relu, pre_bias=bias, seg=s)
            assert type(y.grad_fn).__name__ == "_BnActSegFnBackward"          # the kernels ran, not the composition
        else:
            y = bn_act(bn, add_last_broadcast(x.view(B, C, G, n), s).view(B, C, L), relu=relu, pre_bias=bias)
        (y * up.to(dev)).sum().backward()
        return dict(out=y.detach(), dx=x.grad, dseg=s.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad,
                    running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone())

    new, again, old = run(True), run(True), run(False)
    bad = []
    for k in want:
        ref, got, was = want[k], new[k].cpu().double(), old[k].cpu().double()
        bound = 2e-5 * (float(ref.abs().max()) + 1e-12) + 1e-6
        e_ref, e_old, e_was = (float((p - q).abs().max()) for p, q in ((ref, got), (was, got), (ref, was)))
        print("%s: bound %.3e, new - fp64 %.3e, new - old %.3e (old - fp64 %.3e)" % (k, bound, e_ref, e_old, e_was))
        if e_ref > bound:
            bad.append((k + " against fp64", e_ref, bound))
        if e_old > 2e-5 * (float(was.abs().max()) + 1e-12) + 1e-6:
            bad.append((k + " against add_last_broadcast -> bn_act", e_old, bound))
        assert torch.equal(new[k], again[k]), k                                 # fixed-order sums: the same bits on every call
    assert not bad, bad


# ---- the thin first stage ------------------------------------------------------------------------------------------------
THIN_SHAPES = [(3, 5, 1, 0.0),        # single column
               (1, 1, 63, 0.0),       # smallest J and C
               (3, 128, 4100, 0.0),   # the bench's J and C
               (3, 128, 4100, 50.0),  # x = 50 sigma + noise: the pivot matters
               (8, 67, 8200, 0.0),    # largest J, odd C
               (3, 128, 12300, 0.0)]  # several slices


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("J,C,L,offset", THIN_SHAPES)
def test_thin_stage(J, C, L, offset, relu, training):
    from geot_amd import _lib
    from geot_amd.fused_norm import bn_act, thin_bn_act, thin_mm
    dev = torch.device("cuda:0")
    if L == 12300:
        assert _lib.load().geot_thin_bn_bwd_slices(C, L) == 3 and _lib.load().geot_thin_moments_slices(L) > 1
    g = torch.Generator().manual_seed(100 * J + C + L)
    x0 = torch.randn(J, L, generator=g) + offset
    w0 = torch.randn(C, J, generator=g) * 0.5
    up = torch.randn(C, L, generator=g) + 1.0          # mean 1: see the module docstring
    params = _params(C, g)
    bias0 = torch.randn(C, generator=g)

    w, gamma, beta = (t.double().requires_grad_(True) for t in (w0, params[0], params[1]))
    out, rm, rv = _bn_ref(w @ x0.double(), gamma, beta, params[2].double(), params[3].double(), training, relu, bias0.double())
    (out * up.double()).sum().backward()
    want = dict(out=out.detach(), dw=w.grad, dgamma=gamma.grad, dbeta=beta.grad, running_mean=rm, running_var=rv)

    def run(fold):
        bn = _module(C, params, training, dev)
        wt, bias, x = w0.to(dev).requires_grad_(True), bias0.to(dev).requires_grad_(True), x0.to(dev)
        if fold:
            y = thin_bn_act(bn, wt, x, bias, relu=relu)
            assert type(y.grad_fn).__name__ == "_ThinBnActFnBackward"
        else:
            y = bn_act(bn, thin_mm(wt, x).unsqueeze(0), relu=relu, pre_bias=bias).squeeze(0)
        (y * up.to(dev)).sum().backward()
        return dict(out=y.detach(), dw=wt.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad,
                    running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone())

    new, again, old = run(True), run(True), run(False)
    for k in ("out", "dw", "dgamma", "dbeta"):
        _close(k, want[k], new[k].cpu())
    for k in ("running_mean", "running_var"):      # the statistics: no worse than the old path's on the same input, or the bound
        ref = want[k]
        err_new, err_old = (float((ref - t[k].cpu().double()).abs().max()) for t in (new, old))
        print("%s J=%d C=%d L=%d offset=%g: error new %.3e old %.3e" % (k, J, C, L, offset, err_new, err_old))
        assert err_new <= max(err_old, 2e-5 * (float(ref.abs().max()) + 1e-12) + 1e-6), (k, err_new, err_old)
    for k in new:
        assert torch.equal(new[k], again[k]), k


def test_thin_stage_falls_back_when_x_needs_a_gradient():
    from geot_amd.fused_norm import thin_bn_act
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    x0, w0, up = torch.randn(3, 260, generator=g), torch.randn(7, 3, generator=g), torch.randn(7, 260, generator=g)
    params = _params(7, g)
    x, w = x0.double().requires_grad_(True), w0.double().requires_grad_(True)
    out, _, _ = _bn_ref(w @ x, params[0].double(), params[1].double(), params[2].double(), params[3].double(), True, True, None)
    (out * up.double()).sum().backward()
    bn = _module(7, params, True, dev)
    xg, wg = x0.to(dev).requires_grad_(True), w0.to(dev).requires_grad_(True)
    y = thin_bn_act(bn, wg, xg, None, relu=True)
    assert type(y.grad_fn).__name__ != "_ThinBnActFnBackward"
    (y * up.to(dev)).sum().backward()
    _close("out", out.detach(), y.detach().cpu())
    _close("dx", x.grad, xg.grad.cpu())
    _close("dw", w.grad, wg.grad.cpu())
    y8 = thin_bn_act(bn, torch.randn(7, 9, device=dev), torch.randn(9, 64, device=dev), None)       # J > 8: the old path too
    assert type(y8.grad_fn).__name__ != "_ThinBnActFnBackward"


# ---- the Encoder -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs,g,n", [(2, 3, 32), (1, 1, 4)])
def test_encoder_fold_equals_unfolded_and_reference_order(bs, g, n, monkeypatch):
    """Encoder(factored=True) with the folds, with GEOT_ENCODER_FOLD=0 and Encoder(factored=False): outputs and every
    parameter gradient within the model-level bound (test_model_gpu.py: rtol 2e-4, atol 2e-4 max|a|).  The biases in front
    of a BatchNorm have a mathematically zero gradient (first_conv.3's shifts both halves of what second_conv's BatchNorm
    sees): what each path leaves there is rounding noise, held to the criterion test_model_gpu.py holds it to."""
    from geot_amd.openpoints.models.backbone.transformer import Encoder
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(bs * 10 + n)
    pts = torch.randn(bs, g, n, 3, generator=gen).to(dev)
    up = torch.randn(bs, g, 64, generator=gen).to(dev)
    torch.manual_seed(0)
    base = Encoder(64, factored=False).to(dev).train()
    res = {}
    for name, factored, env in (("fold", True, "1"), ("unfolded", True, "0"), ("reference", False, "1")):
        monkeypatch.setenv("GEOT_ENCODER_FOLD", env)
        enc = Encoder(64, factored=factored).to(dev).train()
        enc.load_state_dict(base.state_dict())
        out = enc(pts)
        (out * up).sum().backward()
        res[name] = (out.detach(), {k: p.grad.detach() for k, p in enc.named_parameters()},
                     {k: b.detach().clone() for k, b in enc.named_buffers()})
    zero = ("first_conv.0.bias", "first_conv.3.bias", "second_conv.0.bias")
    for other in ("unfolded", "reference"):
        a, b = res[other][0], res["fold"][0]
        assert torch.allclose(a, b, rtol=2e-4, atol=2e-4 * float(a.abs().max())), (other, float((a - b).abs().max()))
        assert set(res[other][1]) == set(res["fold"][1])
        for k, ga in res[other][1].items():
            gb = res["fold"][1][k]
            if k in zero:
                wn = float(res["fold"][1][k[:-4] + "weight"].norm())
                assert float(ga.norm()) < 1e-3 * wn and float(gb.norm()) < 1e-3 * wn, (other, k)
                continue
            assert torch.allclose(ga, gb, rtol=2e-4, atol=2e-4 * float(ga.abs().max())), (other, k, float((ga - gb).abs().max()))
        for k, ba in res[other][2].items():
            bb = res["fold"][2][k]
            assert torch.allclose(ba.float(), bb.float(), rtol=2e-4, atol=2e-4 * float(ba.float().abs().max())), (other, k)
