"""GPU tests of conv_max_last (fused_norm.py) and its backward kernels geot_maxconv_dgrad / geot_maxconv_wgrad
(csrc/max_conv.hip): out = max over every group's n columns of W x, back-propagated from the max's one non-zero per (channel,
group) without the dense gradient of W x.

Reference: the same function in fp64 torch on the GPU -- y = W x, y.view(Co, G, n).max(-1), autograd.  Bound on dW and dx:
2e-5 * max|reference| + 1e-6, the one tests/test_encoder_fold_gpu.py holds this encoder to.

W and x are drawn from the multiples of 1/8 in [-1, 1]: every product is a multiple of 1/64 and a sum of up to 512 of them
stays below 2^10, so W x is exact in fp32 in any summation order and the fp32 and fp64 maxima sit in the same slots.  (With
arbitrary floats two columns of a group can lie closer than fp32's rounding of the dot product, the two precisions then choose
different slots and the gradients differ by whole entries: a property of the comparison, not of the kernels.)  The grid also
makes ties frequent in every pattern, which holds arg to torch.max's first-slot rule throughout.  The upstream gradients are
arbitrary floats, so the sums under test round as they do in use."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(5, 8, 1, 4),            # one group, the smallest n
          (7, 12, 3, 32),          # nothing is a multiple of a tile
          (33, 68, 70, 32),        # 3 channel slabs, 3 group chunks (32, 32, 6), odd Co
          (256, 128, 9, 32),       # the workload's channel counts: first_conv.3 ...
          (256, 512, 5, 32),       # ... and second_conv.3
          (6, 16, 4, 256),         # the largest n
          (1024, 8, 9, 64),        # the largest Co: 4 blocks of output channels, 4 sorting waves in two passes
          (1024, 8, 2, 256)]       # ... with the largest n: one sorting wave, 129 KB of LDS in either kernel
PATTERNS = ["random", "same_slot", "tied", "zero_rows"]


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a comparison that fails is one failed case; a device error ends the session: nothing more is launched after it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error, stopping: %s" % e, returncode=3)


def _grid(gen, *shape):
    return torch.randint(-8, 9, shape, generator=gen).float() / 8


@functools.lru_cache(maxsize=None)
def _case(co, ci, g, n, pattern):
    """(w, x, up) on the GPU and the fp64 reference (out, dw, dx, arg) of one shape and input pattern, computed once"""
    gen = torch.Generator().manual_seed(co * 1000 + ci * 10 + g + n + 7 * PATTERNS.index(pattern))
    w, x = _grid(gen, co, ci), _grid(gen, ci, g * n)
    up = torch.randn(co, g, generator=gen) + 0.25
    if pattern == "same_slot":       # W > 0 and one column per group above every other in every row: all channels choose it
        w = w.abs() + 0.125
        for k in range(g):
            x[:, k * n + (7 * k + 3) % n] = 1.25
    elif pattern == "tied":          # a group's columns are copies of two: the maximum is met n / 2 times
        x = x.view(ci, g, n)[:, :, :2].repeat(1, 1, n // 2).reshape(ci, g * n).contiguous()
    elif pattern == "zero_rows":
        up[::2] = 0.0
    w, x, up = w.to(DEV), x.to(DEV), up.to(DEV)
    wd, xd = w.double().requires_grad_(True), x.double().requires_grad_(True)
    out, arg = (wd @ xd).view(co, g, n).max(-1)
    dw, dx = torch.autograd.grad(out, (wd, xd), up.double())
    return w, x, up, (out.detach(), dw, dx, arg)


def _run(w, x, up, n, fused, monkeypatch):
    from geot_amd.fused_norm import conv_max_last
    monkeypatch.setenv("GEOT_MAX_CONV", "1" if fused else "0")
    wt, xt = w.clone().requires_grad_(True), x.clone().requires_grad_(True)
    out = conv_max_last(wt, xt, n)
    assert (type(out.grad_fn).__name__ == "_ConvMaxLastFnBackward") == fused
    dw, dx = torch.autograd.grad(out, (wt, xt), up)
    return out.detach(), dw, dx


def _check(co, ci, g, n, pattern, monkeypatch):
    w, x, up, (r_out, r_dw, r_dx, r_arg) = _case(co, ci, g, n, pattern)
    out, dw, dx = _run(w, x, up, n, True, monkeypatch)
    out2, dw2, dx2 = _run(w, x, up, n, True, monkeypatch)
    old = _run(w, x, up, n, False, monkeypatch)
    assert torch.equal(out, old[0]) and torch.equal(out.double(), r_out)      # the forward is the old one (and exact here)
    for name, ref, got, was in (("dW", r_dw, dw, old[1]), ("dx", r_dx, dx, old[2])):
        bound = 2e-5 * float(ref.abs().max()) + 1e-6
        err, err_old = float((got.double() - ref).abs().max()), float((was.double() - ref).abs().max())
        print("%s %s %s: bound %.3e, new - fp64 %.3e (old - fp64 %.3e)" % ((co, ci, g, n), pattern, name, bound, err, err_old))
        assert got.shape == ref.shape and err <= bound, (name, err, bound)
    assert torch.equal(dw, dw2) and torch.equal(dx, dx2)                      # the same bits on every call
    chosen = torch.zeros(g * n, dtype=torch.bool, device=DEV)
    chosen[(torch.arange(g, device=DEV) * n + r_arg).flatten()] = True
    assert not bool(dx[:, ~chosen].any()), "a column no channel selected is not exactly zero"
    if pattern == "same_slot":
        assert int(chosen.sum()) == g
    return dw, dx


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("co,ci,g,n", SHAPES)
def test_conv_max_last_against_fp64(co, ci, g, n, pattern, monkeypatch):
    from geot_amd import _lib
    if (co, ci, g, n) == (33, 68, 70, 32):
        assert _lib.load().geot_maxconv_ws_floats(co, ci, g, n) == 3 * co * ci
    _check(co, ci, g, n, pattern, monkeypatch)


@pytest.mark.parametrize("chunk", [1, 7])
def test_wgrad_chunks_pinned(chunk, monkeypatch):
    """GEOT_MAXCONV_CHUNK: 70 chunks of one group (every step a partial one), and 10 chunks of 7 (steps of 4 + 3)"""
    from geot_amd import _lib
    co, ci, g, n = 33, 68, 70, 32
    monkeypatch.setenv("GEOT_MAXCONV_CHUNK", str(chunk))
    assert _lib.load().geot_maxconv_ws_floats(co, ci, g, n) == -(-g // chunk) * co * ci
    for pattern in PATTERNS:
        _check(co, ci, g, n, pattern, monkeypatch)


@pytest.mark.parametrize("co,ci,g,n", SHAPES)
def test_results_do_not_depend_on_what_dx_and_ws_held(co, ci, g, n, monkeypatch):
    """the entry points themselves, on buffers pre-filled with NaN: every element of dx and dW is written, none is read"""
    from geot_amd import _lib
    from geot_amd.ext._common import call, ptr
    w, x, up, (_, _, _, r_arg) = _case(co, ci, g, n, "random")
    _, dw, dx = _run(w, x, up, n, True, monkeypatch)
    arg = r_arg.to(torch.uint8).contiguous()
    nan = float("nan")
    ws = torch.full((int(_lib.load().geot_maxconv_ws_floats(co, ci, g, n)),), nan, device=DEV)
    gw, gx = torch.full_like(w, nan), torch.full_like(x, nan)
    call("geot_maxconv_wgrad", w.device, co, ci, g, n, ptr(x), ptr(up), ptr(arg), ptr(ws), ptr(gw))
    call("geot_maxconv_dgrad", w.device, co, ci, g, n, ptr(w), ptr(up), ptr(arg), ptr(gx))
    assert torch.equal(gw, dw) and torch.equal(gx, dx)
    assert not bool(torch.isnan(ws).any())              # ws holds exactly the chunks' partial sums


def test_encoder_with_and_without_max_conv(monkeypatch):
    from geot_amd.ext import _common
    from geot_amd.openpoints.models.backbone.transformer import Encoder
    bs, g, n = 2, 3, 32
    gen = torch.Generator().manual_seed(11)
    pts = torch.randn(bs, g, n, 3, generator=gen).to(DEV)
    up = torch.randn(bs, g, 64, generator=gen).to(DEV)
    torch.manual_seed(0)
    base = Encoder(64, factored=True).to(DEV).train()
    res, names = {}, []
    monkeypatch.setattr(_common, "trace", lambda launch, name: (names.append(name), launch())[1])
    for env in ("1", "0"):
        monkeypatch.setenv("GEOT_MAX_CONV", env)
        enc = Encoder(64, factored=True).to(DEV).train()
        enc.load_state_dict(base.state_dict())
        del names[:]
        out = enc(pts)
        (out * up).sum().backward()
        res[env] = (out.detach(), {k: p.grad.detach() for k, p in enc.named_parameters()})
        new, old = names.count("geot_maxconv_dgrad") + names.count("geot_maxconv_wgrad"), names.count("geot_segment_max_grad")
        assert (new, old) == ((4, 0) if env == "1" else (0, 2)), names      # both maxima take the new backward, or neither
    assert torch.equal(res["1"][0], res["0"][0])
    assert set(res["1"][1]) == set(res["0"][1])
    bad = []
    for k, ref in res["0"][1].items():
        bound = 2e-5 * float(ref.abs().max()) + 1e-6
        err = float((res["1"][1][k].double() - ref.double()).abs().max())
        print("%s: bound %.3e, on - off %.3e" % (k, bound, err))
        if err > bound:
            bad.append((k, err, bound))
    assert not bad, bad


def test_forward_and_backward_capture_as_kernel_nodes(monkeypatch):
    from geot_amd import streams
    co, ci, g, n = 33, 68, 70, 32
    w, x, up, _ = _case(co, ci, g, n, "random")
    out, dw, dx = _run(w, x, up, n, True, monkeypatch)          # eager: also every one-time set-up a first launch does
    from geot_amd.fused_norm import conv_max_last
    wt, xt = w.clone().requires_grad_(True), x.clone().requires_grad_(True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with streams.capture(graph, torch.device(DEV)):
        o = conv_max_last(wt, xt, n)
        gw, gx = torch.autograd.grad(o, (wt, xt), up)
    kinds = streams.node_types(graph)
    assert set(kinds) == {"kernel"}, kinds
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(o.detach(), out) and torch.equal(gw, dw) and torch.equal(gx, dx)


def test_unsupported_shape_takes_the_old_composition(monkeypatch):
    """ci = 6 is no multiple of 4: the old two launches and their dense backward, and their result"""
    from geot_amd import _lib
    from geot_amd.fused_norm import conv_max_last
    co, ci, g, n = 7, 6, 3, 32
    assert _lib.load().geot_maxconv_ws_floats(co, ci, g, n) == -1
    gen = torch.Generator().manual_seed(3)
    w, x, up = _grid(gen, co, ci).to(DEV), _grid(gen, ci, g * n).to(DEV), torch.randn(co, g, generator=gen).to(DEV)
    monkeypatch.setenv("GEOT_MAX_CONV", "1")
    wt, xt = w.clone().requires_grad_(True), x.clone().requires_grad_(True)
    out = conv_max_last(wt, xt, n)
    assert type(out.grad_fn).__name__ != "_ConvMaxLastFnBackward"
    dw, dx = torch.autograd.grad(out, (wt, xt), up)
    wd, xd = w.double().requires_grad_(True), x.double().requires_grad_(True)
    ref = (wd @ xd).view(co, g, n).max(-1)[0]
    r_dw, r_dx = torch.autograd.grad(ref, (wd, xd), up.double())
    assert torch.equal(out.detach().double(), ref.detach())
    for r, got in ((r_dw, dw), (r_dx, dx)):
        assert float((got.double() - r).abs().max()) <= 2e-5 * float(r.abs().max()) + 1e-6
