"""The fused EdgeConv tail (csrc/edgeconv.hip) at every branch of its launch plan, against fp64.

Entry points: geot_edgeconv_gn_max, _grad, _grad_rix with geot_edgeconv_rix_build, and the autograd wrapper
transformer_ops.edgeconv_tail.  Every case asserts the plan it runs under (geot_edgeconv_plan), so a case that drifts onto
another branch fails: forward channels per workgroup 4 / 2 / 1 (1 and 2 also past 64 KiB of LDS) x {k = 4 with every
chunk full, k = 4 with a partial last chunk, the generic k loop}; dP channels 4 / 2 / 1; several slices in all three
passes; 1, 2, 4 and 8 lanes per target in the dP walk, hubs and mostly empty lists; k = 1, 3, 4, 7, 16, 255; groups 1, 4
and c; slopes 0, 0.2 and 1; gamma with 0, -0.0 and negatives; storage at 4-, 8- and 12-byte offsets; data far from zero.

The reference (tests/_edgeconv_ref.py) selects from the fp32 y = P[idx] + Q with the kernel's rule, so the selected y,
its slot and (for integer data) the sum over the slots must be exact.  Tolerances:
  * statistics: rstd within 1e-5 relative, mean within 1e-6 (|mean| + std), on every case;
  * zero-centred data: the output within what those statistics and a few fp32 roundings allow, every gradient within
    (gamma_D + 1e-5) x the sum of the magnitudes of the terms the kernel adds, D the depth of its summation tree, and
    everything within 2e-5 x max|reference| (the bar of test_model_gpu.py::test_edgeconv_tail_matches_composed);
  * far from zero (|mean| = 100 and 1000 std, P ~ +M against Q ~ -M): the output within 1e-3 (std ~ 1, |gamma| <= 2), the
    gradients no worse than 4 x the error of the fp32 torch composition the tail replaces, plus 1e-6 max|reference|.
Every case also checks that _grad and _grad_rix agree bit for bit, that a second call repeats bit for bit, that outputs
and gradients pre-filled with NaN come back fully written, and that edgeconv_tail returns the same bits."""
import math

import pytest
import torch

from _edgeconv_ref import MODEL_SHAPES, composed_fp32, plan, reference
from _fused_ref import at_offset, gamma

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 1e-5
E_STATS = 1e-5          # the statistics' asserted relative error, carried into every quantity that uses them
U32 = 2.0 ** -24
FAR_OUT_TOL = 1e-3      # |out - out_64| far from zero: y ~ 1000 in fp32 is 6e-5 per ulp; std ~ 1, |gamma| <= 2


def C(name, b, c, nq, nk, k, g, want, path, **kw):
    return pytest.param(dict(b=b, c=c, nq=nq, nk=nk, k=k, g=g, want=want, path=path, **kw), id=name)


CASES = [
    # forward 4 channels (nk <= 4096)
    C("f4_fast", 2, 8, 3000, 1000, 4, 4, dict(fwd_ch=4, bwd_ch=4, lg=0), "fast"),
    C("f4_rem", 1, 6, 2500, 700, 4, 2, dict(fwd_ch=4, bwd_ch=4, lg=1), "rem"),
    C("f4_gen_k3", 2, 8, 3000, 300, 3, 4, dict(fwd_ch=4, bwd_ch=4, lg=2), "generic", slope=0.0),
    # forward 2 channels: 64 KiB (nk <= 8192) and one workgroup's LDS (16384 < nk <= 19200)
    C("f2_fast", 1, 4, 5000, 6000, 4, 1, dict(fwd_ch=2, bwd_ch=2, lg=0), "fast"),
    C("f2_rem_groups_c", 1, 5, 2000, 8192, 4, 5, dict(fwd_ch=2, bwd_ch=4, lg=0), "rem"),
    C("f2_gen_k16", 1, 4, 2000, 5000, 16, 2, dict(fwd_ch=2, bwd_ch=4, lg=0), "generic", slope=1.0),
    C("f2_big_lds", 1, 4, 2048, 18000, 4, 4, dict(fwd_ch=2, fwd_lds=144000, bwd_ch=4), "fast"),
    C("f2_big_lds_rem", 1, 3, 2048, 18000, 4, 1, dict(fwd_ch=2, fwd_lds=144000, bwd_ch=4), "rem"),
    # forward 1 channel: 64 KiB and past it
    C("f1_fast", 1, 3, 2000, 12000, 4, 1, dict(fwd_ch=1, bwd_ch=4), "fast"),
    C("f1_gen_k1", 1, 3, 2000, 12000, 1, 3, dict(fwd_ch=1, bwd_ch=4, lg=0), "generic"),
    C("f1_big_lds", 1, 2, 2000, 38400, 4, 1, dict(fwd_ch=1, fwd_lds=153600, bwd_ch=4), "fast"),
    # dP 1 and 2 channels, several slices in every pass
    C("b1_slices", 1, 4, 17066, 2000, 4, 1, dict(fwd_ch=4, fwd_slices=8, red_slices=8, bwd_ch=1, lg=2), "fast"),
    C("all_slices_max", 1, 4, 17066, 38400, 4, 1, dict(fwd_ch=1, fwd_slices=8, red_slices=8, bwd_ch=1, pslices=18, lg=0),
      "fast"),
    C("b2_pslices_empty_lists", 1, 2, 8000, 30000, 4, 2, dict(fwd_ch=1, bwd_ch=2, pslices=14, fwd_slices=3, lg=0), "fast"),
    C("b2_gen_k7", 2, 6, 6000, 3000, 7, 3, dict(fwd_ch=4, bwd_ch=2, lg=1), "generic"),
    # the dP walk: lists empty, one lane, 8 lanes with long shares, hubs
    C("mostly_empty", 1, 8, 2000, 30000, 4, 4, dict(fwd_ch=1, bwd_ch=4, lg=0), "fast"),
    C("lg3_long_shares", 2, 16, 3000, 41, 4, 2, dict(fwd_ch=4, bwd_ch=4, lg=3), "fast"),
    C("hub_lg0", 1, 8, 4000, 3000, 4, 4, dict(fwd_ch=4, bwd_ch=4, lg=0), "fast", hub=True),
    C("hub_lg3", 1, 8, 3000, 60, 4, 4, dict(fwd_ch=4, bwd_ch=4, lg=3), "fast", hub=True),
    C("hub_gen", 1, 6, 3000, 500, 5, 6, dict(fwd_ch=4, bwd_ch=4, lg=2), "generic", hub=True),
    # k at the ends
    C("k255", 1, 4, 300, 2000, 255, 2, dict(fwd_ch=4, bwd_ch=4, lg=2), "generic"),
    C("k16", 2, 8, 2000, 4000, 16, 4, dict(fwd_ch=4, bwd_ch=4, lg=0), "generic", slope=0.0),
    # ties: small integers, so y, the sums and the selection are exact
    C("ties_k4", 2, 8, 3000, 500, 4, 4, dict(fwd_ch=4, bwd_ch=4, lg=1), "fast", data="int"),
    C("ties_k4_rem", 1, 7, 3000, 500, 4, 7, dict(fwd_ch=4, bwd_ch=4, lg=1), "rem", data="int", slope=0.0),
    C("ties_gen", 1, 6, 1000, 300, 7, 3, dict(fwd_ch=4, bwd_ch=4, lg=1), "generic", data="int"),
    C("ties_k255", 1, 2, 200, 50, 255, 1, dict(fwd_ch=4, bwd_ch=4, lg=3), "generic", data="int", slope=1.0),
    # GEOT_REPRODUCIBLE=0: the reverse index keeps its lists in arrival order -- dP within the same bound, not the same bits
    C("ties_k255_arrival_order", 1, 2, 200, 50, 255, 1, dict(fwd_ch=4, bwd_ch=4, lg=3), "generic", data="int", slope=1.0,
      reproducible="0"),
    # storage at 4-, 8- and 12-byte offsets (idx, P, Q and the incoming gradient): no int4 index loads
    C("offset4", 1, 8, 3000, 1000, 4, 4, dict(fwd_ch=4, k4=1), "generic", off=1),
    C("offset8", 1, 6, 3000, 6000, 4, 2, dict(fwd_ch=2, k4=1), "generic", off=2),
    C("offset12", 2, 4, 3000, 12000, 4, 4, dict(fwd_ch=1, k4=1), "generic", off=3),
    # far from zero
    C("mean100", 1, 8, 4096, 2048, 4, 4, dict(fwd_ch=4, fwd_slices=2), "fast", shift=100.0),
    C("mean1000", 1, 8, 4096, 2048, 4, 4, dict(fwd_ch=4, fwd_slices=2), "fast", shift=1000.0),
    C("mean1000_slices", 1, 4, 17066, 2000, 4, 1, dict(fwd_ch=4, fwd_slices=8), "fast", shift=-1000.0),
    C("mean1000_gen", 1, 6, 3000, 6000, 3, 3, dict(fwd_ch=2), "generic", shift=1000.0),
    C("opposite1000", 1, 8, 4096, 2048, 4, 4, dict(fwd_ch=4), "fast", opposite=1000.0),
] + [C("model_%d_%d_%d" % (c, nq, nk), 1, c, nq, nk, k, g, {}, "fast") for c, nq, nk, k, g in MODEL_SHAPES]


def _path(p, c, idx):
    if not p["k4"] or idx.data_ptr() % 16:
        return "generic"
    return "fast" if c % p["fwd_ch"] == 0 else "rem"


def _inputs(cs):
    b, c, nq, nk, k = cs["b"], cs["c"], cs["nq"], cs["nk"], cs["k"]
    gen = torch.Generator().manual_seed(b * 7919 + c * 131 + nq * 17 + nk * 3 + k)
    if cs.get("data") == "int":
        P = torch.randint(-3, 4, (b, c, nk), generator=gen).float()
        Q = torch.randint(-3, 4, (b, c, nq), generator=gen).float()
    else:
        P = torch.randn(b, c, nk, generator=gen) * 0.7
        Q = torch.randn(b, c, nq, generator=gen) * 0.7
    P += cs.get("shift", 0.0) + cs.get("opposite", 0.0)
    Q -= cs.get("opposite", 0.0)
    idx = torch.randint(0, nk, (b, nq, k), generator=gen, dtype=torch.int32)
    if cs.get("hub"):          # one source holds ~60 % of every cloud's pairs
        idx[torch.rand(b, nq, k, generator=gen) < 0.6] = nk // 3
    gm = torch.randn(c, generator=gen).clamp(-2.0, 2.0)
    gm[0] = 0.0
    if c > 1:
        gm[1] = -0.0
    if c > 2:
        gm[2] = -abs(float(gm[2])) - 0.1
    bt = torch.randn(c, generator=gen) * 0.5
    go = torch.randn(b, c, nq, generator=gen)
    return [t.to(DEV) for t in (P, Q, idx, gm, bt, go)]


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan") if dtype.is_floating_point else 255, dtype=dtype, device=DEV)


def _forward(lib, P, Q, idx, gm, bt, g, slope, ws):
    from geot_amd.ext._common import call, ptr
    b, c, nk = P.shape
    nq, k = idx.shape[1], idx.shape[2]
    out, ysel, ysum = _nan((b, c, nq)), _nan((b, c, nq)), _nan((b, c, nq))
    jsel, stats = _nan((b, c, nq), torch.uint8), _nan((b, g, 2))
    call("geot_edgeconv_gn_max", DEV, b, c, nq, nk, k, g, EPS, slope, ptr(P), ptr(Q), ptr(idx), ptr(gm), ptr(bt), ptr(out),
         ptr(ysel), ptr(ysum), ptr(jsel), ptr(stats), ptr(ws), ws.numel())
    return out, ysel, ysum, jsel, stats


def _backward(lib, P, Q, idx, gm, bt, g, slope, fw, go, ws, rix=None):
    from geot_amd.ext._common import call, ptr
    b, c, nk = P.shape
    nq, k = idx.shape[1], idx.shape[2]
    _, ysel, ysum, jsel, stats = fw
    gp, gq, gg, gb = _nan((b, c, nk)), _nan((b, c, nq)), _nan((c,)), _nan((c,))
    name, src = ("geot_edgeconv_gn_max_grad", idx) if rix is None else ("geot_edgeconv_gn_max_grad_rix", rix)
    call(name, DEV, b, c, nq, nk, k, g, slope, ptr(P), ptr(Q), ptr(src), ptr(gm), ptr(bt), ptr(ysel), ptr(ysum), ptr(jsel),
         ptr(stats), ptr(go), ptr(gp), ptr(gq), ptr(gg), ptr(gb), ptr(ws), ws.numel())
    return gp, gq, gg, gb


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.view(torch.uint8) if a.dtype == torch.uint8 else
                                                   a.contiguous().view(torch.int32), b.view(torch.uint8) if
                                                   b.dtype == torch.uint8 else b.contiguous().view(torch.int32)))


@pytest.mark.parametrize("cs", CASES)
def test_edgeconv_tail_against_fp64(cs, monkeypatch):
    from geot_amd import _lib
    from geot_amd.openpoints.models.backbone.transformer_ops import edgeconv_tail, edgeconv_reverse_index
    lib = _lib.load()
    b, c, nq, nk, k, g = (cs[x] for x in ("b", "c", "nq", "nk", "k", "g"))
    slope = cs.get("slope", 0.2)
    monkeypatch.setenv("GEOT_REPRODUCIBLE", cs.get("reproducible", "1"))
    ordered = cs.get("reproducible", "1") == "1"                # lists in arrival order: dP need not repeat bit for bit
    p = plan(lib, b, c, nq, nk, k, g)
    assert p is not None and all(p[key] == v for key, v in cs["want"].items()), (p, cs["want"])
    P0, Q0, idx0, gm, bt, go0 = _inputs(cs)
    off = cs.get("off", 0)
    P, Q, idx, go = (at_offset(t, off) if off else t for t in (P0, Q0, idx0, go0))
    assert _path(p, c, idx) == cs["path"]
    ws = torch.full((p["ws_bytes"],), 0xFF, dtype=torch.uint8, device=DEV)      # scratch: contents irrelevant

    fw = _forward(lib, P, Q, idx, gm, bt, g, slope, ws)
    fw2 = _forward(lib, P, Q, idx, gm, bt, g, slope, ws)
    gr = _backward(lib, P, Q, idx, gm, bt, g, slope, fw, go, ws)
    gr2 = _backward(lib, P, Q, idx, gm, bt, g, slope, fw, go, ws)
    rix = edgeconv_reverse_index(idx, nk)
    gr_rix = _backward(lib, P, Q, idx, gm, bt, g, slope, fw, go, ws, rix)
    # the autograd wrapper, on the same (possibly offset) storage
    pa, qa = P.detach().requires_grad_(True), Q.detach().requires_grad_(True)
    norm = torch.nn.GroupNorm(g, c, eps=EPS).to(DEV)
    with torch.no_grad():
        norm.weight.copy_(gm)
        norm.bias.copy_(bt)
    out_a = edgeconv_tail(pa, qa, idx, norm, slope)
    out_a.backward(go)
    torch.cuda.synchronize()
    for x, y in zip(fw, fw2):
        assert _same_bits(x, y), "forward does not repeat"
    for x, y, z in list(zip(gr, gr2, gr_rix))[0 if ordered else 1:]:
        assert _same_bits(x, y) and _same_bits(x, z), "gradient does not repeat / _grad_rix differs"
    for x, y in zip((fw[0], gr[0], gr[1], gr[2], gr[3]), (out_a, pa.grad, qa.grad, norm.weight.grad, norm.bias.grad)):
        assert _same_bits(x, y.detach()) or (x is gr[0] and not ordered), "edgeconv_tail differs from the C ABI"
    out, ysel, ysum, jsel, stats = fw
    gp, gq, gg, gb = gr
    for t in (out, ysel, ysum, stats, gp, gq, gg, gb):
        assert bool(torch.isfinite(t).all()), "an output left unwritten"

    # the side of the LeakyReLU the gradient kernels take: z = fmaf(gamma, (ysel - mean) * rstd, beta) in fp32 (its sign is
    # that of the exact gamma yh + beta, which fp64 gets right)
    st = stats.repeat_interleave(c // g, 1)
    yh32 = (ysel - st[..., 0:1]) * st[..., 1:2]
    pos_bwd = gm.double().view(1, c, 1) * yh32.double() + bt.double().view(1, c, 1) > 0
    far = "shift" in cs or "opposite" in cs
    ref = reference(P0, Q0, idx0, gm, bt, g, EPS, slope, go0, pos_hint=pos_bwd, kink=FAR_OUT_TOL if far else None)
    # selection: exact
    assert torch.equal(jsel.long(), ref["jsel"]), "selected slot"
    assert torch.equal(ysel.double(), ref["ysel"]), "selected y"
    ysum_err = (ysum.double() - ref["ysum"]).abs()
    if cs.get("data") == "int":
        assert float(ysum_err.max()) == 0.0
    else:
        assert bool((ysum_err <= gamma(k) * ref["y32"].double().abs().sum(-1)).all()), float(ysum_err.max())
    # statistics
    mean, rstd = stats[..., 0].double(), stats[..., 1].double()
    sd = ref["var"].sqrt()
    rstd_rel = float(((rstd - ref["rstd"]) / ref["rstd"]).abs().max())
    mean_err = float(((mean - ref["mean"]).abs() / (ref["mean"].abs() + sd)).max())
    assert rstd_rel <= 1e-5 and mean_err <= 1e-6, (rstd_rel, mean_err)

    got = dict(out=out, dp=gp, dq=gq, dgamma=gg, dbeta=gb)
    if far:
        assert float((out.double() - ref["out"]).abs().max()) <= FAR_OUT_TOL
        torch_res = dict(zip(("out", "dp", "dq", "dgamma", "dbeta"), composed_fp32(P0, Q0, idx0, gm, bt, g, EPS, slope, go0)))
        for name in ("dp", "dq", "dgamma", "dbeta"):
            scale = float(ref[name].abs().max())
            e_fused = float((got[name].double() - ref[name]).abs().max())
            e_torch = float((torch_res[name].double() - ref[name]).abs().max())
            assert e_fused <= 4 * e_torch + 1e-6 * scale, (name, e_fused, e_torch, scale)
        return

    # zero-centred data: the output from the statistics' error and the fp32 roundings of (y - mean) a + beta
    g64, b64 = gm.double().view(1, c, 1), bt.double().view(1, c, 1)
    rs = ref["rstd"].repeat_interleave(c // g, 1).view(b, c, 1)
    mu = ref["mean"].repeat_interleave(c // g, 1).view(b, c, 1)
    sdc = sd.repeat_interleave(c // g, 1).view(b, c, 1)
    ah = (g64 * (ref["ysel"] - mu) * rs).abs()
    out_tol = (E_STATS + 8 * U32) * (ah + b64.abs()) + g64.abs() * rs * 1e-6 * (mu.abs() + sdc) + 1e-30
    out_err = (out.double() - ref["out"]).abs()
    assert bool((out_err <= out_tol).all()), float((out_err / out_tol).max())
    assert float(out_err.max()) <= 2e-5 * float(ref["out"].abs().max())
    # gradients: the depth of each summation tree
    max_cnt = int(ref["cnt"].max())
    depth = dict(dp=math.ceil(max_cnt / (1 << p["lg"])) + p["lg"] + 6, dq=2 * k + 6,
                 dgamma=math.ceil(nq / p["red_slices"] / 256) + 12, dbeta=math.ceil(nq / p["red_slices"] / 256) + 12)
    for name in ("dp", "dq", "dgamma", "dbeta"):
        scale = float(ref[name].abs().max())
        err = (got[name].double() - ref[name]).abs()
        tol = torch.clamp((gamma(depth[name]) + E_STATS) * ref["abs"][name], max=2e-5 * scale) + 1e-30
        assert bool((err <= tol).all()), (name, float((err / tol).max()), float(err.max()), scale)


def test_model_shapes_are_the_models_calls(monkeypatch):
    """MODEL_SHAPES (pinned in test_edgeconv_plan_cpu.py) are what one forward of the configured model hands the tail"""
    from geot_amd.openpoints.models.backbone import transformer
    from geot_amd.openpoints.models.backbone.transformer import PointTransformer_seg_T, TOOTH_SEG_CFG
    from geot_amd.synth import make_batch
    seen = []
    real = transformer.edgeconv_tail

    def rec(p, q, idx, norm, slope, rix=None):
        seen.append((p.shape[1], q.shape[2], p.shape[2], idx.shape[2], norm.num_groups))
        return real(p, q, idx, norm, slope, rix)
    monkeypatch.setattr(transformer, "edgeconv_tail", rec)
    torch.manual_seed(0)
    model = PointTransformer_seg_T(**TOOTH_SEG_CFG).to(DEV)
    pos = torch.from_numpy(make_batch(1, 24000)[0]).to(DEV)
    cls = torch.zeros(1, 1, dtype=torch.long, device=DEV)
    with torch.no_grad():
        model(pos, pos.transpose(1, 2).contiguous(), cls)
    assert sorted(seen) == sorted(MODEL_SHAPES), seen
