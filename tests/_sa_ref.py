"""Shared by the fused SetAbstraction tests (csrc/sa_mlp.hip through geot_sa_* and geot_amd/sa_fused.py): the launch plan as
a dict, a restatement of the launcher as it stood before the plan was pulled out of it, SharedMLP stacks of every foldable
form, an fp64 reference of the whole body with a propagated error bound, and a recorder of the fused launches.

The reference takes the layer-0 input as the kernel forms it, (p - q) * xyz_scale in fp32 (two correctly rounded
operations: the kernel's own values to the bit), and everything after that in fp64 through the UNFOLDED stages: conv +
bias, BatchNorm with its running statistics and eps, ReLU, max over nsample.  The kernel runs the folded stack
W' = W gamma / sqrt(var + eps), b' = (b - mean) gamma / sqrt(var + eps) + beta on fp32 MFMA (an fma chain of depth K_l,
the padded input width, from the bias).  Per layer

    err_l = |W'_l| err_{l-1} + u (K_l + C_MFMA) (|W'_l| (|a_{l-1}| + err_{l-1}) + |b'_l|)
                             + u C_FOLD (|W'_l| (|a_{l-1}| + err_{l-1}) + |b - mean| |s| + |beta|)

with u = 2^-24: Higham's bound of an fma chain, and the fold's own roundings (s = gamma / sqrt(var + eps) takes 3, W' 1 more,
b' 3 more; C_FOLD = 8 covers them with room).  ReLU and max are 1-Lipschitz, so the bound passes through them; the pooled
bound is the largest row bound of the group.  err_0 = 0."""
import ctypes

import torch
import torch.nn as nn

U32 = 2.0 ** -24
C_MFMA = 2          # the bias initialisation and the chain's last rounding
C_FOLD = 8
LDS_CU = 160 * 1024
MAX_LAYERS = 4

PLAN_FIELDS = (("wide", "waves", "lds", "blocks", "gpt", "tpg", "fast_np", "run_len", "nunits", "param_floats",
                "act_stride") + tuple("kp%d" % l for l in range(4)) + tuple("cp%d" % l for l in range(4)) +
               tuple("woff%d" % l for l in range(4)) + tuple("boff%d" % l for l in range(4)))

# BASELINE configs[1] (bench.py --workload sa): one cloud, 24 000 -> 6000 points, nsample 32, SharedMLP [3 + 3, 64, 64, 128]
BENCH_SA = dict(b=1, n=24000, npoint=6000, nsample=32, c_feat=3, widths=(64, 64, 128))


def pad_cols(c):
    return 32 if c <= 32 else 64 if c <= 64 else 128 if c <= 128 else 256


def plan(lib, b, npoint, nsample, c_feat, widths, cus=256, aligned=True):
    """geot_sa_plan as a dict, or None where the kernel refuses the shape"""
    arr = (ctypes.c_int * max(1, len(widths)))(*widths)
    out = (ctypes.c_longlong * len(PLAN_FIELDS))()
    if lib.geot_sa_plan(b, npoint, nsample, c_feat, len(widths), arr, cus, int(aligned), out, len(PLAN_FIELDS)) != 1:
        return None
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def legacy_plan(b, npoint, nsample, c_feat, widths, cus=256, aligned=True):
    """geot_sa_group_mlp_max's launch decisions as the launcher made them in place before geot_sa_plan existed (without
    the GEOT_SA_FAST / GEOT_SA_RUN overrides), restated; None where it refused.  b * npoint == 0 returned before any
    of this; the plan reports 0 workgroups there."""
    nl = len(widths)
    if b < 0 or npoint < 0 or nl < 1 or nl > MAX_LAYERS or c_feat < 0:
        return None
    if not (nsample in (8, 16) or (nsample >= 32 and nsample % 32 == 0)):
        return None
    if any(w < 1 or w > 256 for w in widths):
        return None
    kp, off, maxw = (3 + c_feat + 1) & ~1, 0, (3 + c_feat + 1) & ~1
    p = {k: 0 for k in PLAN_FIELDS}
    for l, w in enumerate(widths):
        cp = pad_cols(w)
        p["kp%d" % l], p["cp%d" % l], p["woff%d" % l] = kp, cp, off
        off += kp * cp
        p["boff%d" % l] = off
        off += cp
        if l + 1 < nl and cp > maxw:
            maxw = cp
        kp = cp
    gpt = 1 if nsample >= 32 else 32 // nsample
    wide = any(pad_cols(w) > 128 for w in widths)
    per_wave = 32 * (maxw + 1) + gpt * pad_cols(widths[-1])
    waves = 8 if wide else 12
    while waves > 4 and (off + waves * per_wave) * 4 > LDS_CU:
        waves -= 4
    lds = (off + waves * per_wave) * 4
    if lds > LDS_CU:
        return None
    nunits = (b * npoint + gpt - 1) // gpt
    blocks = min((nunits + waves - 1) // waves, cus)
    c_last = widths[-1]
    fast_np = c_last // 64 if (nsample == 32 and c_feat <= 8 and c_last == pad_cols(c_last) and c_last >= 64 and
                               b * npoint < 0x7fffffff and b * npoint * 32 < 0x7fffffff * 4) else 0
    run_len = 8 if (fast_np and npoint % 8 == 0 and aligned and nunits >= 16 * blocks * waves) else 1
    p.update(wide=int(wide), waves=waves, lds=lds, blocks=blocks, gpt=gpt, tpg=nsample // 32 if nsample >= 32 else 1,
             fast_np=fast_np, run_len=run_len, nunits=nunits, param_floats=off, act_stride=maxw + 1)
    return p


def make_mlp(c_in, widths, bn=True, relu=True, bias=None, affine=True, seed=0, device="cuda:0"):
    """nn.Sequential of nn.Sequential(Conv2d 1x1 [, BatchNorm2d] [, ReLU]) stages in eval; bn / relu / bias: one bool for
    every stage or a list.  BatchNorm gets running statistics, weights and biases well away from the identity (some
    gammas negative)."""
    nl = len(widths)

    def per(v):
        return list(v) if isinstance(v, (list, tuple)) else [v] * nl
    bn, relu = per(bn), per(relu)
    bias = [not x for x in bn] if bias is None else per(bias)
    g = torch.Generator().manual_seed(seed)
    stages = []
    cin = c_in
    for l, w in enumerate(widths):
        conv = nn.Conv2d(cin, w, 1, bias=bias[l])
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / cin ** 0.5)
            if conv.bias is not None:
                conv.bias.copy_(torch.randn(w, generator=g) * 0.3)
        mods = [conv]
        if bn[l]:
            norm = nn.BatchNorm2d(w, affine=affine, eps=1e-5 * (1 + l))
            with torch.no_grad():
                norm.running_mean.copy_(torch.randn(w, generator=g) * 0.3)
                norm.running_var.copy_(torch.rand(w, generator=g) + 0.5)
                if affine:
                    norm.weight.copy_((torch.rand(w, generator=g) + 0.5) * torch.where(torch.rand(w, generator=g) < 0.15, -1.0, 1.0))
                    norm.bias.copy_(torch.randn(w, generator=g) * 0.2)
            mods.append(norm)
        if relu[l]:
            mods.append(nn.ReLU(inplace=True))
        stages.append(nn.Sequential(*mods))
        cin = w
    return nn.Sequential(*stages).to(device).eval()


def layer0_input(xyz, new_xyz, features, idx, xyz_scale):
    """the kernel's layer-0 rows as fp32 (b, npoint, nsample, 3 + c): (xyz[idx] - centre) * xyz_scale, features[:, idx]"""
    b, n, _ = xyz.shape
    npoint, ns = idx.shape[1], idx.shape[2]
    li = idx.long().reshape(b, npoint * ns)
    p = torch.gather(xyz, 1, li.unsqueeze(-1).expand(-1, -1, 3)).view(b, npoint, ns, 3)
    d = (p - new_xyz.unsqueeze(2)) * torch.tensor(xyz_scale, dtype=torch.float32)
    if features is None or features.shape[1] == 0:
        return d
    c = features.shape[1]
    f = torch.gather(features, 2, li.unsqueeze(1).expand(-1, c, -1)).view(b, c, npoint, ns).permute(0, 2, 3, 1)
    return torch.cat([d, f], -1)


def _stage_terms(conv, norm):
    """fp64 (W (cout, cin), bias (cout), s (cout), shift (cout), |b - mean| |s| + |beta|) of one unfolded stage:
    y = s (W a + bias) + shift; W' = s W is what the kernel holds"""
    w = conv.weight.detach().double().reshape(conv.out_channels, conv.in_channels)
    b = conv.bias.detach().double() if conv.bias is not None else torch.zeros(conv.out_channels, dtype=torch.float64, device=w.device)
    if norm is None:
        one = torch.ones_like(b)
        return w, b, one, torch.zeros_like(b), torch.zeros_like(b)
    gamma = norm.weight.detach().double() if norm.weight is not None else torch.ones_like(b)
    beta = norm.bias.detach().double() if norm.bias is not None else torch.zeros_like(b)
    s = gamma / torch.sqrt(norm.running_var.double() + norm.eps)
    shift = beta - norm.running_mean.double() * s
    return w, b, s, shift, (b - norm.running_mean.double()).abs() * s.abs() + beta.abs()


def reference(xyz, new_xyz, features, idx, mlp, xyz_scale=1.0, chunk_rows=1 << 16):
    """fp64 (b, c_out, npoint) and its error bound (same shape) for the fused kernel's output; mlp = the unfolded stack"""
    from geot_amd.sa_fused import _stages
    st = _stages(mlp)
    assert st, "not a foldable stack"
    a0 = layer0_input(xyz, new_xyz, features, idx, xyz_scale)
    b, npoint, ns, k0 = a0.shape
    terms = [_stage_terms(conv, norm) for conv, norm, _ in st]
    kps = [(3 + (k0 - 3) + 1) & ~1] + [pad_cols(conv.out_channels) for conv, _, _ in st[:-1]]
    c_out = st[-1][0].out_channels
    rows = a0.reshape(-1, ns, k0)
    gchunk = max(1, chunk_rows // ns)
    out = torch.empty(rows.shape[0], c_out, dtype=torch.float64, device=xyz.device)
    bound = torch.empty_like(out)
    for g0 in range(0, rows.shape[0], gchunk):
        a = rows[g0:g0 + gchunk].double()
        err = torch.zeros_like(a)
        for (conv, norm, relu), (w, bias, s, shift, fold_b), kp in zip(st, terms, kps):
            wf = (w * s[:, None]).t()                 # W'^T (cin, cout)
            y = (a @ w.t() + bias) * s + shift
            aw = (a.abs() + err) @ wf.abs()
            bf = (bias * s + shift).abs()
            err = err @ wf.abs() + U32 * (kp + C_MFMA) * (aw + bf) + U32 * C_FOLD * (aw + fold_b)
            a = torch.relu(y) if relu else y
        out[g0:g0 + gchunk] = a.amax(1)
        bound[g0:g0 + gchunk] = err.amax(1)
    return (out.view(b, npoint, c_out).permute(0, 2, 1).contiguous(),
            bound.view(b, npoint, c_out).permute(0, 2, 1).contiguous())


def composed(xyz, new_xyz, features, idx, mlp, xyz_scale=1.0):
    """the torch composition the kernel replaces, fp32: grouped (b, 3 + c, npoint, nsample) -> mlp -> max over nsample"""
    a0 = layer0_input(xyz, new_xyz, features, idx, xyz_scale).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        return mlp(a0).max(-1)[0]


def assert_within(got, ref, bound, what=""):
    """|got - ref| <= bound elementwise (got fp32, ref / bound fp64), NaN where ref is NaN, equal infinities"""
    g = got.double()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(g), nan), "%s: NaN mask differs (%d vs %d)" % (what, int(torch.isnan(g).sum()), int(nan.sum()))
    inf = torch.isinf(ref)
    assert torch.equal(g[inf], ref[inf]) and not torch.isinf(g[~inf]).any(), "%s: infinities differ" % what
    fin = ~(nan | inf)
    diff = (g[fin] - ref[fin]).abs()
    over = diff > bound[fin]
    assert not over.any(), "%s: %d of %d over the bound, worst |err| %.3g at bound %.3g" % (
        what, int(over.sum()), diff.numel(), float(diff.max()), float(bound[fin][diff.argmax()]))


class SaLaunches:
    """records the C-ABI entry points sa_fused launched (monkeypatched over sa_fused.call)"""

    def __init__(self, monkeypatch):
        from geot_amd import sa_fused
        self.names = []
        real = sa_fused.call

        def rec(name, dev, *args):
            self.names.append(name)
            return real(name, dev, *args)
        monkeypatch.setattr(sa_fused, "call", rec)

    def take(self):
        names, self.names = self.names, []
        return names
