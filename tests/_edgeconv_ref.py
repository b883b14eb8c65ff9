"""Shared by the fused EdgeConv tail tests (csrc/edgeconv.hip through geot_edgeconv_* and transformer_ops.edgeconv_tail):
the launch plan as a dict, the model's call shapes, and an fp64 reference of the whole tail.

The reference takes the selection from the fp32 sums y32 = P[idx] + Q -- one correctly rounded add, so it is the kernel's
own y to the bit -- with the kernel's rule: the FIRST extremum over the k slots, the maximum where gamma >= 0 (0 and -0.0
included) and the minimum where gamma < 0.  Everything after that is fp64: the GroupNorm statistics of y32, the output,
and the gradients through a gather at the chosen slot."""
import ctypes

import torch

PLAN_FIELDS = ("fwd_ch", "fwd_slices", "fwd_lds", "k4", "red_slices", "bwd_ch", "pslices", "bwd_lds", "lg", "rec",
               "part_floats", "coef_off", "rix_off", "ws_bytes")

# (c, nq, nk, k, groups) of the four calls per step, DGCNN_Propagation's two modules x two layers: dgcnn_pro_2 on 4096
# queries among the 512 group centres and then among themselves, dgcnn_pro_1 on 8192 queries among those 4096 and then
# among themselves (TOOTH_SEG_CFG's downsample_targets).  test_edgeconv_gpu.py records them from a forward of the model.
MODEL_SHAPES = ((512, 4096, 512, 4, 4), (384, 4096, 4096, 4, 4), (512, 8192, 4096, 4, 4), (384, 8192, 8192, 4, 4))


def plan(lib, b, c, nq, nk, k, groups):
    """geot_edgeconv_plan as a dict, or None where the shape is not eligible"""
    out = (ctypes.c_longlong * len(PLAN_FIELDS))()
    if lib.geot_edgeconv_plan(b, c, nq, nk, k, groups, out, len(PLAN_FIELDS)) != 1:
        return None
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def first_extremum(y, want_max):
    """(b, c, nq, k), (c,) bool -> int64 (b, c, nq, 1): the first slot holding the row's maximum (want_max) or minimum"""
    ext = torch.where(want_max.view(1, -1, 1, 1), y.amax(-1, keepdim=True), y.amin(-1, keepdim=True))
    slots = torch.arange(y.shape[-1], device=y.device).expand_as(y)
    return torch.where(y == ext, slots, y.shape[-1]).amin(-1, keepdim=True)


def reference(P, Q, idx, gamma, beta, groups, eps, slope, go, pos_hint=None, kink=None):
    """fp64 forward and backward of the tail; P, Q, gamma, beta, go fp32 on the GPU, idx int32.  Also returns, per
    gradient, the sum of the magnitudes of the terms the kernel adds up (the scale of its rounding error).  pos_hint
    (b, c, nq) bool: the side of the LeakyReLU the gradient kernels took, used where the fp64 pre-activation lies within `kink` of 0
    (the output's tolerance: an fp32 pre-activation that close may fall on either side; default 1e-5 of its terms).  The
    side of one element moves the group's gradient coefficients too, so the reference has to follow the kernel there."""
    b, c, nk = P.shape
    nq, k = idx.shape[1], idx.shape[2]
    gi = idx.long().reshape(b, 1, nq * k).expand(-1, c, -1)
    y32 = torch.gather(P, 2, gi).view(b, c, nq, k) + Q.unsqueeze(-1)
    j = first_extremum(y32, gamma >= 0)
    y = y32.double()
    yg = y.view(b, groups, -1)
    mean_g, var_g = yg.mean(-1), yg.var(-1, unbiased=False)
    rstd_g = 1.0 / torch.sqrt(var_g + eps)
    cpg = c // groups
    mean = mean_g.repeat_interleave(cpg, 1).view(b, c, 1)
    rstd = rstd_g.repeat_interleave(cpg, 1).view(b, c, 1)
    g64, b64 = gamma.double().view(1, c, 1), beta.double().view(1, c, 1)
    ysel = torch.gather(y, 3, j).squeeze(-1)
    yh_sel = (ysel - mean) * rstd
    z = g64 * yh_sel + b64
    pos = z > 0
    if pos_hint is not None:
        band = 1e-5 * ((g64 * yh_sel).abs() + b64.abs()) if kink is None else kink
        pos = torch.where(z.abs() <= band, pos_hint, pos)
    out = torch.where(pos, z, slope * z)
    dz = go.double() * torch.where(pos, 1.0, float(slope))
    a = g64 * dz                                                        # d/d yhat at the chosen slot
    dyh = torch.zeros_like(y).scatter_(3, j, a.unsqueeze(-1))
    yh = (y - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)
    s1 = dyh.view(b, groups, -1).mean(-1).repeat_interleave(cpg, 1).view(b, c, 1)
    s2 = (dyh * yh).view(b, groups, -1).mean(-1).repeat_interleave(cpg, 1).view(b, c, 1)
    dy = rstd.unsqueeze(-1) * (dyh - s1.unsqueeze(-1) - yh * s2.unsqueeze(-1))
    dq = dy.sum(-1)
    dp = torch.zeros(b, c, nk, dtype=torch.float64, device=P.device).scatter_add_(2, gi, dy.reshape(b, c, nq * k))
    dgamma = (dz * yh_sel).sum((0, 2))
    dbeta = dz.sum((0, 2))
    # the kernel's terms: dP[n] = rstd (sum_pairs (a_i [j == jsel] + u_i) - cnt (s1 + s2 rstd (P_n - mean))), u_i = -s2 rstd Q_i;
    # dQ[i] = rstd (a_i - k s1 - s2 rstd (ysum_i - k mean))
    u = (s2 * rstd * Q.double()).abs()
    pair_terms = dyh.abs().reshape(b, c, nq * k) + u.unsqueeze(-1).expand(-1, -1, -1, k).reshape(b, c, nq * k)
    cnt = torch.zeros(b, nk, dtype=torch.float64, device=P.device).scatter_add_(
        1, idx.long().reshape(b, nq * k), torch.ones(b, nq * k, dtype=torch.float64, device=P.device)).unsqueeze(1)
    dp_abs = rstd * (torch.zeros_like(dp).scatter_add_(2, gi, pair_terms) +
                     cnt * (s1.abs() + (s2 * rstd).abs() * (P.double() - mean).abs()))
    dq_abs = rstd * (a.abs() + k * s1.abs() + (s2 * rstd).abs() * (y.abs().sum(-1) + k * mean.abs()))
    return dict(out=out, ysel=ysel, ysum=y.sum(-1), jsel=j.squeeze(-1), mean=mean_g, rstd=rstd_g, var=var_g,
                dp=dp, dq=dq, dgamma=dgamma, dbeta=dbeta, y32=y32, cnt=cnt,
                abs=dict(dp=dp_abs, dq=dq_abs, dgamma=(dz * yh_sel).abs().sum((0, 2)), dbeta=dz.abs().sum((0, 2))))


def composed_fp32(P, Q, idx, gamma, beta, groups, eps, slope, go):
    """the torch composition the fused tail replaces (transformer.py's grouping + GroupNorm + LeakyReLU + max), in fp32:
    (out, dP, dQ, dgamma, dbeta)"""
    b, c, nk = P.shape
    nq, k = idx.shape[1], idx.shape[2]
    p, q = P.clone().requires_grad_(True), Q.clone().requires_grad_(True)
    norm = torch.nn.GroupNorm(groups, c, eps=eps).to(P.device)
    with torch.no_grad():
        norm.weight.copy_(gamma)
        norm.bias.copy_(beta)
    y = torch.gather(p, 2, idx.long().reshape(b, 1, nq * k).expand(-1, c, -1)).view(b, c, nq, k) + q.unsqueeze(-1)
    out = torch.nn.functional.leaky_relu(norm(y), slope).max(dim=-1)[0]
    (out * go).sum().backward()
    return out.detach(), p.grad, q.grad, norm.weight.grad, norm.bias.grad
