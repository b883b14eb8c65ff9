"""Host side of the fused SetAbstraction kernel (geot_amd/csrc/sa_mlp.hip): folds an
eval-mode SharedMLP (pointnet2/pytorch_utils.py:8-33: conv1x1 -> BatchNorm -> ReLU) into
the padded parameter block the kernel expects and launches it."""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from .ext._common import f32, i32, same_device, need, call, ptr

_MAX_LAYERS = 4
_CACHE_ATTR = "_geot_sa_params"


def _pad_cols(c):
    return 32 if c <= 32 else 64 if c <= 64 else 128 if c <= 128 else 256


def _stages(mlp):
    """[(conv, bn or None, relu: bool)] or None if the stack is not a plain post-act SharedMLP: every stage is
    Conv2d(1x1, stride 1, padding 0, groups 1) [-> one BatchNorm2d with running statistics, in eval] [-> ReLU], in
    that order -- what pack_params can fold.  Anything else (pre-activation, a second norm, a norm after the ReLU, a
    BatchNorm that normalises with batch statistics) takes the composed path."""
    out = []
    for stage in mlp.children():
        mods = list(stage.children())
        if not mods or not isinstance(mods[0], nn.Conv2d):
            return None
        conv, bn, relu = mods[0], None, False
        if conv.kernel_size != (1, 1) or conv.stride != (1, 1) or conv.groups != 1 or conv.padding not in ((0, 0), "valid"):
            return None
        for m in mods[1:]:
            if isinstance(m, nn.Sequential) and len(m) == 1 and isinstance(m[0], nn.BatchNorm2d):
                m = m[0]
            if isinstance(m, nn.BatchNorm2d) and bn is None and not relu:
                if m.training or m.running_mean is None or m.running_var is None:
                    return None                 # batch statistics: nothing to fold
                bn = m
            elif isinstance(m, nn.ReLU) and not relu:
                relu = True
            else:
                return None
        out.append((conv, bn, relu))
    return out or None


def _plan_ok(c_feat, widths, nsample):
    """geot_sa_plan: does the kernel take this stack at this nsample (any b, npoint and CU count)"""
    arr = (ctypes.c_int * len(widths))(*widths)
    return _lib.load().geot_sa_plan(1, 1, nsample, c_feat, len(widths), arr, 1, 1, None, 0) == 1


def fused_sa_available(mlp, nsample=32):
    """True when the fused kernel launches for this stack AND this neighbourhood size (geot_sa_plan: nsample 8, 16 or
    a multiple of 32, widths up to 256, at most 4 layers, weights + activation tiles within the LDS); callers compose
    grouper + SharedMLP + max otherwise."""
    st = _stages(mlp)
    if not st or len(st) > _MAX_LAYERS:
        return False
    widths = [c.out_channels for c, _, _ in st]
    c_feat = st[0][0].in_channels - 3
    return c_feat >= 0 and _plan_ok(c_feat, widths, nsample)


@torch.no_grad()
def pack_params(mlp):
    """-> (params f32 device tensor, widths list, relu_mask, c_feat); BN folded with running stats."""
    st = _stages(mlp)
    need(bool(st), "SharedMLP layout not supported by the fused SA kernel")
    # what the fold reads: the tensors, and eps and the stage structure, which are no tensors
    key = tuple((p._version, p.data_ptr()) for p in mlp.parameters()) + \
        tuple((b._version, b.data_ptr()) for b in mlp.buffers()) + \
        tuple((id(conv), id(bn), None if bn is None else float(bn.eps), relu) for conv, bn, relu in st)
    cached = getattr(mlp, _CACHE_ATTR, None)
    if cached is not None and cached[0] == key:
        return cached[1]
    dev = st[0][0].weight.device
    c_feat = st[0][0].in_channels - 3
    kp = (3 + c_feat + 1) & ~1
    blocks, widths, relu_mask = [], [], 0
    for l, (conv, bn, relu) in enumerate(st):
        w = conv.weight.detach().float().reshape(conv.out_channels, conv.in_channels)
        b = conv.bias.detach().float() if conv.bias is not None else torch.zeros(conv.out_channels, device=dev)
        if bn is not None:     # affine=False: gamma = 1, beta = 0
            gamma = bn.weight.detach().float() if bn.weight is not None else torch.ones(conv.out_channels, device=dev)
            beta = bn.bias.detach().float() if bn.bias is not None else torch.zeros(conv.out_channels, device=dev)
            scale = gamma / torch.sqrt(bn.running_var.float() + bn.eps)
            w = w * scale[:, None]
            b = (b - bn.running_mean.float()) * scale + beta
        cp = _pad_cols(conv.out_channels)
        wt = torch.zeros((kp, cp), dtype=torch.float32, device=dev)
        wt[:conv.in_channels, :conv.out_channels] = w.t()
        bb = torch.zeros(cp, dtype=torch.float32, device=dev)
        bb[:conv.out_channels] = b
        blocks += [wt.reshape(-1), bb]
        widths.append(conv.out_channels)
        relu_mask |= int(relu) << l
        kp = cp
    res = (torch.cat(blocks).contiguous(), widths, relu_mask, c_feat)
    setattr(mlp, _CACHE_ATTR, (key, res))
    return res


def fused_group_mlp_max(xyz, new_xyz, features, idx, mlp, xyz_scale=1.0):
    """xyz (B,N,3), new_xyz (B,npoint,3), features (B,C,N), idx (B,npoint,nsample) i32
    -> (B, C_out, npoint) = max_s MLP([ (xyz[idx]-new_xyz)*scale ; features[idx] ])."""
    params, widths, relu_mask, c_feat = pack_params(mlp)
    f32(xyz, "xyz", 3); f32(new_xyz, "new_xyz", 3); i32(idx, "idx", 3)
    dev = same_device(xyz, new_xyz, idx, params)
    b, n, _ = xyz.shape
    npoint, nsample = idx.shape[1], idx.shape[2]
    if c_feat:
        f32(features, "features", 3)
        need(tuple(features.shape) == (b, c_feat, n), "features must be (B, %d, N)" % c_feat)
    need(tuple(new_xyz.shape) == (b, npoint, 3), "new_xyz shape mismatch")
    out = torch.empty((b, widths[-1], npoint), dtype=torch.float32, device=dev)
    warr = (ctypes.c_int * len(widths))(*widths)
    call("geot_sa_group_mlp_max", dev, b, n, npoint, nsample, c_feat, ptr(xyz), ptr(new_xyz),
         ptr(features) if c_feat else None, ptr(idx), float(xyz_scale), len(widths), warr, relu_mask,
         ptr(params), ptr(out))
    return out
