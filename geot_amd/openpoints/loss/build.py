"""The criteria train_one_epoch has a branch for (examples/segmentation/train.py:449-454, 576-596): the two the shipped
cfg configures (cfgs/tooth_semi/transformer_finetune_fixmatch_ntm.yaml criterion_args / criterion_u_args) --
Poly1FocalLoss (openpoints/loss/build.py:183-258) on the labelled clouds, Poly1FocalLoss_U_corr (:799-892) on the
NTM-corrected strong-view logits -- and the alternatives its comments list (yaml :51, :54): Weight_CELoss (:913-925, the
loss the teacher checkpoint was pretrained with), Weight_CELoss_U (:928-938), Poly1FocalLoss_U (:261-354) and
Poly1FocalLoss_U_T (:564-688).  Same constructor arguments and forward signatures, same arithmetic; on (B, C, N) fp32
CUDA logits with int64 labels each runs as fused kernels (csrc/loss.hip), otherwise as a torch composite that restates
the reference's statements.  build_criterion_from_cfg({"NAME": ...}) resolves them by name."""
import os

import torch
import torch.nn.functional as F
from torch.autograd import Function

from ... import _lib


class _Poly1FocalFn(Function):
    """csrc/loss.hip: the loss from integer labels in two launches, its gradient in one."""

    @staticmethod
    def forward(ctx, logits, labels, keep, alpha, gamma, epsilon):
        from ...ext._common import call, ptr
        b, c, n = logits.shape
        ws = torch.empty(int(_lib.load().geot_poly1_focal_ws_doubles(b, c, n)), dtype=torch.float64, device=logits.device)
        out2 = torch.empty(2, dtype=torch.float32, device=logits.device)
        call("geot_poly1_focal", logits.device, b, c, n, float(alpha), float(gamma), float(epsilon), ptr(logits), ptr(labels),
             ptr(keep), ptr(ws), ptr(out2))
        ctx.save_for_backward(logits, labels, keep, out2)
        ctx.cfg = (float(alpha), float(gamma), float(epsilon))
        return out2[0]

    @staticmethod
    def backward(ctx, g):
        from ...ext._common import call, ptr
        logits, labels, keep, out2 = ctx.saved_tensors
        b, c, n = logits.shape
        up = g.reshape(1).float().contiguous()
        grad = torch.empty_like(logits)
        call("geot_poly1_focal_grad", logits.device, b, c, n, *ctx.cfg, ptr(logits), ptr(labels), ptr(keep), ptr(out2), ptr(up),
             ptr(grad))
        return grad, None, None, None, None, None


def _check_labels(logits, labels):
    """GEOT_CHECK_LABELS=1: the synchronous range check F.one_hot does in the reference (openpoints/loss/build.py:223-230
    raise on a label outside [0, C)).  Off by default -- it costs a device round trip per call; without it the fused
    kernel returns NaN for such input (csrc/loss.hip) instead of a silently different loss."""
    if os.environ.get("GEOT_CHECK_LABELS", "0") == "1" and labels.numel():
        lo, hi = int(labels.min()), int(labels.max())
        if lo < 0:
            raise RuntimeError("Class values must be non-negative.")
        if hi >= logits.shape[1]:
            raise RuntimeError("Class values must be smaller than num_classes.")


def _fused_ok(mod, logits, labels, reduction_ok):
    return (reduction_ok and not mod.label_is_onehot and mod.weight is None and mod.pos_weight is None and logits.is_cuda
            and logits.dtype == torch.float32 and logits.dim() == 3 and labels.dim() == 2 and labels.dtype == torch.int64
            and tuple(labels.shape) == (logits.shape[0], logits.shape[2]) and logits.numel() > 0
            and logits.shape[0] <= 65535 and logits.shape[1] <= 65535)


def _one_hot_like(logits, labels):
    if labels.ndim == 1:
        labels = F.one_hot(labels, num_classes=logits.shape[1])
    else:
        labels = F.one_hot(labels.unsqueeze(1), logits.shape[1]).transpose(1, -1).squeeze(-1)
    return labels.to(device=logits.device, dtype=logits.dtype)


def _poly1(logits, labels, weight, pos_weight, alpha, gamma, epsilon):
    p = torch.sigmoid(logits)
    ce = F.binary_cross_entropy_with_logits(input=logits, target=labels, reduction="none", weight=weight,
                                            pos_weight=pos_weight)
    pt = labels * p + (1 - labels) * (1 - p)
    fl = ce * ((1 - pt) ** gamma)
    if alpha >= 0:
        fl = (alpha * labels + (1 - alpha) * (1 - labels)) * fl
    return fl + epsilon * torch.pow(1 - pt, gamma + 1)


class Poly1FocalLoss(torch.nn.Module):
    def __init__(self, epsilon=1.0, alpha=0.25, gamma=2.0, reduction="mean", weight=None, pos_weight=None,
                 label_is_onehot=False, **kwargs):
        super().__init__()
        self.epsilon, self.alpha, self.gamma, self.reduction = epsilon, alpha, gamma, reduction
        self.weight, self.pos_weight, self.label_is_onehot = weight, pos_weight, label_is_onehot

    def forward(self, logits, labels):
        if _fused_ok(self, logits, labels, self.reduction == "mean"):
            _check_labels(logits, labels)
            return _Poly1FocalFn.apply(logits.contiguous(), labels.contiguous(), None, self.alpha, self.gamma, self.epsilon)
        if not self.label_is_onehot:
            labels = _one_hot_like(logits, labels)
        poly1 = _poly1(logits, labels.to(logits.dtype), self.weight, self.pos_weight, self.alpha, self.gamma, self.epsilon)
        if self.reduction == "mean":
            return poly1.mean()
        return poly1.sum() if self.reduction == "sum" else poly1


class Poly1FocalLoss_U_corr(Poly1FocalLoss):
    def forward(self, logits, labels, logits_pred, thresh=0.95, mask=None):
        # a soft (float) mask multiplies the loss by its VALUES in the reference (:872-875): only a 0/1 mask is a `keep` flag
        hard_mask = mask is None or mask.dtype in (torch.bool, torch.uint8)
        if hard_mask and _fused_ok(self, logits, labels, True):
            _check_labels(logits, labels)
            keep = (mask if mask is not None else logits_pred.ge(thresh)).to(torch.uint8).contiguous()
            if tuple(keep.shape) == tuple(labels.shape):
                return _Poly1FocalFn.apply(logits.contiguous(), labels.contiguous(), keep, self.alpha, self.gamma, self.epsilon)
        if not self.label_is_onehot:
            labels = _one_hot_like(logits, labels)
        poly1 = _poly1(logits, labels.to(logits.dtype), self.weight, self.pos_weight, self.alpha, self.gamma, self.epsilon)
        keep = mask if mask is not None else logits_pred.ge(thresh)
        keep = keep.unsqueeze(1).to(poly1.dtype)                      # broadcast over the class axis (:872-875)
        return torch.sum(poly1 * keep) / (keep.sum() * poly1.shape[1] + 0.001)


class Poly1FocalLoss_U(Poly1FocalLoss_U_corr):
    """openpoints/loss/build.py:261-354: the body of Poly1FocalLoss_U_corr under its own name (train.py:588-590 hands it the
    UNcorrected strong-view logits)."""


class _Poly1FocalBetaFn(Function):
    """csrc/loss.hip geot_poly1_focal_beta: Poly1FocalLoss_U_T in two launches, both gradients in one."""

    @staticmethod
    def forward(ctx, logits, labels, keep, conf, t, alpha, gamma, epsilon):
        from ...ext._common import call, ptr
        b, c, n = logits.shape
        ws = torch.empty(int(_lib.load().geot_poly1_focal_ws_doubles(b, c, n)), dtype=torch.float64, device=logits.device)
        out2 = torch.empty(2, dtype=torch.float32, device=logits.device)
        call("geot_poly1_focal_beta", logits.device, b, c, n, float(alpha), float(gamma), float(epsilon), ptr(logits),
             ptr(labels), ptr(keep), ptr(conf), ptr(t), ptr(ws), ptr(out2))
        ctx.save_for_backward(logits, labels, keep, conf, t, out2)
        ctx.cfg = (float(alpha), float(gamma), float(epsilon))
        return out2[0]

    @staticmethod
    def backward(ctx, g):
        from ...ext._common import call, ptr
        logits, labels, keep, conf, t, out2 = ctx.saved_tensors
        b, c, n = logits.shape
        up = g.reshape(1).float().contiguous()
        grad, grad_t = torch.empty_like(logits), torch.empty_like(t)
        call("geot_poly1_focal_beta_grad", logits.device, b, c, n, *ctx.cfg, ptr(logits), ptr(labels), ptr(keep), ptr(conf),
             ptr(t), ptr(out2), ptr(up), ptr(grad), ptr(grad_t))
        return grad, None, None, None, grad_t, None, None, None


class Poly1FocalLoss_U_T(Poly1FocalLoss):
    """openpoints/loss/build.py:564-688: the masked Poly-1 focal loss with every point's terms multiplied by
    beta = logits_pred / pred_u_t[b, label, n] (train.py:594-596 passes the confidence and the corrected strong-view
    logits); differentiable w.r.t. `logits` and `pred_u_t`.  `T` is accepted and unused, as there."""

    def forward(self, logits, labels, logits_pred, T, pred_u_t, thresh=0.95, mask=None):
        hard_mask = mask is None or mask.dtype in (torch.bool, torch.uint8)
        if (hard_mask and _fused_ok(self, logits, labels, True) and logits.shape[1] <= MAX_FUSED_CLASSES
                and _plain_f32(logits_pred, labels.shape, logits.device) and _f32_like(pred_u_t, logits)):
            _check_labels(logits, labels)
            keep = (mask if mask is not None else logits_pred.ge(thresh)).to(torch.uint8).contiguous()
            if tuple(keep.shape) == tuple(labels.shape):
                return _Poly1FocalBetaFn.apply(logits.contiguous(), labels.contiguous(), keep, logits_pred.contiguous(),
                                               pred_u_t.contiguous(), self.alpha, self.gamma, self.epsilon)
        num_classes = logits.shape[1]
        label_raw = labels
        if not self.label_is_onehot:
            labels = _one_hot_like(logits, labels)
        poly1 = _poly1(logits, labels.to(logits.dtype), self.weight, self.pos_weight, self.alpha, self.gamma, self.epsilon)
        batch_size, num_point = label_raw.shape
        flat = pred_u_t.transpose(1, 2).contiguous().view(-1)                                       # BNC (:656)
        index = torch.arange(batch_size * num_point, device=flat.device).long() * num_classes + label_raw.contiguous().view(-1)
        beta = (logits_pred / flat[index].view(batch_size, num_point)).unsqueeze(1)                 # (:663-665)
        poly1 = poly1 * beta
        keep = mask if mask is not None else logits_pred.ge(thresh)
        keep = keep.unsqueeze(1).to(poly1.dtype)
        return torch.sum(poly1 * keep) / (keep.sum() * poly1.shape[1] + 0.001)


MAX_FUSED_CLASSES = _lib.NTM_MAX_C      # include/geot_hip.h GEOT_NTM_MAX_C: the class cap of the library's per-point kernels


def _plain_f32(t, shape, device):
    return (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == device and tuple(t.shape) == tuple(shape)
            and not t.requires_grad)


def _f32_like(t, like):
    return torch.is_tensor(t) and t.dtype == torch.float32 and t.device == like.device and t.shape == like.shape


class _WeightedCEFn(Function):
    """csrc/loss.hip geot_weighted_ce: the loss from integer labels in two launches, its gradient in one."""

    @staticmethod
    def forward(ctx, logits, labels, class_weights, conf, thresh):
        from ...ext._common import call, ptr
        b, c, n = logits.shape
        bw = class_weights.shape[0]
        ws = torch.empty(int(_lib.load().geot_weighted_ce_ws_doubles(b, c, n)), dtype=torch.float64, device=logits.device)
        out2 = torch.empty(2, dtype=torch.float32, device=logits.device)
        call("geot_weighted_ce", logits.device, b, c, n, bw, float(thresh), ptr(logits), ptr(labels), ptr(class_weights),
             ptr(conf), ptr(ws), ptr(out2))
        ctx.save_for_backward(logits, labels, class_weights, conf, out2)
        ctx.thresh = float(thresh)
        return out2[0]

    @staticmethod
    def backward(ctx, g):
        from ...ext._common import call, ptr
        logits, labels, class_weights, conf, out2 = ctx.saved_tensors
        b, c, n = logits.shape
        up = g.reshape(1).float().contiguous()
        grad = torch.empty_like(logits)
        call("geot_weighted_ce_grad", logits.device, b, c, n, class_weights.shape[0], ctx.thresh, ptr(logits), ptr(labels),
             ptr(class_weights), ptr(conf), ptr(out2), ptr(up), ptr(grad))
        return grad, None, None, None, None


def _wce_fused_ok(ret, gt, class_weights):
    return (ret.is_cuda and ret.dtype == torch.float32 and ret.dim() == 3 and gt.dim() == 2 and gt.dtype == torch.int64
            and tuple(gt.shape) == (ret.shape[0], ret.shape[2]) and ret.numel() > 0 and ret.shape[0] <= 65535
            and ret.shape[1] <= MAX_FUSED_CLASSES and gt.device == ret.device and torch.is_tensor(class_weights)
            and class_weights.dtype == torch.float32 and class_weights.device == ret.device and class_weights.dim() == 2
            and class_weights.shape[0] >= 1 and class_weights.shape[1] == ret.shape[1] and not class_weights.requires_grad)


def _check_labels_ce(ret, gt, ignore=None):
    """GEOT_CHECK_LABELS=1 for the cross-entropy criteria: the synchronous form of the device assert nll_loss fails with
    on a target outside [0, C) (other than the ignore index)."""
    if os.environ.get("GEOT_CHECK_LABELS", "0") == "1" and gt.numel():
        seen = gt if ignore is None else gt[gt != ignore]
        if seen.numel() and (int(seen.min()) < 0 or int(seen.max()) >= ret.shape[1]):
            raise RuntimeError("Target out of bounds: class values must lie in [0, %d)" % ret.shape[1])


class Weight_CELoss(torch.nn.Module):
    """openpoints/loss/build.py:913-925: soft-max cross-entropy with the class weights class_weights.mean(dim=0), averaged
    over ALL B * N points (`.mean()` of a reduction='none' tensor: the weights' sum is not the denominator)."""

    def __init__(self, **kwargs):
        super().__init__()

    def forward(self, ret, gt, class_weights):
        if _wce_fused_ok(ret, gt, class_weights):
            _check_labels_ce(ret, gt)
            return _WeightedCEFn.apply(ret.contiguous(), gt.contiguous(), class_weights.contiguous(), None, 0.0)
        temperature = 1.
        ret = F.log_softmax(ret / temperature, dim=1)
        loss = F.nll_loss(ret, gt.long(), weight=class_weights.mean(dim=0), reduction='none')
        return loss.mean()


class Weight_CELoss_U(torch.nn.Module):
    """openpoints/loss/build.py:928-938: the same on pseudo labels `gt`, with every point whose confidence `logits` is not
    >= thresh (a NaN confidence included) and every point labelled 0 (background) or 255 ignored -- they still count in
    the denominator B * N.  Unlike the reference, which writes the ignore index 255 into the `gt` it is handed
    (train.py:586 passes a clone for that reason), this class does NOT modify the caller's `gt`."""

    def __init__(self, **kwargs):
        super().__init__()

    def forward(self, ret, gt, class_weights, logits, thresh=0.95):
        if _wce_fused_ok(ret, gt, class_weights) and _plain_f32(logits, gt.shape, ret.device):
            if os.environ.get("GEOT_CHECK_LABELS", "0") == "1":
                _check_labels_ce(ret, gt[logits.ge(thresh)], ignore=255)
            return _WeightedCEFn.apply(ret.contiguous(), gt.contiguous(), class_weights.contiguous(), logits.contiguous(),
                                       thresh)
        thresh_mask = logits.ge(torch.tensor(thresh)).bool()
        gt = gt.clone()
        gt[~thresh_mask] = 255
        gt[gt == 0] = 255
        loss = F.cross_entropy(ret, gt.long(), weight=class_weights.mean(dim=0), ignore_index=255, reduction='none')
        return loss.mean()


CRITERIA = {cls.__name__: cls for cls in (Poly1FocalLoss, Poly1FocalLoss_U, Poly1FocalLoss_U_corr, Poly1FocalLoss_U_T,
                                          Weight_CELoss, Weight_CELoss_U)}
SUPERVISED_CRITERIA = ("Poly1FocalLoss", "Weight_CELoss")                       # train.py:449-454, 576-581
UNSUPERVISED_CRITERIA = ("Weight_CELoss_U", "Poly1FocalLoss_U", "Poly1FocalLoss_U_corr", "Poly1FocalLoss_U_T")   # :584-596
# registered by the reference, but train_one_epoch has no branch that calls them with their arguments (`unsup_loss` would be
# unbound at train.py:602, MultiShapeCrossEntropy needs the shape-wise logits the segmentor does not return)
UNBRANCHED = ("MSE_Loss_U", "MultiShapeCrossEntropy", "Poly1FocalLoss_U_Cur", "Poly1FocalLoss_U_top2", "Poly1FocalLoss_U_T_v1")


def criterion_class(name):
    """The class registered under `name`; NotImplementedError (naming it) for a criterion the loop has no branch for."""
    if name in UNBRANCHED:
        raise NotImplementedError("criterion %r: train_one_epoch (examples/segmentation/train.py:449-454, 576-596) has no "
                                  "branch that calls it; it is not mirrored" % (name,))
    if name not in CRITERIA:
        raise KeyError("criterion %r is not one of %s" % (name, sorted(CRITERIA)))
    return CRITERIA[name]


def build_criterion_from_cfg(cfg, **kwargs):
    """openpoints/loss/build.py:956-963: {"NAME": ..., **constructor arguments} -> the criterion."""
    args = dict(cfg)
    name = args.pop("NAME")
    args.update(kwargs)
    return criterion_class(name)(**args)
