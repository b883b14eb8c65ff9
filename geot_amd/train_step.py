"""The training steps the BASELINE configs time, composed from the mirrored modules -- the part of
examples/segmentation/train.py that drives the hot path, and nothing else of the driver (no loaders,
logging, files; the epoch meters only on request, computed on the device; state_dict() / load_state_dict() hand a step's
whole state out and take it back in place, geot_amd/checkpoint.py writes it to a file):

* ``SupervisedStep``  -- configs[2]/[3]: forward of the segmentor on a batch of clouds, Poly1FocalLoss,
  backward, (DDP gradient all-reduce when wrapped,) clip + AdamW step (train.py:436-452, 646-657).
* ``FixMatchNTMStep`` -- configs[4]: one semi-supervised iteration (train.py:455-602, 646-699): frozen
  teacher on the weak view -> pseudo labels (after cfg switch_ep: the student's own weak view, set_epoch());
  student on labelled + strong + weak (WholePartSeg, 6 clouds at B_l = B_u = 2); class-level transition (anchors,
  Gaussian prior, EMA); per-point transition matrices (T_predictor); corrected strong logits; 3-D smoothness loss;
  Poly1Focal losses; backward; both optimisers.  Optionally the epoch meters (train.py:599-644, 672-699) on the
  device: geot_amd/meters.py.

Both are plain callables over device tensors; `ddp()` wraps student and T_predictor the way train.py:159-166
does (SyncBatchNorm + DistributedDataParallel) -- and also wraps T_predictor, which the reference leaves
unsynchronised (last row: an intentional divergence).
"""
import contextlib
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ntm as ntm_mod
from .openpoints.loss.build import SUPERVISED_CRITERIA, UNSUPERVISED_CRITERIA, criterion_class
from .openpoints.models.segmentation import WholePartSeg

NTM_CFG = dict(threshold=0.0, unsupervised_loss_weight=1.0, ema_t_decay=0.999, lambma=0.9, geo_lambma=0.999,
               threed_loss_weight=0.1, threed_k=32, threed_sigma=1.0, filter_outlier=False, lr=1e-3,
               weight_decay=1e-4, grad_norm_clip=None, batch_size_l=2, batch_size_u=2, num_classes=17, switch_ep=50,
               criterion="Poly1FocalLoss", criterion_u="Poly1FocalLoss_U_corr", use_3d_loss=True, use_feat_loss=False,
               feat_loss_weight=10.0, feat_k=16, feat_sigma=1.0, use_identity_loss=False, identity_loss_weight=1.0,
               pseudo_refine=False, pseudo_refine_size=4, pseudo_refine_neighbors=1,
               use_contrastive=False, contrastive_loss_weight=1.0, cur_threshold=0.9, contrast_samples=1024, contrast_seed=0,
               ema_teacher=False, ema_decay=0.99, fused_tail=False, step_per_update=1)
# cfgs/tooth_semi/transformer_finetune_fixmatch_ntm.yaml:45-96 (+ default.yaml); criterion / criterion_u are its
# criterion_args.NAME / criterion_u_args.NAME (a {"NAME": ..., **constructor arguments} dict is taken too).
# pseudo_refine (yaml:75, which the reference never reads): False, True (= "max") or one of utils/pseudo_mask.py's three
# refinements, "max" / "margin" / "margin_v1"; pseudo_refine_size / pseudo_refine_neighbors are their neigborhood_size / n_neigbors
# use_contrastive / contrastive_loss_weight / cur_threshold (yaml:70, 71, 68, which the reference never reads either): the
# teacher-student contrastive loss of utils/cluster_contrastloss.py on the 128-wide head feature, its weight in the total and
# its selection threshold; contrast_samples is the class's sample_nums, contrast_seed the key of its device draws
# ema_teacher / ema_decay (yaml:66 names the decay; the reference freezes its teacher, train.py:218-222, and never applies it):
# after every update the teacher's state_dict() entries follow the student's, t = ema_decay t + (1 - ema_decay) s (integer
# buffers are copied); fused_tail: clip + AdamW (+ that EMA) in one multi-tensor HIP pass (geot_amd/optim_tail.py) instead of
# clip_grad_norm_ + optimizer.step() -- ema_teacher without it runs the same semantics in torch ops
# step_per_update (train.py:435, 440, 463, 657-669): clipping, both optimizers, the EMA and zero_grad run on every
# step_per_update-th call only, with the gradients of the calls in between summed; set_epoch() with another epoch restarts the
# count and keeps the sum, as train.py:435 against :664 does.  With fused_tail the sum is the tail's flat accumulator and the
# count a device int, so a replayed step needs no further graph; without it .grad accumulates in place (eager only)
PSEUDO_REFINE_MODES = ("max", "margin", "margin_v1")
PSEUDO_REFINE_MAX_SIZE = _lib.PSEUDO_REFINE_MAX_N      # include/geot_hip.h GEOT_PSEUDO_REFINE_MAX_N


def _criterion(spec, allowed, what):
    """The criterion a cfg entry names (a NAME or a {"NAME": ..., **kwargs} dict), of the ones train_one_epoch's dispatch
    (train.py:449-454, 576-596) has a branch for in that place.  Raises before anything touches a device."""
    args = dict(spec) if isinstance(spec, dict) else {"NAME": spec}
    name = args.pop("NAME", None)
    cls = criterion_class(name)          # NotImplementedError for a registered criterion the loop has no branch for
    if name not in allowed:
        raise ValueError("%s=%r: train_one_epoch calls one of %s there" % (what, name, ", ".join(allowed)))
    return name, cls(**args)


def check_cfg(cfg):
    """A FixMatch+NTM cfg's switches, checked on the host: -> (criterion name, criterion, criterion_u name, criterion_u)."""
    for key in ("use_3d_loss", "use_feat_loss", "use_identity_loss"):
        if not isinstance(cfg[key], bool):
            raise TypeError("cfg %s must be a bool, got %r" % (key, cfg[key]))
    if cfg["use_feat_loss"] and not (isinstance(cfg["feat_k"], int) and cfg["feat_k"] >= 1 and cfg["feat_sigma"] > 0):
        raise ValueError("cfg use_feat_loss: feat_k must be a positive int and feat_sigma positive, got %r / %r"
                         % (cfg["feat_k"], cfg["feat_sigma"]))
    out = (_criterion(cfg["criterion"], SUPERVISED_CRITERIA, "criterion")
           + _criterion(cfg["criterion_u"], UNSUPERVISED_CRITERIA, "criterion_u"))
    mode = pseudo_refine_mode(cfg)
    size, k = cfg["pseudo_refine_size"], cfg["pseudo_refine_neighbors"]
    for key, v in (("pseudo_refine_size", size), ("pseudo_refine_neighbors", k)):
        if not isinstance(v, int) or isinstance(v, bool):
            raise TypeError("cfg %s must be an int, got %r" % (key, v))
    if not 1 <= k <= size <= PSEUDO_REFINE_MAX_SIZE:
        raise ValueError("cfg pseudo_refine: 1 <= pseudo_refine_neighbors <= pseudo_refine_size <= %d, got %r / %r"
                         % (PSEUDO_REFINE_MAX_SIZE, k, size))
    if mode is not None:
        if out[2] == "Weight_CELoss_U":      # train.py:586-587: its call has no mask
            raise ValueError("cfg pseudo_refine=%r: criterion_u='Weight_CELoss_U' takes no mask (train.py:586-587)"
                             % (cfg["pseudo_refine"],))
        c = cfg["num_classes"]
        if (mode != "max" and c < 2) or (mode == "margin_v1" and c > 17):
            raise ValueError("cfg pseudo_refine=%r: the margin needs 2 classes, margin_v1's E_joint has 17; num_classes is %r"
                             % (mode, c))
    check_contrast_cfg(cfg)
    check_tail_cfg(cfg)
    return out


def check_tail_cfg(cfg):
    """The keys of the moving teacher and the fused tail (a cfg without them is one with the switches off)."""
    for key in ("ema_teacher", "fused_tail"):
        if key in cfg and not isinstance(cfg[key], bool):
            raise TypeError("cfg %s must be a bool, got %r" % (key, cfg[key]))
    if "step_per_update" in cfg:
        check_step_per_update(cfg["step_per_update"], "cfg step_per_update")
    if "ema_decay" in cfg:
        d = cfg["ema_decay"]
        if isinstance(d, bool) or not isinstance(d, (int, float)):
            raise TypeError("cfg ema_decay must be a number, got %r" % (d,))
        if not 0.0 <= float(d) < 1.0:
            raise ValueError("cfg ema_decay must be in [0, 1), got %r" % (d,))


def check_step_per_update(k, what="step_per_update"):
    """An int >= 1 (a bool is none), checked on the host."""
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError("%s must be an int, got %r" % (what, k))
    if k < 1:
        raise ValueError("%s must be at least 1, got %r" % (what, k))
    return k


def check_contrast_cfg(cfg):
    """The contrastive loss's keys (a cfg without them is one with the switch off)."""
    if "use_contrastive" not in cfg:
        return
    if not isinstance(cfg["use_contrastive"], bool):
        raise TypeError("cfg use_contrastive must be a bool, got %r" % (cfg["use_contrastive"],))
    full = dict(NTM_CFG, **cfg)
    for key in ("contrast_samples", "contrast_seed"):
        if not isinstance(full[key], int) or isinstance(full[key], bool):
            raise TypeError("cfg %s must be an int, got %r" % (key, full[key]))
    for key in ("contrastive_loss_weight", "cur_threshold"):
        if isinstance(full[key], bool) or not isinstance(full[key], (int, float)):
            raise TypeError("cfg %s must be a number, got %r" % (key, full[key]))
    w, th, s = float(full["contrastive_loss_weight"]), float(full["cur_threshold"]), full["contrast_samples"]
    if not (0.0 < w < float("inf")):
        raise ValueError("cfg contrastive_loss_weight must be positive and finite, got %r" % (full["contrastive_loss_weight"],))
    if not 0.0 < th <= 1.0:
        raise ValueError("cfg cur_threshold must be in (0, 1], got %r" % (full["cur_threshold"],))
    if not 1 <= s <= _lib.CONTRAST_MAX_S:
        raise ValueError("cfg contrast_samples must be in 1..%d, got %r" % (_lib.CONTRAST_MAX_S, s))


def pseudo_refine_mode(cfg):
    """cfg pseudo_refine -> None (off) or "max" / "margin" / "margin_v1" (True = "max")."""
    v = cfg["pseudo_refine"]
    if v is False:
        return None
    if v is True:
        return "max"
    if not isinstance(v, str):
        raise TypeError("cfg pseudo_refine must be False, True or one of %s, got %r" % (", ".join(PSEUDO_REFINE_MODES), v))
    if v not in PSEUDO_REFINE_MODES:
        raise ValueError("cfg pseudo_refine must be False, True or one of %s, got %r" % (", ".join(PSEUDO_REFINE_MODES), v))
    return v


def unused_parameters(cfg=None):
    """Names (suffixes, as ddp(unused=...) takes them) of the student's and T_predictor's parameters that receive no
    gradient under `cfg` (NTM_CFG's keys; missing ones at their defaults).  T_revision / T_linear never do (see
    UNUSED_SUPERVISED); `sigma` reaches the loss only through the class-transition prior inside the corrected logits, which
    Poly1FocalLoss_U and Weight_CELoss_U do not read; T_predictor ("fc.": every layer of Ins_T_mean / sig_t_mean) reaches it
    through the corrected logits and the 3-D, feature and identity losses."""
    cfg = dict(NTM_CFG, **(cfg or {}))
    name_u = cfg["criterion_u"]["NAME"] if isinstance(cfg["criterion_u"], dict) else cfg["criterion_u"]
    unused = ["T_revision.weight", "T_linear.weight"]
    if name_u in _IGNORES_CORRECTION:
        unused.append("sigma")
        if not (cfg["use_3d_loss"] or cfg["use_feat_loss"] or cfg["use_identity_loss"]):
            unused.append("T_predictor.*")
    return tuple(unused)


_IGNORES_CORRECTION = ("Poly1FocalLoss_U", "Weight_CELoss_U")      # train.py:584-590: they get the uncorrected strong logits


# parameters the configured step never differentiates: T_revision is not used by forward() at all and the
# `correction` output of T_linear is dropped by the caller (train.py:490 `pred_all, delta_T, sigma = ...`, delta_T
# unused); `sigma` only receives a gradient through the class-transition prior of the FixMatch step.  DDP's reducer
# must be told, or it waits for their gradients (the reference never ran its DDP path: train.py:7 pins one GPU).
UNUSED_SUPERVISED = ("T_revision.weight", "T_linear.weight", "sigma")
UNUSED_FIXMATCH = ("T_revision.weight", "T_linear.weight")       # = unused_parameters() of the default cfg


def ddp(module, device, sync_bn=True, unused=(), min_world=2, **kw):
    """train.py:159-166: SyncBatchNorm conversion + DistributedDataParallel when a process group of at least `min_world`
    ranks is up (min_world=1: wrap even a single rank -- the one way to put DDP's reducer and RCCL under a step on a
    one-GPU box, tests/test_dist_gpu.py)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() >= min_world):
        return module
    if sync_bn:
        module = nn.SyncBatchNorm.convert_sync_batchnorm(module)
    skip = [n for n, _ in module.named_parameters() if any(n.endswith(u) for u in unused)]
    skip += ["." + n for n in skip if "." not in n]     # DDP spells a root-level parameter "<module_name>.<param>" = ".sigma"
    if skip:
        nn.parallel.DistributedDataParallel._set_params_and_buffers_to_ignore_for_model(module, skip)
    ids = [device.index] if device.type == "cuda" else None
    kw.setdefault("gradient_as_bucket_view", True)      # gradients live in the all-reduce buckets: no 108 MB copy per step
    return nn.parallel.DistributedDataParallel(module, device_ids=ids, **kw)


def sync_only(module, sync_bn=True, min_world=2):
    """The data-parallel form of a module for a step that is REPLAYED FROM hipGraphs (geot_amd/graph_step.py): SyncBatchNorm
    conversion as train.py:159-166 does it, but NO DistributedDataParallel wrapper -- the step exchanges its gradients itself
    (GradSync).  Why not wrap and bypass: DDP's reducer keeps every parameter's AccumulateGrad node alive from its
    construction on, on the stream that was current then; a backward captured on the capture stream hops to that stream and
    back for each of them -- forks inside a capture, which this runtime answers with a crash in hipStreamEndCapture
    (profiles/r04_graph_capture_notes.txt; reproduced with DDP in round 5)."""
    import torch.distributed as dist
    if sync_bn and dist.is_available() and dist.is_initialized() and dist.get_world_size() >= min_world:
        module = nn.SyncBatchNorm.convert_sync_batchnorm(module)
    return module


class GradSync:
    """The data-parallel gradient exchange as ONE flat all-reduce, for a step that is replayed from a hipGraph
    (geot_amd/graph_step.py): DistributedDataParallel's reducer is host logic (bucket hooks fired from the autograd engine)
    and cannot be captured, an RCCL collective on the current stream can -- it is a kernel node.  The step holds the bare
    (SyncBatchNorm-converted: sync_only) modules and calls this between the backward and the optimizer: every gradient that
    exists is packed into one static fp32 buffer, divided by the world size (before the sum, as the reducer does), summed
    over the ranks, and copied back.  108 MB at the segmentor's size: one collective instead of five 25-MB buckets; nothing
    overlaps the backward -- the price of a host-free step (train.py:159-166 wraps the model; :646-669 is the loop this
    replaces).  Construction broadcasts rank 0's parameters and buffers, as DDP's does."""

    def __init__(self, modules, group=None, broadcast=True):
        import torch.distributed as dist
        modules = [_unwrapped(m) for m in modules]
        self.params = [p for m in modules for p in m.parameters() if p.requires_grad]
        self.group = group
        self.world = dist.get_world_size(group)
        self.flat = None
        self.views = None
        self.collectives = 0
        if broadcast and self.world > 1:
            with torch.no_grad():
                for m in modules:
                    for t in list(m.parameters()) + list(m.buffers()):
                        dist.broadcast(t, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)

    def __call__(self):
        import torch.distributed as dist
        grads = [p.grad for p in self.params if p.grad is not None]
        if not grads:
            return
        sizes = [g.numel() for g in grads]
        if self.flat is None or self.flat.numel() != sum(sizes):
            self.flat = torch.empty(sum(sizes), dtype=grads[0].dtype, device=grads[0].device)
            self.views = list(torch.split(self.flat, sizes))
        flat_grads = [g.reshape(-1) for g in grads]          # (gradients are contiguous: views, not copies)
        torch._foreach_copy_(self.views, flat_grads)
        if self.world > 1:
            self.flat.mul_(1.0 / self.world)
        dist.all_reduce(self.flat, group=self.group)
        self.collectives += 1
        torch._foreach_copy_(flat_grads, self.views)

    def exchange(self, flat):
        """The same exchange for gradients that already lie in one flat buffer (OptimTail's accumulator under
        step_per_update): divided by the world size, summed over the ranks, in place -- one collective."""
        import torch.distributed as dist
        if self.world > 1:
            flat.mul_(1.0 / self.world)
        dist.all_reduce(flat, group=self.group)
        self.collectives += 1


def _unwrapped(module):
    """The module inside a DistributedDataParallel wrapper (the module itself when it is not wrapped)."""
    return module.module if hasattr(module, "module") else module


def _inner(module, bypass):
    """The module a step calls: DDP's wrapped module when the step exchanges its gradients itself (GradSync)."""
    return _unwrapped(module) if bypass else module


def _update(grad_sync, clip, model, optimizers, tail=None, fused=False):
    """The tail of an iteration behind its backward: the step's own gradient exchange (GradSync, if any), clipping of
    `model`'s gradients, then every optimizer in order (train.py:656-660).  tail: the step's OptimTail (geot_amd/optim_tail.py),
    which holds the same clip and optimizers (and the teacher's EMA, if any): its fused pass when `fused`, else the same
    semantics in torch ops."""
    if grad_sync is not None:
        grad_sync()
    if tail is not None:
        if fused:
            tail.step()
        else:
            tail.composite()
        for optimizer in optimizers:
            optimizer.zero_grad(set_to_none=True)
        return
    if clip is not None:
        torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
    for optimizer in optimizers:
        optimizer.step()
        optimizer.zero_grad(set_to_none=True)


def _window_update(step, clip, model, fused):
    """_update under the step's step_per_update = k.  1: _update, call for call.  With the fused tail every call runs it: the
    tail sums the gradients, gates the update on its device counter and exchanges its accumulator on update calls; the
    gradients are dropped every time.  Otherwise the reference's form: nothing runs before call k of a window, and .grad
    accumulates in place (host logic: eager only)."""
    k = step.step_per_update
    if k == 1:
        return _update(step.grad_sync, clip, model, step.optimizers(), step.tail, fused)
    if fused:
        step.tail.step(sync=step.grad_sync)
        for optimizer in step.optimizers():
            optimizer.zero_grad(set_to_none=True)
        return
    step._window_calls += 1
    if step._window_calls < k:
        return
    step._window_calls = 0
    _update(step.grad_sync, clip, model, step.optimizers(), step.tail, False)


def _accumulating(step, fused):
    """The context of a call's forward and backward: with step_per_update > 1 in the torch form, a DistributedDataParallel
    module runs the calls that do not update under its no_sync() -- its reducer exchanges the accumulated .grad on the update
    call alone.  (With the fused tail the gradients are dropped after every call, so each call's exchange is needed.)"""
    stack = contextlib.ExitStack()
    if step.step_per_update > 1 and not fused and step._window_calls + 1 < step.step_per_update:
        for m in step.sync_modules():
            if isinstance(m, nn.parallel.DistributedDataParallel):
                stack.enter_context(m.no_sync())
    return stack


class _UpdateWindow:
    """What both steps keep of the open update window (cfg step_per_update): the calls counted so far in the torch form, the
    clip value and whether the tail is its fused pass -- the arguments of _window_update / _accumulating, held once."""

    def open_window(self, step_per_update, clip, fused):
        self.step_per_update, self.clip, self.fused = step_per_update, clip, fused
        self._window_calls = 0         # calls of the open window (the torch form's count; the fused tail keeps its own)

    def restart_window(self):
        """step_per_update > 1: the count of the open window returns to 0 and the gradients summed so far stay, joining the
        next window's first update (train.py:435 against :664).  With step_per_update = 1 nothing is issued."""
        if self.step_per_update > 1:
            self._window_calls = 0
            if self.tail is not None:
                self.tail.restart()

    # ---- what a checkpoint keeps of the window (geot_amd/checkpoint.py) ----
    def window_state(self, modules):
        """-> {"window_calls", "tail", "grads"}: the torch form's count, the tail's state_dict() (None without a tail) and --
        in the torch form inside an open window only -- the .grad of `modules`' parameters ({name: module}), which hold the
        window's partial sum.  (The fused tail sums in its accumulator and the gradients are dropped after every call.)"""
        from . import checkpoint as ck
        grads = None
        if not self.fused and self._window_calls > 0:
            grads = {name: {n: ck.copied(p.grad) for n, p in _unwrapped(m).named_parameters() if p.grad is not None}
                     for name, m in modules.items()}
        return {"window_calls": self._window_calls, "tail": self.tail.state_dict() if self.tail is not None else None,
                "grads": grads}

    def restore_window(self, r, state, modules):
        """window_state()'s counterpart, first half: checks, and hands the writes to r (a checkpoint.Restore)."""
        calls = r.number("window_calls", state["window_calls"], int)
        if not 0 <= calls < self.step_per_update or (self.fused and calls):
            raise ValueError("window_calls: %r is no call of this step's window (step_per_update %d, %s form)"
                             % (calls, self.step_per_update, "fused" if self.fused else "torch"))
        if (state["tail"] is None) != (self.tail is None):
            raise ValueError("tail: %s key 'tail' (the step is built %s a tail)"
                             % (("missing", "with") if self.tail is not None else ("unexpected", "without")))
        if self.tail is not None:
            self.tail.restore(r, state["tail"])
        grads = state["grads"]
        if (grads is not None) != (not self.fused and calls > 0):
            raise ValueError("grads: %s key 'grads' (the torch form carries its open window in .grad, and only there)"
                             % ("unexpected" if grads is not None else "missing"))
        writes = []
        if grads is not None:
            r.keys(grads, list(modules), "grads")
        for name, m in modules.items():
            own = dict(_unwrapped(m).named_parameters())
            saved = grads[name] if grads is not None else {}
            r.keys(saved, (), "grads.%s" % name, optional=list(own))
            for n, p in own.items():
                if n in saved:
                    r.check("grads.%s.%s" % (name, n), p, saved[n])
                writes.append((p, saved.get(n)))

        def host():
            self._window_calls = calls
            if self.fused:
                return
            for p, g in writes:        # (outside a window the torch form holds no gradient: zero_grad(set_to_none=True))
                if g is None:
                    p.grad = None
                elif p.grad is None:
                    p.grad = g.detach().to(p.device, copy=True)
                else:
                    p.grad.copy_(g)
        r.then(host)


def _check_head(r, state, keys, kind, layout):
    """The head of a step's state: its keys, the format version, the kind of step and the layout cfg keys."""
    from . import checkpoint as ck
    r.keys(state, keys, "")
    if state["format"] != ck.FORMAT:
        raise ValueError("format: the state has format %r, this package reads %r" % (state["format"], ck.FORMAT))
    if state["kind"] != kind:
        raise ValueError("kind: the state is a %s's, the step is a %s" % (state["kind"], kind))
    ck.same_layout(state["layout"], layout)


class _Cut:
    """A forward with the segmentor cutting its autograd graph at the transformer blocks (cut_at_blocks / take_cut), for a
    two-phase backward:  with _Cut(seg) as cut: <forward>;  loss.backward() then stops at the blocks and cut.rest() hands
    back the second phase as data -- (the blocks' outputs, their gradients), what backward_rest() takes; None for a model
    that cannot cut (or on=False): loss.backward() was the whole backward."""

    def __init__(self, seg, on=True):
        self.seg, self.cut = seg if on and hasattr(seg, "take_cut") else None, None

    def __enter__(self):
        if self.seg is not None:
            self.seg.cut_at_blocks = True
        return self

    def __exit__(self, kind, *_):
        if self.seg is not None:
            self.seg.cut_at_blocks = False
            self.cut = self.seg.take_cut() if kind is None else None

    def rest(self):
        return None if self.cut is None else (self.cut[0], [d.grad for d in self.cut[1]])


def backward_rest(rest):
    """The rest of a backward that _Cut stopped at the blocks (the blocks, the patch encoder); None: nothing is left."""
    if rest is not None:
        torch.autograd.backward(rest[0], rest[1])


def parameter_groups(model, weight_decay=1e-4, skip_list=()):
    """The two AdamW parameter groups of the reference's optimizer factory (openpoints/optim/optim_factory.py:66-119
    get_parameter_groups, reached through build_optimizer_from_cfg :190-198 with its default filter_bias_and_bn=True,
    train.py:169 / :225): every 1-D parameter (BatchNorm / LayerNorm / GroupNorm weights, `sigma`, ...), every
    `*.bias` and everything named in the model's no_weight_decay() goes WITHOUT weight decay, the rest with it.
    Group order and the `lr_scale` key are the factory's (first appearance; 1.0 without layer decay)."""
    module = _unwrapped(model)                                            # DDP wrapper: the factory looks inside (:190-193)
    if not skip_list and hasattr(module, "no_weight_decay"):
        skip_list = module.no_weight_decay()
    groups = {}
    for name, param in model.named_parameters():
        if not param.requires_grad:
            continue
        no_decay = param.ndim == 1 or name.endswith(".bias") or any(key in name for key in skip_list)
        key = "no_decay" if no_decay else "decay"
        if key not in groups:
            groups[key] = {"weight_decay": 0.0 if no_decay else weight_decay, "params": [], "lr_scale": 1.0}
        groups[key]["params"].append(param)
    return list(groups.values())


def _join(dev, side, *tensors):
    """The one place a side stream's results are handed to the current stream: the current stream waits for `side`,
    and -- outside graph capture, where record_stream is not allowed and the capture's own dependency edges keep the
    memory alive -- every tensor allocated on `side` is recorded as used by the current stream, so the caching allocator
    cannot hand its block to a later allocation on `side` while a reader queued here is still pending (whatever the
    order of frees / allocations a future change introduces)."""
    cur = torch.cuda.current_stream(dev)
    cur.wait_stream(side)
    if not torch.cuda.is_current_stream_capturing():
        for t in tensors:
            if t is not None and t.is_cuda:
                t.record_stream(cur)


class BatchWork:
    """Everything of a FixMatch iteration that depends on its batches (and on frozen state) alone -- what
    FixMatchNTMStep.lookahead_work() returns and student_iteration() consumes.  None: not part of this phase / switch off.
    geom_s / geom_t: the student's / the teacher's Geometry (geom_t only while a MOVING teacher's forward is still to run:
    a frozen teacher's forward has consumed it); pseudo: (pred_u, logits_u_aug, label_u_aug) of the teacher, feat_t: its
    head feature (cfg use_contrastive); knn: (nbr, order), the 3-D loss's kNN graph and Morton order of raw_pos (cfg
    use_3d_loss); refine_nbr: the weak view's neighbour table (cfg pseudo_refine, utils/pseudo_mask.py neighbours).
    The object alone knows which fields were made on a side stream (made_on) and still need joining: the first read of
    such a field hands it -- and the fields made with it -- to the current stream (_join); a product made in line has
    nothing to join.  made() asks whether a field is there without joining it."""
    FIELDS = ("geom_s", "geom_t", "pseudo", "feat_t", "knn", "refine_nbr")

    def __init__(self, geom_s=None, geom_t=None, pseudo=None, feat_t=None, knn=None, refine_nbr=None):
        self.__dict__.update(geom_s=geom_s, geom_t=geom_t, pseudo=pseudo, feat_t=feat_t, knn=knn, refine_nbr=refine_nbr)
        self._sides = {}               # field -> (side stream, the fields made there together), until joined

    def tree_fields(self):
        """(buffers, identities) for graph_step.py, as Geometry.tree_fields: a clone has nothing left to join."""
        return self.FIELDS, ("_sides",)

    def made_on(self, side, *names):
        """These fields were queued on `side` together (None: in line, nothing to join)."""
        for n in names if side is not None else ():
            self._sides[n] = (side, names)

    def made(self, name):
        return self.__dict__[name] is not None

    def _read(self, name):
        pending = self._sides.pop(name, None) if self._sides else None
        if pending is not None:
            side, names = pending
            for n in names:
                self._sides.pop(n, None)
            values = [self.__dict__[n] for n in names]
            _join(side.device, side, *(t for v in values for t in (v if isinstance(v, tuple) else (v,))))
        return self.__dict__[name]


for _name in BatchWork.FIELDS:      # plain attributes to write; reading one joins it first
    setattr(BatchWork, _name, property(lambda self, n=_name: self._read(n), lambda self, v, n=_name: self.__dict__.__setitem__(n, v)))


def make_optimizer(model, lr=1e-3, weight_decay=1e-4):
    """AdamW as train.py:169 / :225 build it (cfgs/tooth_semi/default.yaml:66-68: adamw, weight_decay 1e-4)."""
    groups = parameter_groups(model, weight_decay) if weight_decay else \
        [{"params": [p for p in model.parameters() if p.requires_grad]}]
    params = [p for g in groups for p in g["params"]]
    fused = bool(params) and all(p.is_cuda for p in params)
    return torch.optim.AdamW(groups, lr=lr, weight_decay=0.0 if weight_decay else weight_decay, fused=fused)


_MODE_SENSITIVE = (nn.modules.batchnorm._BatchNorm, nn.modules.dropout._DropoutNd, nn.GroupNorm, nn.LayerNorm)


def _mode(module, training):
    """module.train(training) unless the tree is in that mode already: train.py sets the modes once per epoch
    (train_one_epoch: model.train(), model_t.eval()); walking ~180 modules three times per iteration cost 2 ms of host time.
    "Already" = the root's flag AND the flag of every submodule whose behaviour depends on it (BatchNorm, Dropout, DropPath --
    a short list cached on the module): a child toggled on its own (a BatchNorm put in eval() for a partial validation, a
    helper that flips the teacher's children) is put back instead of silently running in the wrong mode."""
    watch = module.__dict__.get("_geot_mode_watch")
    if watch is None:
        watch = [m for m in module.modules()
                 if isinstance(m, _MODE_SENSITIVE) or type(m).__name__ == "DropPath"]
        module.__dict__["_geot_mode_watch"] = watch
    if module.training != training or any(m.training != training for m in watch):
        module.train(training)


class _LookAhead:
    """Where an iteration queues the next batch's geometry -- make() -> the geometry, or None: nothing to queue -- inside the
    backward, when it reaches the transformer blocks ("blocks"; the segmentor must offer the hook), or right behind the
    forward ("forward").  GEOT_LOOKAHEAD_AT overrides the step's default -- measured (profiles/r03_ab_lookahead_at*.txt): the
    supervised step 33.27 ms at "blocks" against 33.61 at "forward" (behind the forward the 8192-sample FPS shares the chip
    with the decoder's widest GEMMs and takes 5.5 instead of 4.8 ms); the FixMatch iteration 32.1 ms at "forward" against
    32.7 at "blocks" (behind its student forward come the NTM block and the losses: a stretch of small kernels that leaves
    the FPS launches room)."""

    def __init__(self, segmentor, default, make):
        self.segmentor, self.make, self.queued = segmentor, make, None
        self.at_blocks = os.environ.get("GEOT_LOOKAHEAD_AT", default) == "blocks" and hasattr(segmentor, "at_blocks_backward")
        if make is not None and self.at_blocks:
            segmentor.at_blocks_backward = self._queue     # runs inside the backward, when it reaches the transformer blocks

    def _queue(self):
        self.queued = self.make()

    def behind_forward(self):
        if self.make is not None and not self.at_blocks:
            self._queue()

    def done(self):
        """Behind the backward: clear the hook -> what was queued (None: nothing)."""
        if self.at_blocks:
            self.segmentor.at_blocks_backward = None
        return self.queued


class SupervisedStep(_UpdateWindow):
    def __init__(self, model, lr=1e-3, weight_decay=1e-4, grad_norm_clip=None, grad_sync=None, criterion="Poly1FocalLoss",
                 fused_tail=False, step_per_update=1):
        """criterion: cfg criterion_args -- "Poly1FocalLoss" or "Weight_CELoss" (or {"NAME": ..., **kwargs}); the latter takes
        the batch's class_weights (train.py:449-450).  fused_tail: clip + AdamW as one multi-tensor HIP pass
        (geot_amd/optim_tail.py; with a clip, self.tail.total_norm is the gradient norm on the device).  step_per_update = k:
        clipping, the optimizer and zero_grad run on every k-th call with the gradients summed since (cfg step_per_update,
        train.py:657-669) -- in the fused tail's accumulator, or without it in .grad (eager only); new_epoch() restarts the count."""
        if not isinstance(fused_tail, bool):
            raise TypeError("SupervisedStep: fused_tail must be a bool, got %r" % (fused_tail,))
        self.open_window(check_step_per_update(step_per_update, "SupervisedStep: step_per_update"), grad_norm_clip, fused_tail)
        self.criterion_name, self.criterion = _criterion(criterion, SUPERVISED_CRITERIA, "criterion")
        self.model = model
        self.optimizer = make_optimizer(model, lr, weight_decay)
        self._geometry = None          # coordinate-only work of the next batch, queued by the previous call
        self.grad_sync = grad_sync     # a GradSync: the step exchanges its gradients itself (bare modules: sync_only)
        self.tail = None
        if fused_tail:
            from .optim_tail import OptimTail
            self.tail = OptimTail([self.optimizer], max_norm=grad_norm_clip,
                                  clip_params=list(model.parameters()) if grad_norm_clip is not None else None,
                                  accumulate=self.step_per_update)

    def optimizers(self):
        return [self.optimizer]

    new_epoch = _UpdateWindow.restart_window       # (the next call opens an epoch)

    def sync_modules(self):
        return [self.model]

    _STATE_KEYS = ("format", "kind", "layout", "model", "optimizer", "window_calls", "tail", "grads")

    def layout(self):
        """The constructor arguments that fix the layout of state_dict()."""
        return {"step_per_update": self.step_per_update, "fused_tail": self.fused}

    def state_dict(self):
        """Everything a resumed run needs of this step ("Checkpoints"): the model (unwrapped), the
        optimizer in torch's own layout, the open step_per_update window.  Copies made on the current stream, no
        synchronisation; between any two calls, not under stream capture."""
        from . import checkpoint as ck
        ck.refuse_capture("SupervisedStep")
        out = {"format": ck.FORMAT, "kind": "SupervisedStep", "layout": self.layout(), "model": ck.module_state(self.model),
               "optimizer": ck.optimizer_state(self.optimizer)}
        out.update(self.window_state({"model": self.model}))
        return out

    def load_state_dict(self, state):
        """state_dict()'s counterpart: everything is checked first (ValueError naming the key; the step is left as it was),
        then every tensor that exists is written in place -- a captured graph holds them -- and optimizer state that does not
        exist yet is created as the first eager call would.  A queued look-ahead is dropped."""
        from . import checkpoint as ck
        r = ck.Restore()
        _check_head(r, state, self._STATE_KEYS, "SupervisedStep", self.layout())
        r.module("model", self.model, state["model"])
        r.optimizer("optimizer", self.optimizer, state["optimizer"], self.tail if self.fused else None)
        self.restore_window(r, state, {"model": self.model})
        r.then(lambda: setattr(self, "_geometry", None))
        r.commit()

    def __call__(self, pos, cls, target, next_pos=None, class_weights=None):
        """pos (B,N,3) f32, cls (B,1) int64 jaw id, target (B,N) int64 -> detached loss.
        class_weights (B, C) f32: data['class_weights'], required by (and only read under) criterion="Weight_CELoss".
        next_pos: the coordinates of the NEXT batch, when the loop already holds them (a data loader with one batch of
        look-ahead): their sampling / grouping / index work is queued between this batch's forward and backward
        (PointTransformer_seg_T.prefetch_geometry) and picked up by the next call -- same results, 0.6 ms less per step.
        The queued work is used only if the next call passes that very tensor, unedited (the model checks the tensor, its
        version counter and, for WholePartSeg, the tensors it was assembled from); anything else is computed in line."""
        geometry, self._geometry = self._geometry, None
        with _accumulating(self, self.fused):
            loss, self._geometry = self.iteration(pos, cls, target, geometry, next_pos, class_weights)
        return loss

    def lookahead_work(self, pos):
        """Everything of an iteration that depends on its batch alone (the geometry: Group, the 8192-sample FPS, the index
        plan), on the CURRENT stream -> what iteration(geometry=...) takes.  graph_step.py replays this as a graph of its
        own beside the previous iteration's training graph."""
        _mode(self.model, True)
        inner = _unwrapped(self.model)
        return inner.prefetch_geometry(pos, inline=True) if hasattr(inner, "prefetch_geometry") else None

    def forward_loss(self, pos, cls, target, geometry=None, class_weights=None):
        """The first half of an iteration: the forward and the loss (with its autograd graph)."""
        weighted = self.criterion_name == "Weight_CELoss"
        if weighted and class_weights is None:
            raise RuntimeError("SupervisedStep(criterion='Weight_CELoss'): the batch's class_weights are required")
        _mode(self.model, True)
        logits = _inner(self.model, self.grad_sync is not None)(pos, pos.transpose(1, 2).contiguous(), cls, geometry=geometry)[0]
        return self.criterion(logits, target, class_weights) if weighted else self.criterion(logits, target)

    def backward_update(self, loss):
        """The second half: backward, clipping, the optimizer -> the detached loss."""
        loss.backward()
        _window_update(self, self.clip, self.model, self.fused)
        return loss.detach()

    def forward_backward_head(self, pos, cls, target, geometry=None, class_weights=None):
        """The iteration up to the point where the backward reaches the transformer blocks -- forward, loss, the backward of
        the head and the decoder -- for a model that can cut its autograd graph there (cut_at_blocks / take_cut: the
        segmentor); otherwise the whole backward.  -> (detached loss, what backward_rest_update needs)."""
        with _Cut(_unwrapped(self.model)) as cut:
            loss = self.forward_loss(pos, cls, target, geometry, class_weights)
        loss.backward()
        return loss.detach(), cut.rest()

    def backward_rest_update(self, rest):
        """The rest of the backward (the blocks, the patch encoder), clipping, the optimizer."""
        backward_rest(rest)
        _window_update(self, self.clip, self.model, self.fused)

    def iteration(self, pos, cls, target, geometry=None, next_pos=None, class_weights=None):
        """One iteration -> (detached loss, the geometry queued for next_pos or None)."""
        inner = _unwrapped(self.model)
        make = None
        if next_pos is not None and hasattr(inner, "prefetch_geometry"):
            def make():
                return inner.prefetch_geometry(next_pos)
        look = _LookAhead(inner, "blocks", make)
        loss = self.forward_loss(pos, cls, target, geometry, class_weights)
        look.behind_forward()
        loss = self.backward_update(loss)
        return loss, look.done()


PHASES = ("", "@e", "@2")      # frozen teacher; moving teacher (cfg ema_teacher), up to switch_ep; self-labelling, after it


def lookahead_keys(phase, cfg):
    """The keys of (data, data_u) FixMatchNTMStep.lookahead_work reads in `phase`: after switch_ep no teacher forward, and
    without cfg use_3d_loss no raw_pos -- the look-ahead then builds no kNN graph and no Morton order."""
    keys_u = ("pos_s", "pos_w", "raw_pos") if phase == "@2" else ("pos_s", "pos_w", "x_w", "cls_w", "raw_pos")
    return ("pos",), keys_u if cfg.get("use_3d_loss", True) else tuple(k for k in keys_u if k != "raw_pos")


class FixMatchNTMStep(_UpdateWindow):
    """State of train_one_epoch that survives an iteration: ema_t (C,C), cm (C,C), both optimisers (and the epoch meters,
    when asked for).  The epoch set by set_epoch() picks the pseudo labels' source, as train.py:469-498 does: the frozen
    teacher up to cfg switch_ep (and when no epoch was ever set), the student's own weak view after it."""

    def __init__(self, student, teacher, t_predictor, cm=None, cfg=None, group=None, meters=None):
        """meters: None / False (off: nothing runs), True (a geot_amd.meters.FixMatchMeters from cfg) or such an object --
        updated by every iteration on the device, read with its read(), emptied with its reset().  The unlabelled batch
        must then carry the ground truth data_u["y"] (B_u, N) or (B_u, N, 1)."""
        self.cfg = dict(NTM_CFG, **(cfg or {}))
        c = self.cfg["num_classes"]
        # the cfg's switches first: a criterion the loop has no branch for is refused before anything touches a device
        self.criterion_name, self.criterion, self.criterion_u_name, self.criterion_u = check_cfg(self.cfg)
        self.model, self.model_t, self.T_predictor = student, teacher, t_predictor
        for p in self.model_t.parameters():
            p.requires_grad = False                                                    # train.py:221-222
        dev = next(student.parameters()).device
        self.threed_loss = ntm_mod.threeD_space_loss(self.cfg["threed_k"], self.cfg["threed_sigma"], c)
        self.feat_S_loss = ntm_mod.feature_space_loss(self.cfg["feat_k"], self.cfg["feat_sigma"], c)      # train.py:268-269
        self.identity_loss = ntm_mod.Idenyity_loss()
        self.Identity_t = torch.eye(c, device=dev) if self.cfg["use_identity_loss"] else None              # train.py:430
        # the corrected strong logits have a reader only under these two (train.py:591-596)
        self.needs_correction = self.criterion_u_name not in _IGNORES_CORRECTION
        self.refine_mode = pseudo_refine_mode(self.cfg)      # None: off -- nothing below runs
        # cfg use_contrastive: the teacher-student contrastive loss on the 128-wide head feature (the output of seg_head[1]);
        # off (the default): nothing is allocated and no launch is added.  Bank, pointer and draw counter are allocated
        # here, per rank like every other buffer of the step: a first use under graph capture would be a memcpy node
        self.contrast = None
        if self.cfg["use_contrastive"]:
            from .utils.cluster_contrastloss import nativeContrastLoss_t
            from .openpoints.dataset.sample_draw import DeviceDraws
            segs = [getattr(_unwrapped(m), "segmentor", None) for m in (student, teacher)]
            if not all(hasattr(sg, "keep_head_feature") for sg in segs):
                raise RuntimeError("cfg use_contrastive: the segmentor has no head feature to tap (PointTransformer_seg_T has)")
            self.contrast = nativeContrastLoss_t(self.cfg["contrast_samples"], segs[0].seg_head[1].num_features,
                                                 self.cfg["cur_threshold"], dev, DeviceDraws(self.cfg["contrast_seed"]))
            for sg in segs:
                sg.keep_head_feature = True
        if self.refine_mode == "margin_v1" and dev.type == "cuda":
            from .utils.pseudo_mask import _e_joint
            _e_joint(dev, c)          # uploaded here: a first use under graph capture would be a memcpy node
        self.optimizer = make_optimizer(student, self.cfg["lr"], self.cfg["weight_decay"])
        self.T_optimizer = make_optimizer(t_predictor, self.cfg["lr"], self.cfg["weight_decay"])
        # cfg ema_teacher / fused_tail (both off: no tail object, _update is the torch code it always was).  The teacher's
        # parameters keep requires_grad=False: the EMA writes their memory, autograd never sees them
        self.tail = None
        self.open_window(self.cfg["step_per_update"], self.cfg["grad_norm_clip"], self.cfg["fused_tail"])
        if self.cfg["ema_teacher"] or self.cfg["fused_tail"]:
            from .optim_tail import OptimTail
            clip, ema = self.cfg["grad_norm_clip"], self.cfg["ema_teacher"]
            self.tail = OptimTail(self.optimizers(), clip_params=list(student.parameters()) if clip is not None else None,
                                  max_norm=clip, teacher=teacher if ema else None, student=student if ema else None,
                                  ema_decay=self.cfg["ema_decay"] if ema else None,
                                  accumulate=self.step_per_update if self.cfg["fused_tail"] else 1)
        self.ema_t = torch.eye(c, device=dev)                                          # train.py:274
        self.cm = cm if cm is not None else torch.full((c, c), 1.0 / c, device=dev)    # cal_mean_feature's output
        self.group = group
        self._side = None
        self._geometry = (None, None)      # coordinate-only work of the next student / teacher batch (look-ahead)
        self._teacher_stream = None
        # the frozen teacher's forward on its own stream beside the student's (same results; GEOT_TEACHER_STREAM=0: in line)
        self.overlap_teacher = os.environ.get("GEOT_TEACHER_STREAM", "1") != "0"
        self.share_weak_geometry = os.environ.get("GEOT_SHARE_WEAK_GEOMETRY", "1") != "0"
        self.grad_sync = None          # a GradSync: see SupervisedStep
        self.epoch = None              # set_epoch(); None: never set (the teacher's phase)
        if meters is True:
            from .meters import FixMatchMeters
            meters = FixMatchMeters(c, dev, self.cfg["batch_size_l"], self.cfg["batch_size_u"], self.cfg["threshold"], self.ema_t)
        self.meters = meters or None
        if self.meters is not None and self.meters.ema_t is None:
            self.meters.ema_t = self.ema_t           # read() reports the step's transition buffer

    def optimizers(self):
        return [self.optimizer, self.T_optimizer]

    def sync_modules(self):
        return [self.model, self.T_predictor]

    _STATE_KEYS = ("format", "kind", "layout", "model", "model_t", "T_predictor", "optimizer", "T_optimizer", "ema_t", "cm",
                   "epoch", "window_calls", "tail", "grads", "contrast", "meters")
    _LAYOUT_KEYS = ("num_classes", "step_per_update", "fused_tail", "ema_teacher", "use_contrastive", "contrast_samples")

    def layout(self):
        """The cfg keys that fix the layout of state_dict(), and the width of the segmentor's head feature (None: a
        segmentor without one)."""
        out = {k: self.cfg[k] for k in self._LAYOUT_KEYS}
        try:
            out["head_width"] = int(_unwrapped(self.model).segmentor.seg_head[1].num_features)
        except (AttributeError, IndexError, TypeError):
            out["head_width"] = None
        return out

    def _stepped(self):
        return {"model": self.model, "T_predictor": self.T_predictor}

    def state_dict(self):
        """Everything a resumed run needs of this step ("Checkpoints"): student, teacher and T_predictor
        (unwrapped), both optimizers in torch's own layout, ema_t, cm, the epoch, the open step_per_update window, the
        contrastive loss's bank and counters, the meters' buffers.  Copies made on the current stream, no synchronisation;
        between any two calls -- inside an open window too --, not under stream capture."""
        from . import checkpoint as ck
        ck.refuse_capture("FixMatchNTMStep")
        out = {"format": ck.FORMAT, "kind": "FixMatchNTMStep", "layout": self.layout(),
               "model": ck.module_state(self.model), "model_t": ck.module_state(self.model_t),
               "T_predictor": ck.module_state(self.T_predictor),
               "optimizer": ck.optimizer_state(self.optimizer), "T_optimizer": ck.optimizer_state(self.T_optimizer),
               "ema_t": ck.copied(self.ema_t), "cm": ck.copied(self.cm), "epoch": self.epoch,
               "contrast": self.contrast.state_dict() if self.contrast is not None else None,
               "meters": self.meters.state_dict() if self.meters is not None else None}
        out.update(self.window_state(self._stepped()))
        return out

    def load_state_dict(self, state):
        """state_dict()'s counterpart: everything is checked first (ValueError naming the key; the step is left as it was),
        then every tensor that exists is written in place -- a captured graph holds them -- and optimizer state that does not
        exist yet is created as the first eager call would.  The epoch is set as it was saved, WITHOUT restart_window(): the
        window is the saved one.  A queued look-ahead is dropped: the next call computes its batch work in line."""
        from . import checkpoint as ck
        r = ck.Restore()
        _check_head(r, state, self._STATE_KEYS, "FixMatchNTMStep", self.layout())
        for key, module in (("model", self.model), ("model_t", self.model_t), ("T_predictor", self.T_predictor)):
            r.module(key, module, state[key])
        tail = self.tail if self.fused else None
        r.optimizer("optimizer", self.optimizer, state["optimizer"], tail)
        r.optimizer("T_optimizer", self.T_optimizer, state["T_optimizer"], tail)
        r.tensor("ema_t", self.ema_t, state["ema_t"])
        r.tensor("cm", self.cm, state["cm"])
        epoch = state["epoch"]
        if epoch is not None:
            r.number("epoch", epoch, int)
        for key, part in (("contrast", self.contrast), ("meters", self.meters)):
            if (state[key] is None) != (part is None):
                raise ValueError("%s: %s key %r (the step is built %s it)"
                                 % ((key, "missing", key, "with") if part is not None else (key, "unexpected", key, "without")))
            if part is not None:
                part.restore(r, state[key], key)
        self.restore_window(r, state, self._stepped())

        def host():
            self.epoch = epoch
            self._geometry = (None, None)
        r.then(host)
        r.commit()

    def set_epoch(self, epoch):
        """The epoch of the iterations that follow (train.py's loop variable): above cfg switch_ep the pseudo labels come
        from the student's own weak view and the teacher no longer runs (train.py:469-475, 494-498).  Another epoch than the
        last: restart_window()."""
        epoch = None if epoch is None else int(epoch)
        if epoch != self.epoch:
            self.restart_window()
        self.epoch = epoch

    @property
    def self_labelling(self):
        """True after switch_ep: the phase in which the student labels its own weak view."""
        return self.epoch is not None and self.epoch > self.cfg["switch_ep"]

    @property
    def phase(self):
        """One of PHASES: who makes the pseudo labels now, and can that forward run ahead of the update before it."""
        return "@2" if self.self_labelling else "@e" if self.cfg["ema_teacher"] else ""

    def lookahead_keys(self, phase=None):
        """lookahead_keys() of a phase (default: the current one) under the step's cfg."""
        return lookahead_keys(self.phase if phase is None else phase, self.cfg)

    def check_meter_batch(self, data_u):
        """With the meters on, the unlabelled batch must carry its ground truth data_u["y"] on the meters' GPU: checked
        before anything of the iteration is queued (the meters' kernels read it through a raw device pointer)."""
        if self.meters is None:
            return
        y = data_u.get("y")
        if not torch.is_tensor(y):
            raise RuntimeError("FixMatchNTMStep(meters=...): the unlabelled batch carries no ground truth data_u['y']")
        if y.device != self.meters.counts.device:
            raise RuntimeError("FixMatchNTMStep(meters=...): data_u['y'] is on %s, the meters on %s -- move it to the GPU"
                               % (y.device, self.meters.counts.device))

    def __call__(self, data, data_u, next_batches=None):
        """data: labelled batch {pos (B_l,N,3), x (B_l,3,N), cls (B_l,1), y (B_l,N)}; data_u: unlabelled batch
        {pos_w, x_w, cls_w, pos_s, x_s, cls_s, raw_pos (B_u,N,3)} -> dict of detached losses.
        next_batches = (data', data_u') of the NEXT iteration when the loop already holds them: the coordinate-only work of
        the next student and teacher batches is queued behind this iteration's student forward (SupervisedStep's look-ahead;
        the caller must then pass exactly those dicts next time -- the positions are matched by identity and version
        counter, not trusted: WholePartSeg.forward refuses a geometry of other tensors, for the student and for the teacher
        alike, and the work is done in line)."""
        self.check_meter_batch(data_u)
        geoms, self._geometry = self._geometry, (None, None)
        with _accumulating(self, self.fused):
            losses, self._geometry = self.iteration(data, data_u, geoms, next_batches)
        return losses

    def _teacher_forward(self, data_u, geom_t):
        """train.py:462-475: the teacher on the weak view -> ((softmax, its maximum, its arg-max), with cfg use_contrastive
        the head feature of that forward (no_grad: a constant), taken off the module -- else None)."""
        with torch.no_grad():
            _mode(self.model_t, False)
            pred_u = F.softmax(self.model_t(data_u, if_teacher=True, geometry=geom_t)[0], dim=1)
            logits_u_aug, label_u_aug = torch.max(pred_u, dim=1)
        feat = None
        if self.contrast is not None:
            seg = _unwrapped(self.model_t).segmentor
            feat, seg.head_feature = seg.head_feature, None
        return (pred_u, logits_u_aug, label_u_aug), feat

    def _teacher_geometry(self, inner, geom_s, data, data_u, inline=False):
        """The teacher's geometry: the weak view is the last third of the student's batch, so its sampling / grouping / index
        work is a slice of the student's (WholePartSeg.weak_view_geometry; the teacher's own 8192-sample FPS was 4.7 ms on two
        CUs beside the student's); computed on its own only when there is nothing to slice (GEOT_SHARE_WEAK_GEOMETRY=0: always)."""
        g = None
        if self.share_weak_geometry and hasattr(inner, "weak_view_geometry"):
            g = inner.weak_view_geometry(geom_s, data, data_u)
        return g if g is not None else self.model_t.prefetch_geometry(data_u, if_teacher=True, inline=inline)

    def _refine_neighbours(self, data_u):
        """The neighbour table cfg pseudo_refine reads: the weak view's nearest neighbours (batch-only work)."""
        from .utils.pseudo_mask import neighbours
        return neighbours(data_u["pos_w"].contiguous(), self.cfg["pseudo_refine_size"])

    def lookahead_work(self, data, data_u, self_labelling=None):
        """Everything of an iteration that depends on its batches and on FROZEN state alone, on the CURRENT stream: the
        student's and the teacher's geometry, the teacher's forward -> pseudo labels (the teacher is never updated:
        train.py:218-222 loads and freezes it; it is in eval mode and draws no random numbers), the kNN graph and Morton
        order of the 3-D loss (and what the switches add: BatchWork).  -> the BatchWork student_iteration() takes.
        graph_step.py replays this as a graph of its own on a second stream beside the PREVIOUS iteration's training graph;
        the eager iteration() below spreads the same work over side streams inside the iteration instead.  After switch_ep
        (self_labelling; default: the step's epoch) the teacher does not run.  With cfg ema_teacher the teacher is no frozen
        state: before switch_ep the product holds its geometry and its forward runs inside the iteration."""
        return self._batch_work(data, data_u, self.self_labelling if self_labelling is None else self_labelling)

    def _forked(self, name, dev):
        """The step's side stream `name` (created on first use), put behind the current stream."""
        side = getattr(self, name) or torch.cuda.Stream(device=dev)
        setattr(self, name, side)
        side.wait_stream(torch.cuda.current_stream(dev))
        return side

    def _batch_work(self, data, data_u, self_labelling, geoms=None):
        """The batch-only work, listed once.  geoms None: in line -- everything on the current stream, the geometry included.
        geoms = (student, teacher) geometries the previous call queued, or Nones: the eager iteration -- the kNN graph and
        the refine table on self._side, the teacher's forward on self._teacher_stream (GEOT_TEACHER_STREAM=0: in line),
        to be joined by the product's first reader."""
        inline = geoms is None
        dev = data["pos"].device
        with torch.no_grad():
            if inline:
                _mode(self.model, True)
                inner = _unwrapped(self.model)
                geom_s, geom_t = inner.prefetch_geometry(data, data_u, fixmatch=True, inline=True), None
                if not self_labelling:
                    _mode(self.model_t, False)
                    geom_t = self._teacher_geometry(inner, geom_s, data, data_u, inline=True)
            else:
                geom_s, geom_t = geoms
            pre = BatchWork(geom_s)
            # the kNN graph of the 3-D loss needs raw_pos only: build it beside the teacher / student forwards
            if self.cfg["use_3d_loss"] or self.refine_mode is not None:
                side = None if inline else self._forked("_side", dev)
                with torch.cuda.stream(side):
                    if self.cfg["use_3d_loss"]:                   # (off: nobody reads the 3-D loss's graph)
                        raw = data_u["raw_pos"].contiguous()
                        pre.knn = (self.threed_loss.neighbours(raw), ntm_mod.spatial_order(raw))
                        pre.made_on(side, "knn")
                    if self.refine_mode is not None:      # the weak view's neighbour table: batch-only work, like the graph above
                        pre.refine_nbr = self._refine_neighbours(data_u)
                        pre.made_on(side, "refine_nbr")
        # 1. pseudo labels from the frozen teacher on the weak view (train.py:462-475).  The teacher's 2-cloud forward
        #    is short and mostly waits for its own 8192-sample FPS (4.7 ms on 2 CUs); nothing in the student's forward
        #    depends on it, so it is queued on a stream of its own and the student's kernels fill the gap (the eval-mode
        #    teacher draws no random numbers: identical results).  Its outputs are first used at step 3, after the join;
        #    next iteration's entry wait keeps the stream's allocations ordered behind this iteration's readers.
        #    After switch_ep there is no teacher: student_iteration takes the pseudo labels from the student's weak view.
        if self_labelling:
            return pre
        if self.cfg["ema_teacher"] and inline:
            # a teacher that moves with every update cannot run ahead of the update before it: its forward belongs to the
            # iteration itself (student_iteration runs it at its head); what depends on the batch alone is its geometry
            pre.geom_t = geom_t
        else:
            # (cfg ema_teacher: the fork's wait also puts the teacher's forward behind the previous iteration's update,
            # which wrote the teacher's weights on the current stream; the join behind the student's forward puts this
            # iteration's update behind the teacher's reads)
            t_stream = self._forked("_teacher_stream", dev) if self.overlap_teacher and not inline else None
            with torch.cuda.stream(t_stream):
                pre.pseudo, pre.feat_t = self._teacher_forward(data_u, geom_t)
            pre.made_on(t_stream, "pseudo", "feat_t")
        return pre

    def iteration(self, data, data_u, geoms=(None, None), next_batches=None):
        """One iteration, eagerly, its batch-only work spread over side streams -> (dict of detached losses, (student,
        teacher) geometries queued for next_batches; no teacher geometry after switch_ep)."""
        self_labelling = self.self_labelling
        pre = self._batch_work(data, data_u, self_labelling, geoms)
        inner = _unwrapped(self.model)
        make = None
        if next_batches is not None:
            nd, nu = next_batches

            def make():
                if not self_labelling:
                    _mode(self.model_t, False)
                g_s = inner.prefetch_geometry(nd, nu, fixmatch=True)
                return g_s, None if self_labelling else self._teacher_geometry(inner, g_s, nd, nu)
        look = _LookAhead(inner.segmentor, "forward", make)
        losses = self.student_iteration(data, data_u, pre, look.behind_forward)
        return losses, look.done() or (None, None)

    def student_iteration(self, data, data_u, pre, after_forward=None, defer_rest=False):
        """Steps 2-5 of the iteration (train.py:478-602, 646-660) over its batch-only work `pre` (a BatchWork): the student on
        labelled + strong + weak views, the class transition, the per-point matrices, the corrected logits, the losses,
        backward, both optimisers (and the meters).  pre.pseudo None before switch_ep (a moving teacher under replay): the
        teacher's forward runs here, at the head, in line, over pre.geom_t.  None after switch_ep: the labels are the soft-max
        of the student's weak-view slice and its maximum (train.py:494-498) -- from the DETACHED slice: the reference only
        ever uses detached copies of that pred_u (:498, :507), so autograd stays out of it.  after_forward(): called behind
        the student's forward and behind the read of pre.pseudo (the eager iteration queues its look-ahead there).
        defer_rest: stop where the backward reaches the student's transformer blocks (_Cut) and return (losses, rest) --
        backward_rest_update(rest) runs the rest of the backward, the EMA update and both optimisers (graph_step's split).
        cfg pseudo_refine: the refined mask is taken from the pred_u the class transition reads and goes to the unsupervised
        criterion as its mask= (train.py:500, 588-596); scale_factor keeps the unrefined threshold mask (:599-602); the losses
        gain "kept", the mask's sum.  cfg use_contrastive: the loss (utils/cluster_contrastloss.py) reads the student's
        strong-view slice against pre.feat_t (B_u, 128, N) -- None (after switch_ep): the student's own weak-view slice,
        detached -- both channel-first and in place, selects by logits_u_aug >= cfg cur_threshold with draws made on the
        device, and is added LAST, times cfg contrastive_loss_weight; the losses gain "contrast" and "anchors" (the number
        of anchors, a device tensor)."""
        cfg = self.cfg
        seg = getattr(_unwrapped(self.model), "segmentor", None)
        bl, bu = data["pos"].shape[0], data_u["pos_w"].shape[0]
        n = data["pos"].shape[1]
        pseudo = feat_t = None
        if not pre.made("pseudo") and not self.self_labelling:
            pseudo, feat_t = self._teacher_forward(data_u, pre.geom_t)
        # 2. student on labelled + strong + weak (train.py:478-492)
        _mode(self.model, True)
        _mode(self.T_predictor, True)
        data_u = dict(data_u, T=self.ema_t)
        with _Cut(seg, defer_rest) as cut:
            pred_all, _, sigma = _inner(self.model, self.grad_sync is not None)(data, u0=data_u, fixmatch=True, geometry=pre.geom_s)
        feat_all = None
        if self.contrast is not None:
            feat_all, seg.head_feature = seg.head_feature, None
        # (split, not two slices: its backward is one concatenation kernel; a slice's backward copies the gradient into a zero
        # tensor with a device-to-device memcpy -- a memcpy node when the iteration is captured)
        pred_l, pred_u_strong, pred_u_weak = torch.split(pred_all, [bl, bu, pred_all.shape[0] - bl - bu])
        # the teacher joins (the read of pre.pseudo) BEFORE the look-ahead is queued (after_forward): the look-ahead's side
        # streams (the student's and the teacher's segmentor streams) start behind the current stream only, and a teacher
        # forward without a prefetched geometry allocates its in-line index plan on the teacher segmentor's side stream and
        # frees it when the no_grad forward returns -- behind this join those blocks cannot be handed to the look-ahead's
        # kernels while the teacher's decoder still reads them (the teacher is long done by the end of the student's
        # forward: free)
        if pseudo is None:
            pseudo, feat_t = pre.pseudo, pre.feat_t
        if pseudo is None:
            with torch.no_grad():
                pred_u = F.softmax(pred_u_weak.detach(), dim=1)
                logits_u_aug, label_u_aug = torch.max(pred_u, dim=1)
            pseudo = (pred_u, logits_u_aug, label_u_aug)
        if after_forward is not None:
            after_forward()
        pred_u, logits_u_aug, label_u_aug = pseudo
        # 3. class-level transition matrix, prior, EMA (train.py:502-545, 556-557)
        ema_t_corr, ema_next, _, _ = ntm_mod.class_transition(
            pred_u, sigma, self.ema_t, cfg["geo_lambma"], cfg["ema_t_decay"], group=self.group,
            filter_outlier=cfg["filter_outlier"])
        # 4. per-point matrices + corrected strong logits (train.py:547-552)
        prob_s = F.softmax(pred_u_strong, dim=1).detach()
        ins_t = _inner(self.T_predictor, self.grad_sync is not None)(prob_s, self.cm)
        # (Poly1FocalLoss_U / Weight_CELoss_U read the uncorrected logits: the correction would have no reader)
        pred_u_strong_corr = ntm_mod.correct_logits(pred_u_strong, ins_t, ema_t_corr, cfg["lambma"]) \
            if self.needs_correction else None
        # 5. losses (train.py:560-602)
        loss_feat = loss_ident = loss_3d = None
        if cfg["use_feat_loss"]:
            loss_feat = self.feat_S_loss(prob_s, label_u_aug, ins_t) * cfg["feat_loss_weight"]
        if cfg["use_identity_loss"]:
            loss_ident = self.identity_loss(ins_t, self.Identity_t) * cfg["identity_loss_weight"]
        if cfg["use_3d_loss"]:
            nbr, order = pre.knn
            loss_3d = self.threed_loss(data_u["raw_pos"], label_u_aug, ins_t, nbr=nbr, order=order) * cfg["threed_loss_weight"]
        if self.criterion_name == "Weight_CELoss":
            sup_loss = self.criterion(pred_l, data["y"], data["class_weights"])
        else:
            sup_loss = self.criterion(pred_l, data["y"])
        conf, thresh = logits_u_aug.detach(), cfg["threshold"]
        mask = None                                             # train.py:500
        if self.refine_mode is not None:
            from .utils.pseudo_mask import pseudo_refine_mask
            mask = pseudo_refine_mask(pred_u, thresh, data_u["pos_w"], cfg["pseudo_refine_size"], cfg["pseudo_refine_neighbors"],
                                      mode=self.refine_mode, nbr=pre.refine_nbr)
        if self.criterion_u_name == "Weight_CELoss_U":          # (the labelled batch's weights: train.py:585-587)
            unsup_loss = self.criterion_u(pred_u_strong, label_u_aug.detach(), data["class_weights"], conf, thresh=thresh)
        elif self.criterion_u_name == "Poly1FocalLoss_U":
            unsup_loss = self.criterion_u(pred_u_strong, label_u_aug.detach(), conf, thresh=thresh, mask=mask)
        elif self.criterion_u_name == "Poly1FocalLoss_U_corr":
            unsup_loss = self.criterion_u(pred_u_strong_corr, label_u_aug.detach(), conf, thresh=thresh, mask=mask)
        else:                                                   # Poly1FocalLoss_U_T
            unsup_loss = self.criterion_u(pred_u_strong, label_u_aug.detach(), conf, self.ema_t, pred_u_strong_corr,
                                          thresh=thresh, mask=mask)
        thresh_mask = logits_u_aug.ge(cfg["threshold"])
        unsup_loss = unsup_loss * (cfg["unsupervised_loss_weight"] * (bu * n) / thresh_mask.sum())
        loss = sup_loss + unsup_loss                            # train.py:646-655, in its order
        if loss_feat is not None:
            loss = loss + loss_feat
        if loss_ident is not None:
            loss = loss + loss_ident
        if loss_3d is not None:
            loss = loss + loss_3d
        loss_contrast = None
        if self.contrast is not None:
            # (split, as above: all three pieces, so that the backward is one concatenation kernel)
            _, feat_strong, feat_weak = torch.split(feat_all, [bl, bu, feat_all.shape[0] - bl - bu])
            if feat_t is None:
                feat_t = feat_weak.detach()
            loss_contrast = self.contrast(feat_strong, logits_u_aug.detach(), feat_t, channels_first=True)[0]
            loss = loss + cfg["contrastive_loss_weight"] * loss_contrast
        if self.meters is not None:
            if "y" not in data_u:
                raise RuntimeError("FixMatchNTMStep(meters=...): the unlabelled batch carries no ground truth data_u['y']")
            # (3-D loss off: the reference meters torch.tensor([0.]).item())
            self.meters.update(label_u_aug, logits_u_aug, data_u["y"], prob_s, loss, sup_loss, unsup_loss,
                               loss_3d if loss_3d is not None else torch.zeros((), device=loss.device), ema_t_corr,
                               feat=loss_feat, identity=loss_ident)
        loss.backward()
        rest = (cut.rest(), ema_next)
        losses = {"loss": loss.detach(), "sup": sup_loss.detach(), "unsup": unsup_loss.detach(),
                  "threed": loss_3d.detach() if loss_3d is not None else torch.zeros((), device=loss.device)}
        if loss_feat is not None:
            losses["feat"] = loss_feat.detach()
        if loss_ident is not None:
            losses["identity"] = loss_ident.detach()
        if mask is not None:
            losses["kept"] = mask.sum()
        if loss_contrast is not None:
            losses["contrast"], losses["anchors"] = loss_contrast.detach(), self.contrast.anchors
        if cfg["fused_tail"] and cfg["grad_norm_clip"] is not None:
            losses["grad_norm"] = self.tail.total_norm       # (a device scalar the tail rewrites: read it behind the update)
        if defer_rest:
            return losses, rest
        self.backward_rest_update(rest)
        return losses

    def forward_backward_head(self, data, data_u, pre):
        """As SupervisedStep's: up to where the backward reaches the student's blocks -> (losses, what backward_rest_update needs)."""
        return self.student_iteration(data, data_u, pre, defer_rest=True)

    def backward_rest_update(self, rest):
        """The rest of the backward (the blocks, the patch encoder), the EMA transition matrix, clipping, both optimisers.
        rest = (what _Cut left or None, the next ema_t)."""
        backward_rest(rest[0])
        with torch.no_grad():
            # in its buffer, never rebound (a captured replay holds this very tensor, and so do the meters), behind everything
            # that read the old one; a kernel, not a memcpy node (x 1.0 is exact)
            torch.mul(rest[1], 1.0, out=self.ema_t)
        _window_update(self, self.clip, self.model, self.fused)


def build_fixmatch(device, seg_cfg=None, cfg=None, use_ddp=True, group=None, graph_sync=False, min_world=2, meters=None):
    """Student, frozen teacher and T_predictor as train.py:154-226 builds them (random init: the pretrained
    checkpoints are the authors' local files).  graph_sync: the data-parallel form for a replay from hipGraphs -- bare
    SyncBatchNorm-converted modules + one flat gradient all-reduce (sync_only / GradSync) instead of DDP wrappers.
    meters: see FixMatchNTMStep."""
    from .openpoints.models.backbone.transformer import TOOTH_SEG_CFG
    import torch.distributed as dist
    check_cfg(dict(NTM_CFG, **(cfg or {})))            # a bad cfg is refused before any module goes to the device
    unused = unused_parameters(cfg)
    if graph_sync and ("sigma" in unused or "T_predictor.*" in unused):
        # GradSync sizes its one flat all-reduce by the gradients that exist when it is called: a synchronised parameter
        # that never gets one is the case in which ranks can meet with buffers of different sizes -- a hang, or corruption
        # inside a captured graph, not an error.  The multi-rank run of the non-default switches is out of scope: refuse.
        raise RuntimeError("build_fixmatch(graph_sync=True): under this cfg %s receive no gradient (unused_parameters(cfg)); "
                           "the flat gradient exchange of a replayed step expects one for every synchronised parameter -- "
                           "build the step without graph_sync (one rank, or eager DDP)"
                           % ", ".join(u for u in unused if u in ("sigma", "T_predictor.*")))
    world = dist.is_available() and dist.is_initialized() and dist.get_world_size() >= min_world
    seg = dict(NAME="PointTransformer_seg_T", **(seg_cfg or TOOTH_SEG_CFG))
    student = WholePartSeg(segmentor_args=seg).to(device)
    teacher = WholePartSeg(segmentor_args=seg).to(device)
    teacher.load_state_dict(student.state_dict())
    t_pred = ntm_mod.Ins_T_mean(nclasses=(cfg or NTM_CFG).get("num_classes", 17)).to(device)
    if graph_sync:
        student = sync_only(student, min_world=min_world)
        step = FixMatchNTMStep(student, teacher, t_pred, cfg=cfg, group=group, meters=meters)
        if world:
            step.grad_sync = GradSync([student, t_pred], group)
        return step
    if use_ddp:
        student = ddp(student, device, unused=[u for u in unused if u != "T_predictor.*"], min_world=min_world)
        if "T_predictor.*" in unused:
            t_pred = ddp(t_pred, device, sync_bn=False, unused=[n for n, _ in t_pred.named_parameters()], min_world=min_world)
        else:
            t_pred = ddp(t_pred, device, sync_bn=False, min_world=min_world)
    return FixMatchNTMStep(student, teacher, t_pred, cfg=cfg, group=group, meters=meters)
