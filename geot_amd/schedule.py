"""The configured learning-rate schedule, in device memory.

    schedule = LrSchedule(step.optimizers(), cfg)        # every group's lr becomes a one-element float32 device tensor
    ...                                                  # an epoch, eager or replayed
    schedule.step(epoch)                                 # fill_: the tensors a captured AdamW reads are written, never rebound

cfgs/tooth_semi/*.yaml configure `sched: multistep`, `decay_epochs: [210, 270]` / `[220]`, `decay_rate: 0.1`,
`sched_on_epoch: True`; the reference builds openpoints/scheduler/multistep_lr.py MultiStepLRScheduler from them
(scheduler_factory.py build_scheduler_from_cfg) and calls `scheduler.step(epoch)` behind every epoch
(examples/segmentation/train.py:333-338), which writes python floats into the parameter groups.  A python float is baked into a
captured AdamW step (geot_amd/graph_step.py), so here the groups hold tensors and the schedule fills them.

The values are MultiStepLRScheduler.get_epoch_values' (multistep_lr.py:44-59), in python floats, operation for operation:
below warmup_epochs `warmup_lr + t * ((base - warmup_lr) / warmup_epochs)`, from there `base * decay_rate **
bisect_right(decay_epochs, t + 1)`; tests/golden/lr_schedule_ref.npz holds what the reference's class returns.  `step(t)` is
called BEHIND epoch t and sets the rate of epoch t + 1; the first epoch of a run trains at values(0).

The schedule is a pure function of the epoch: a resumed run calls step(epoch) and nothing of it goes into a checkpoint.
"""
import bisect

import numpy as np
import torch

SCHEDULES = ("multistep",)


def _cfg(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


class LrSchedule:
    def __init__(self, optimizers, cfg, device=None):
        """optimizers: an optimizer or a list of them (a step's optimizers()).  cfg (a dict or an object with attributes)
        is read as build_scheduler_from_cfg reads it: lr, sched, decay_epochs, decay_rate, warmup_epochs (0), warmup_lr
        (1e-6), min_lr (lr / 1000; read and unused by multistep, as there); lr_noise and sched_on_epoch: False are refused,
        and so is every sched but "multistep" (NotImplementedError, before a group is touched).  device: where the tensors
        go (default: the device of the group's first parameter).

        Every group's lr becomes a one-element float32 tensor holding values(0); a group whose lr is a tensor already keeps
        THAT tensor (a captured graph, OptimTail and checkpoint.Restore may hold it).  The base value of a group is its
        `initial_lr` when a scheduler left one, else its lr -- for a tensor lr cfg.lr when that is the number the tensor
        holds in float32, so that the schedule starts from the configured double -- and is recorded as `initial_lr`, as the
        reference's Scheduler does (geot_amd/checkpoint.py carries the key)."""
        sched = _cfg(cfg, "sched")
        if sched not in SCHEDULES:
            raise NotImplementedError("LrSchedule: sched=%r is not built (only %s)" % (sched, ", ".join(SCHEDULES)))
        if _cfg(cfg, "lr_noise") is not None:
            raise NotImplementedError("LrSchedule: lr_noise=%r is not built" % (_cfg(cfg, "lr_noise"),))
        if not _cfg(cfg, "sched_on_epoch", True):
            raise NotImplementedError("LrSchedule: sched_on_epoch=False (a step per update) is not built")
        self.sched = sched
        self.lr = _cfg(cfg, "lr")
        decay = _cfg(cfg, "decay_epochs", 1)
        self.decay_t = [int(t) for t in (decay if isinstance(decay, (list, tuple)) else [decay])]
        if self.decay_t != sorted(self.decay_t):
            raise ValueError("LrSchedule: decay_epochs must be sorted, got %r" % (decay,))
        rate = _cfg(cfg, "decay_rate")
        if rate is None:
            raise ValueError("LrSchedule: cfg decay_rate is missing")
        self.decay_rate = rate
        self.warmup_t = int(_cfg(cfg, "warmup_epochs", 0) or 0)
        self.warmup_lr_init = _cfg(cfg, "warmup_lr", 1.0e-6)
        self.min_lr = _cfg(cfg, "min_lr") or (self.lr / 1000.0 if self.lr is not None else None)
        if isinstance(optimizers, torch.optim.Optimizer):
            optimizers = [optimizers]
        self.groups = [group for opt in optimizers for group in opt.param_groups]
        self.base_values = []
        for group in self.groups:
            base = group.get("initial_lr")
            if base is None:
                base = group["lr"]
                if torch.is_tensor(base):
                    held = float(base)
                    base = self.lr if self.lr is not None and float(np.float32(self.lr)) == held else held
            group["initial_lr"] = base = float(base)
            self.base_values.append(base)
        self.warmup_steps = [(v - self.warmup_lr_init) / self.warmup_t if self.warmup_t else 1 for v in self.base_values]
        first = self.values(0)
        self.tensors = []
        for group, value in zip(self.groups, first):
            lr = group["lr"]
            if torch.is_tensor(lr):
                lr.fill_(value)
            else:
                dev = device if device is not None else group["params"][0].device
                lr = group["lr"] = torch.full((), value, dtype=torch.float32, device=dev)
            self.tensors.append(lr)
        self.epoch = 0

    def values(self, epoch):
        """The python floats get_epoch_values(epoch) returns, one per group (host only)."""
        t = int(epoch)
        if t < self.warmup_t:
            return [self.warmup_lr_init + t * s for s in self.warmup_steps]
        return [v * (self.decay_rate ** bisect.bisect_right(self.decay_t, t + 1)) for v in self.base_values]

    def step(self, epoch):
        """Behind epoch `epoch`: its values go into the groups' tensors in place, one fill_ per group."""
        for lr, value in zip(self.tensors, self.values(epoch)):
            lr.fill_(value)
        self.epoch = int(epoch)
