"""The reference's checkpoint files -- mirror of ``save_checkpoint`` / ``resume_checkpoint`` / ``load_checkpoint`` of
openpoints/utils/ckpt_util.py, which examples/segmentation/train.py calls at :180-203 (resume, pretrained weights) and :342
(every epoch).  Written from the format, which tests/golden/ckpt_ref.* pins by executing the reference's own functions:

    {"model": state_dict, "optimizer": state_dict, "scheduler": state_dict, "epoch": int, **additional}

as one torch.save pickle named <ckpt_dir>/<run_name>_<post_fix>.pth.  Files the authors' code wrote (``pretrained_path``)
load here and files written here load there; the model is stored unwrapped, and a loader takes keys with or without a
DistributedDataParallel ``module.`` prefix.

Beyond the reference: save_checkpoint(step=...) stores the package's own training state (geot_amd/checkpoint.py: a step's
state_dict()) under the key ``geot_amd_step``, which the reference's loaders pass over, and resume_checkpoint(step=...)
restores it when the file carries it.  Files are read with torch.load(weights_only=True); a file that holds other python
objects (a numpy scalar as best_val) needs weights_only=False, for files whose origin is trusted.
"""
import logging
import os
import pickle
import shutil

import torch

WRAPPER_KEYS = ("model", "net", "network", "state_dict", "base_model")
METRIC_WORDS = ("metric", "miou", "dsc", "acc", "test", "val")
STEP_KEY = "geot_amd_step"


def _bare(model):
    return model.module if hasattr(model, "module") else model


def _cfg(cfg, name, default=None):
    return cfg.get(name, default) if isinstance(cfg, dict) else getattr(cfg, name, default)


def _read(path, weights_only):
    try:
        return torch.load(path, map_location="cpu", weights_only=weights_only)
    except pickle.UnpicklingError as e:
        if not weights_only:
            raise
        raise RuntimeError("%s holds python objects torch.load(weights_only=True) does not read; pass weights_only=False "
                           "if the file's origin is trusted (%s)" % (path, str(e).splitlines()[0])) from e


def save_checkpoint(cfg, model, epoch, optimizer=None, scheduler=None, additioanl_dict=None, is_best=False,
                    post_fix="ckpt_latest", save_name=None, step=None, additional_dict=None):
    """Write <cfg.ckpt_dir>/<save_name or cfg.run_name>_<post_fix>.pth -> its path.  additioanl_dict (the reference's
    spelling; additional_dict is taken too): further top-level entries, e.g. {"best_val": ...}.  cfg.save_freq > 0: a copy
    named ..._E<epoch>.pth every save_freq epochs; is_best: a copy named ..._ckpt_best.pth.  step: a training step of this
    package, stored under "geot_amd_step".  A post_fix containing "clean" stores the encoder alone ("encoder." stripped)."""
    name = save_name if save_name is not None else _cfg(cfg, "run_name")
    folder = _cfg(cfg, "ckpt_dir")
    path = os.path.join(folder, "%s_%s.pth" % (name, post_fix))
    weights = _bare(model).state_dict()
    if "clean" in post_fix:
        out = {"model": {k[len("encoder."):]: v for k, v in weights.items() if k.startswith("encoder.")}}
    else:
        out = {"model": weights,
               "optimizer": optimizer.state_dict() if optimizer is not None else {},
               "scheduler": scheduler.state_dict() if scheduler is not None else {},
               "epoch": epoch}
        for more in (additioanl_dict, additional_dict):
            if more:
                out.update(more)
        if step is not None:
            from ... import checkpoint
            out[STEP_KEY] = checkpoint.numbers_only(step.state_dict())
    torch.save(out, path)
    every = _cfg(cfg, "save_freq", 0) or 0
    if every > 0 and epoch % every == 0:
        shutil.copyfile(path, os.path.join(folder, "%s_E%d.pth" % (name, epoch)))
    if is_best:
        shutil.copyfile(path, os.path.join(folder, "%s_ckpt_best.pth" % name if name else "ckpt_best.pth"))
    return path


def _match_prefix(weights, model):
    """The file's keys spelled the way `model` spells its own: with or without a leading ``module.``."""
    own = next(iter(model.state_dict()), "")
    wrapped = own.startswith("module.")
    out = {}
    for k, v in weights.items():
        if k.startswith("module.") and not wrapped:
            k = k[len("module."):]
        elif wrapped and not k.startswith("module."):
            k = "module." + k
        out[k] = v
    return out


def resume_checkpoint(config, model, optimizer=None, scheduler=None, pretrained_path=None, printer=logging.info, step=None,
                      weights_only=True):
    """Continue a run from a file save_checkpoint wrote -> (start_epoch, best_val or None), and config.start_epoch =
    config.epoch = the file's epoch + 1.  The model is loaded strictly; an optimizer or scheduler state that does not fit is
    reported through `printer` and skipped, as the reference does.  step: a training step of this package -- when the file
    carries its state ("geot_amd_step") it is restored through step.load_state_dict(): in place, model and optimizers
    included, so `model` / `optimizer` are then loaded from that entry and may be left out."""
    path = pretrained_path if pretrained_path is not None else _cfg(config, "pretrained_path")
    if path is None:
        raise ValueError("resume_checkpoint: no pretrained_path")
    printer("=> loading checkpoint '%s'" % path)
    ckpt = _read(path, weights_only)
    start = ckpt["epoch"] + 1
    if step is not None and STEP_KEY in ckpt:
        step.load_state_dict(ckpt[STEP_KEY])
    else:
        for what, obj in (("optimizer", optimizer), ("scheduler", scheduler)):
            if obj is not None:
                try:
                    obj.load_state_dict(ckpt[what])
                except Exception:
                    printer("%s does not match" % what)
        if model is not None:
            model.load_state_dict(_match_prefix(ckpt["model"], model))
    if isinstance(config, dict):
        config["start_epoch"] = config["epoch"] = start
    else:
        config.start_epoch = config.epoch = start
    best = ckpt.get("best_val")
    printer("=> loaded successfully '%s' (epoch %s, best val %s)" % (path, ckpt["epoch"], best))
    return start, best


def load_checkpoint(model, pretrained_path, prefix=None, module=None, return_pretrained_keys=False, weights_only=True):
    """Pretrained weights into `model`, non-strictly -> (epoch or -1, {key: value} of the file's metric entries).  The
    file is a bare state dict or holds one under "model" / "net" / "network" / "state_dict" / "base_model"; ``module.`` is
    stripped from its keys; module: keep the keys containing it; prefix: prepended to every key.  Missing and unexpected
    keys are logged.  return_pretrained_keys: -> the keys of the file's "model" entry instead."""
    if not os.path.exists(pretrained_path):
        raise NotImplementedError("no checkpoint file from path %s..." % pretrained_path)
    ckpt = _read(pretrained_path, weights_only)
    weights = ckpt
    for key in WRAPPER_KEYS:
        if key in ckpt and isinstance(ckpt[key], dict):
            weights = ckpt[key]
    weights = {k.replace("module.", ""): v for k, v in weights.items()}
    if module is not None:
        weights = {k: v for k, v in weights.items() if module in k}
    if prefix is not None:
        weights = {prefix + k: v for k, v in weights.items()}
    result = _bare(model).load_state_dict(weights, strict=False)
    logging.info("missing_keys: %s", ", ".join(result.missing_keys) or "none")
    logging.info("unexpected_keys: %s", ", ".join(result.unexpected_keys) or "none")
    epoch = ckpt.get("epoch", -1)
    metrics = {k: v for k, v in ckpt.items() if any(word in k for word in METRIC_WORDS)}
    logging.info("ckpts @ %s epoch( %s )", epoch, metrics)
    if return_pretrained_keys:
        return ckpt["model"].keys()
    return epoch, metrics
