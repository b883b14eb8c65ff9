"""Saving and resuming a training run, bit for bit: k calls, save, load, k more calls give the bits of 2k calls -- for the
eager steps of train_step.py and for their replays from hipGraphs (graph_step.py) alike.

    checkpoint.save(path, step, draws=(draws,), rng_device=device, epoch=epoch)      # between any two calls of the step
    ...
    extra = checkpoint.load(path, step, draws=(draws,))                              # -> {"epoch": epoch}

`step` is a SupervisedStep, a FixMatchNTMStep or one of their graphed wrappers; what its state_dict() holds, and why, is
listed in INTEGRATION.md ("Checkpoints").  The reference saves a model, an optimizer and a scheduler per epoch
(openpoints/utils/ckpt_util.py, called from examples/segmentation/train.py:180-203, 342: mirrored in
geot_amd/openpoints/utils/ckpt_util.py); it has no counterpart for the state this package added to its loop.

Two rules carry the design:

* state_dict() COPIES on the current stream and never synchronises: it may be called between any two calls of a step,
  inside an open step_per_update window too, and a later call does not change what it returned.
* load_state_dict() VALIDATES everything first (Restore below: every key, shape and dtype; a ValueError names the key) and
  then restores strictly IN PLACE -- copy_ into the tensors that exist.  A captured graph holds those very tensors, so no
  tensor is ever rebound, and torch.optim.Optimizer.load_state_dict (which rebinds every state tensor) is not used.

The file is one torch.save of tensors, numbers, strings, lists, dicts and None: torch.load(path, weights_only=True) reads it.
"""
import os
import random
import tempfile

import numpy as np
import torch

FORMAT = 1        # of a step's state_dict() and of save()'s file


# ---- copying out ----------------------------------------------------------------------------------------------------------
def refuse_capture(what):
    """state_dict() allocates and copies: not under stream capture (the copies would become nodes of the graph)."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("%s.state_dict(): called under stream capture -- take the state between two calls of the step" % what)


def copied(t):
    """A copy of a tensor made on the current stream (no synchronisation)."""
    return t.detach().clone()


def module_state(module):
    """The unwrapped module's state_dict(), copied: a DistributedDataParallel wrapper adds no `module.` prefix."""
    module = module.module if hasattr(module, "module") else module
    return {k: copied(v) for k, v in module.state_dict().items()}


_GROUP_RUNTIME = ("capturable", "fused", "foreach", "differentiable")      # how the TARGET executes: never restored
_GROUP_OPTIONAL = _GROUP_RUNTIME + ("initial_lr",)                         # (a scheduler's mark: there with one attached)


def optimizer_state(optimizer):
    """optimizer.state_dict() in torch's own layout -- {"state": {index: {...}}, "param_groups": [{..., "params": [index]}]} --
    with every tensor copied.  A device-tensor lr is copied as a tensor (reading it would synchronise); numbers_only() turns
    it into a number where the state leaves the process."""
    index, groups = {}, []
    for group in optimizer.param_groups:
        out = {}
        for k, v in group.items():
            if k == "params":
                out[k] = [index.setdefault(id(p), len(index)) for p in v]
            elif torch.is_tensor(v):
                out[k] = copied(v)
            else:
                out[k] = list(v) if isinstance(v, tuple) else v
        groups.append(out)
    state = {}
    for p, st in optimizer.state.items():
        if id(p) in index:
            state[index[id(p)]] = {k: copied(v) if torch.is_tensor(v) else v for k, v in st.items()}
    return {"state": state, "param_groups": groups}


def numbers_only(state):
    """The state with every param group's tensor lr turned into a python number (one synchronising read each: done where
    the state is written to a file, which synchronises anyway) -- a plain torch.optim.AdamW then loads the entry."""
    if isinstance(state, dict):
        if "param_groups" in state and "state" in state:
            groups = [dict(g, lr=float(g["lr"])) if torch.is_tensor(g.get("lr")) else g for g in state["param_groups"]]
            return dict(state, param_groups=groups)
        return {k: numbers_only(v) for k, v in state.items()}
    return state


# ---- copying in -------------------------------------------------------------------------------------------------------------
class Restore:
    """A load in two halves.  The first collects: every tensor to write with its source (checked: a tensor of that shape and
    dtype) and every host action, under the key that names it in an error.  commit() runs them -- only when nothing has
    raised, so a refused state leaves its target untouched."""

    def __init__(self):
        self.copies, self.actions = [], []

    def keys(self, state, expected, where, optional=()):
        if not isinstance(state, dict):
            raise ValueError("%s: expected a dict, got %s" % (where or "state", type(state).__name__))
        for k in expected:
            if k not in state:
                raise ValueError("%s: missing key %r" % (where or "state", k))
        for k in state:
            if k not in expected and k not in optional:
                raise ValueError("%s: unexpected key %r" % (where or "state", k))

    def check(self, key, dst, src):
        if not torch.is_tensor(src):
            raise ValueError("%s: expected a tensor, got %s" % (key, type(src).__name__))
        if tuple(src.shape) != tuple(dst.shape):
            raise ValueError("%s: shape %s, the step holds %s" % (key, tuple(src.shape), tuple(dst.shape)))
        if src.dtype != dst.dtype:
            raise ValueError("%s: dtype %s, the step holds %s" % (key, src.dtype, dst.dtype))

    def tensor(self, key, dst, src):
        """dst.copy_(src) at commit."""
        self.check(key, dst, src)
        self.copies.append((dst, src))

    def number(self, key, value, kinds=(int, float)):
        if isinstance(value, bool) or not isinstance(value, kinds):
            raise ValueError("%s: expected a number, got %r" % (key, value))
        return value

    def then(self, fn):
        self.actions.append(fn)

    def module(self, key, module, state):
        module = module.module if hasattr(module, "module") else module
        own = module.state_dict(keep_vars=True)
        self.keys(state, list(own), key)
        for k, dst in own.items():
            self.tensor("%s.%s" % (key, k), dst, state[k])

    def optimizer(self, key, optimizer, state, tail=None):
        """An optimizer_state() entry into `optimizer`, in place.  State that does not exist yet is created as the first
        eager step would create it -- by `tail` (an OptimTail run as its fused pass: its step counters are views of one flat
        tensor) or as torch.optim.AdamW._init_group does -- and then filled.  State the optimizer holds and the entry lacks
        cannot be restored in place (dropping it would rebind): refused."""
        self.keys(state, ("state", "param_groups"), key)
        groups, saved = state["param_groups"], state["state"]
        if not isinstance(groups, list) or len(groups) != len(optimizer.param_groups):
            raise ValueError("%s.param_groups: %s groups, the optimizer has %d"
                             % (key, len(groups) if isinstance(groups, list) else type(groups).__name__, len(optimizer.param_groups)))
        params, at = [], 0
        for gi, (group, own) in enumerate(zip(groups, optimizer.param_groups)):
            where = "%s.param_groups[%d]" % (key, gi)
            self.keys(group, [k for k in own if k not in _GROUP_OPTIONAL], where, optional=_GROUP_OPTIONAL)
            if list(group["params"]) != list(range(at, at + len(own["params"]))):
                raise ValueError("%s.params: %r, the optimizer's group holds parameters %d..%d"
                                 % (where, group["params"], at, at + len(own["params"]) - 1))
            at += len(own["params"])
            params.extend(own["params"])
            for k, v in group.items():
                if k == "params" or k in _GROUP_RUNTIME:
                    continue
                if k == "lr":
                    self._lr(where + ".lr", own, v)
                elif torch.is_tensor(own.get(k)):
                    self.tensor("%s.%s" % (where, k), own[k], v)
                else:
                    self.then(lambda own=own, k=k, v=v: own.__setitem__(k, tuple(v) if isinstance(own.get(k), tuple) else v))
        if not isinstance(saved, dict):
            raise ValueError("%s.state: expected a dict, got %s" % (key, type(saved).__name__))
        for i in saved:
            if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < len(params):
                raise ValueError("%s.state: unexpected key %r (the optimizer has parameters 0..%d)" % (key, i, len(params) - 1))
        fresh = []
        for i, p in enumerate(params):
            have = optimizer.state.get(p)          # (.get: the defaultdict must not grow an entry here)
            where = "%s.state[%d]" % (key, i)
            if i not in saved:
                if have:
                    raise ValueError("%s: missing key %d (the optimizer holds state for that parameter)" % (key + ".state", i))
                continue
            entry = saved[i]
            self.keys(entry, ("step", "exp_avg", "exp_avg_sq"), where)
            for k in ("exp_avg", "exp_avg_sq"):
                self.check("%s.%s" % (where, k), p, entry[k])
                if p.dtype != entry[k].dtype:
                    raise ValueError("%s.%s: dtype %s, the parameter is %s" % (where, k, entry[k].dtype, p.dtype))
            step = entry["step"]
            if torch.is_tensor(step):
                if step.numel() != 1:
                    raise ValueError("%s.step: shape %s, expected one number" % (where, tuple(step.shape)))
            else:
                self.number(where + ".step", step)
            if not have:
                fresh.append(i)
        if fresh:
            self.then(lambda: _create_state(optimizer, params, fresh, tail))
        # (read at commit: the entries may only exist once _create_state has run)
        for i in sorted(saved):
            self.then(lambda p=params[i], entry=saved[i]: _fill_state(optimizer.state[p], entry))

    def _lr(self, key, group, value):
        own = group["lr"]
        if torch.is_tensor(value):
            if value.numel() != 1:
                raise ValueError("%s: shape %s, expected one number" % (key, tuple(value.shape)))
        else:
            self.number(key, value)
        if torch.is_tensor(own):          # a device lr: a captured step reads this very tensor
            self.then(lambda: own.copy_(value.reshape(own.shape)) if torch.is_tensor(value) else own.fill_(float(value)))
        else:
            self.then(lambda: group.__setitem__("lr", float(value)))

    def commit(self):
        with torch.no_grad():
            for dst, src in self.copies:
                dst.copy_(src)
            for fn in self.actions:
                fn()


def _create_state(optimizer, params, fresh, tail):
    if tail is not None:
        where = {id(p): i for i, (p, _, _) in enumerate(tail.params)}
        tail.create_state([where[id(params[i])] for i in fresh])
        return
    for i in fresh:
        p = params[i]
        group = next(g for g in optimizer.param_groups if any(q is p for q in g["params"]))
        st = optimizer.state[p]
        # torch.optim.AdamW._init_group
        st["step"] = (torch.zeros((), dtype=torch.float32, device=p.device) if group.get("capturable") or group.get("fused")
                      else torch.tensor(0.0, dtype=torch.float32))
        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)


def _fill_state(own, entry):
    for k in ("exp_avg", "exp_avg_sq"):
        own[k].copy_(entry[k])
    step = entry["step"]
    if torch.is_tensor(own["step"]):
        if torch.is_tensor(step):
            own["step"].copy_(step.reshape(own["step"].shape))
        else:
            own["step"].fill_(float(step))
    else:
        own["step"] = float(step)


def same_layout(saved, own, where="layout"):
    """The cfg keys that fix the layout of a state must agree: a ValueError names the first that does not."""
    r = Restore()
    r.keys(saved, list(own), where)
    for k, v in own.items():
        if saved[k] != v:
            raise ValueError("%s.%s: the state was saved with %r, the step is built with %r" % (where, k, saved[k], v))


# ---- the generators a run reads ---------------------------------------------------------------------------------------------
def rng_state(device=None):
    """The state of the four generators a run reads -- torch's CPU generator, numpy's and python's global ones, and the
    CUDA generator of `device` (None: left out) that dropout and DropPath draw from -- as tensors, numbers and lists."""
    kind, key, pos, has_gauss, cached = np.random.get_state()
    version, words, gauss_next = random.getstate()
    cuda = None
    if device is not None:
        device = torch.device(device)
        cuda = {"device": str(device), "state": torch.cuda.get_rng_state(device)}
    return {"torch": torch.get_rng_state(),
            "numpy": {"kind": kind, "key": torch.from_numpy(key.astype(np.int64)), "pos": int(pos), "has_gauss": int(has_gauss),
                      "cached_gaussian": float(cached)},
            "python": {"version": int(version), "words": list(words), "gauss_next": gauss_next},
            "cuda": cuda}


def _check_rng(state):
    r = Restore()
    r.keys(state, ("torch", "numpy", "python", "cuda"), "rng")
    r.keys(state["numpy"], ("kind", "key", "pos", "has_gauss", "cached_gaussian"), "rng.numpy")
    r.keys(state["python"], ("version", "words", "gauss_next"), "rng.python")
    if state["cuda"] is not None:
        r.keys(state["cuda"], ("device", "state"), "rng.cuda")


def set_rng_state(state):
    """Restore what rng_state() took.  The CUDA generator is written in place (seed and offset): a captured graph reads
    both anew at every replay, so replays that follow continue the saved sequence."""
    _check_rng(state)
    torch.set_rng_state(state["torch"].cpu())
    n = state["numpy"]
    key = n["key"].cpu().numpy() if torch.is_tensor(n["key"]) else np.asarray(n["key"])
    np.random.set_state((n["kind"], key.astype(np.uint32), int(n["pos"]), int(n["has_gauss"]), float(n["cached_gaussian"])))
    p = state["python"]
    random.setstate((int(p["version"]), tuple(int(w) for w in p["words"]), p["gauss_next"]))
    if state["cuda"] is not None:
        torch.cuda.set_rng_state(state["cuda"]["state"].cpu(), torch.device(state["cuda"]["device"]))


# ---- one file ---------------------------------------------------------------------------------------------------------------
def save(path, step, draws=(), rng_device=None, **extra):
    """One file: the step's state_dict(), the state() of every DeviceDraws in `draws`, the generators (rng_state(rng_device))
    when rng_device is given, and `extra` (tensors, numbers, strings, lists, dicts, None: epoch, metrics, a scheduler's
    state_dict()).  Written under a temporary name in the same directory and renamed over `path`: a reader never sees a
    partial file, and a failed write leaves an earlier checkpoint as it was.  Take it before the next batch is drawn
    (with a loader that looks one batch ahead, the generators are those of the batch the resumed loop redraws)."""
    state = {"format": FORMAT, "step": numbers_only(step.state_dict()), "draws": [d.state() for d in draws],
             "rng": rng_state(rng_device) if rng_device is not None else None, "extra": extra}
    path = os.fspath(path)
    fd, tmp = tempfile.mkstemp(dir=os.path.dirname(os.path.abspath(path)), prefix=os.path.basename(path) + ".", suffix=".tmp")
    try:
        with os.fdopen(fd, "wb") as fh:
            torch.save(state, fh)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise


def load(path, step, draws=(), restore_rng=True, map_location="cpu"):
    """The counterpart of save() -> `extra`.  Everything is checked before anything is written: the file's format, the
    number of draws, and the step's state (its load_state_dict raises ValueError naming the key and leaves the step as it
    was).  restore_rng=False leaves the generators alone (a file saved without rng_device holds none)."""
    state = torch.load(os.fspath(path), map_location=map_location, weights_only=True)
    Restore().keys(state, ("format", "step", "draws", "rng", "extra"), "checkpoint")
    if state["format"] != FORMAT:
        raise ValueError("checkpoint.format: the file has format %r, this package reads %r" % (state["format"], FORMAT))
    draws = list(draws)
    if len(state["draws"]) != len(draws):
        raise ValueError("checkpoint.draws: the file holds %d draw states, %d DeviceDraws were given" % (len(state["draws"]), len(draws)))
    for i, d in enumerate(state["draws"]):
        Restore().keys(d, ("seed", "counter"), "checkpoint.draws[%d]" % i, optional=("views",))
    if restore_rng and state["rng"] is not None:
        _check_rng(state["rng"])
    step.load_state_dict(state["step"])
    for d, s in zip(draws, state["draws"]):
        d.set_state(s)
    if restore_rng and state["rng"] is not None:
        set_rng_state(state["rng"])
    return state["extra"]
