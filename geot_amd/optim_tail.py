"""The tail of a training iteration behind its backward -- gradient clipping, AdamW, and the exponential moving average that
makes a mean teacher follow its student -- as one multi-tensor HIP pass (csrc/optim_tail.hip, include/geot_hip.h "ABI 25").

    tail = OptimTail([optimizer, t_optimizer], clip_params=student.parameters(), max_norm=1.0,
                     teacher=teacher, student=student, ema_decay=0.99)
    loss.backward()
    tail.step()                     # norm sweep, finish, update sweep; tail.total_norm is a device scalar
    optimizer.zero_grad(set_to_none=True)

The reference clips and steps with torch ops (examples/segmentation/train.py:656-660, cfgs/tooth_semi/default.yaml:83) and
names an `ema_decay` (cfgs/tooth_semi/transformer_finetune_fixmatch_ntm.yaml:66) that it never applies: its teacher is loaded,
frozen (train.py:218-222) and left alone.

The torch optimizers stay the owners of the state: step() is another way of executing their step().  exp_avg / exp_avg_sq /
step are created in optimizer.state[p] in the form fused, capturable torch.optim.AdamW creates them (zeros like the parameter,
a 0-dim float32 step on the parameter's device) for the parameters that have a gradient when they first get one, and existing
state is adopted; the only difference is that every `step` is a 0-dim VIEW of one flat float32 tensor, which lets one
workgroup raise all of them.  optimizer.state_dict() therefore loads into a fresh torch.optim.AdamW and continues there, and a
state loaded into the optimizer is adopted by the next step().

composite() runs the same semantics in torch ops -- clip_grad_norm_, optimizer.step(), torch._foreach_lerp_ and a kernel copy
for integer buffers: the second oracle of the tests and the baseline tools/time_optim_tail.py measures against.

accumulate=k > 1 (cfg step_per_update, examples/segmentation/train.py:435, 440, 463, 657-669: the reference updates its
optimizers every step_per_update-th iteration, and every backward in between adds into .grad): step() adds the gradients
into one flat float32 accumulator, in call order, and call k of a window clips, steps and moves the teacher with the
sum -- gated on a counter in device memory (`tail.window`), so that every call issues the same launches and one captured
graph serves every call of a window.  The gradients are still dropped after every call.  total_norm / clip_coef are written
by update calls only: between two updates they hold the norm of the last window's sum.  A window that an epoch cuts off is
not lost: restart() returns the counter to 0 and keeps the sum, which joins the next window, as the reference's num_iter = 0
(train.py:435) against its zero_grad() (train.py:664) has it.  `tail.window` and `tail.accumulator` are public: a checkpoint
in the middle of a window saves both and hands them back with accumulator.copy_() and restart(window=n) -- which is what
state_dict() / load_state_dict() below do, in place and checked first (geot_amd/checkpoint.py).  Which parameters
an open window holds is followed on the host, by the eager calls (a replayed graph has its set fixed); a caller that changes the
set of parameters with gradients between a replay and an eager call of one window starts that window with restart(drop=True).

There is no fallback: a missing library or kernel raises.
"""
import numpy as np
import torch

from . import _lib
from .ext._common import call, need

CAP = _lib.OPTIM_TAIL_CAP
BLOCK_ELEMS = _lib.OPTIM_TAIL_BLOCK_ELEMS
MAX_GROUPS = _lib.OPTIM_TAIL_MAX_GROUPS
CLIPPED, VECTOR = _lib.OPTIM_TAIL_CLIPPED, _lib.OPTIM_TAIL_VECTOR
EMA_ONLY, INT64 = _lib.OPTIM_TAIL_EMA_ONLY, _lib.OPTIM_TAIL_INT64

# the host records of include/geot_hip.h (GEOT_OPTIM_TAIL_REC_WORDS / GEOT_OPTIM_TAIL_GROUP_WORDS 32-bit words)
RECORD = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("t", "<u8"), ("n", "<i8"),
                   ("first_block", "<i4"), ("group", "<i4"), ("flags", "<i4"), ("step", "<i4")])
GROUP = np.dtype([("beta1", "<f8"), ("beta2", "<f8"), ("eps", "<f4"), ("weight_decay", "<f4"), ("lr", "<f4"),
                  ("pad", "<i4"), ("lr_ptr", "<u8")])
assert RECORD.itemsize == 4 * _lib.OPTIM_TAIL_REC_WORDS
assert GROUP.itemsize == 4 * _lib.OPTIM_TAIL_GROUP_WORDS


def plan(counts, aligned, flags):
    """geot_optim_tail_plan: -> dict update_launches, norm_launches, update_blocks, slots, blocks (T,), vector (T,)."""
    t = len(counts)
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    aligned = np.ascontiguousarray(aligned, dtype=np.int32)
    flags = np.ascontiguousarray(flags, dtype=np.int32)
    need(len(aligned) == t and len(flags) == t, "optim_tail.plan: counts, aligned and flags must have one entry per record")
    out = np.zeros(4 + 2 * t, dtype=np.int64)
    ok = _lib.load().geot_optim_tail_plan(t, counts.ctypes.data, aligned.ctypes.data, flags.ctypes.data, out.ctypes.data, len(out))
    need(ok == 1, "geot_optim_tail_plan refused the records (a negative count)")
    return {"update_launches": int(out[0]), "norm_launches": int(out[1]), "update_blocks": int(out[2]), "slots": int(out[3]),
            "blocks": out[4:4 + t].copy(), "vector": out[4 + t:].copy()}


def acc_plan(counts, aligned, flags):
    """geot_optim_tail_acc_plan: -> dict acc_launches, finish_launches, update_launches, acc_blocks, update_blocks, slots."""
    t = len(counts)
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    aligned = np.ascontiguousarray(aligned, dtype=np.int32)
    flags = np.ascontiguousarray(flags, dtype=np.int32)
    need(len(aligned) == t and len(flags) == t, "optim_tail.acc_plan: counts, aligned and flags must have one entry per record")
    out = np.zeros(6, dtype=np.int64)
    ok = _lib.load().geot_optim_tail_acc_plan(t, counts.ctypes.data, aligned.ctypes.data, flags.ctypes.data, out.ctypes.data, len(out))
    need(ok == 1, "geot_optim_tail_acc_plan refused the records (a negative count)")
    return dict(zip(("acc_launches", "finish_launches", "update_launches", "acc_blocks", "update_blocks", "slots"),
                    (int(v) for v in out)))


def check_accumulate(k, what="accumulate"):
    """step_per_update: an int >= 1 (a bool is none)."""
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError("%s must be an int, got %r" % (what, k))
    if k < 1:
        raise ValueError("%s must be at least 1, got %r" % (what, k))
    return k


def _unwrapped(module):
    return module.module if hasattr(module, "module") else module


def teacher_pairs(student, teacher):
    """The (student tensor, teacher tensor, name) of every state_dict() entry of the unwrapped modules, paired by name.
    A mismatch of names, shapes or dtypes, or a dtype that is neither float32 nor int64, is a RuntimeError."""
    s_sd, t_sd = _unwrapped(student).state_dict(keep_vars=True), _unwrapped(teacher).state_dict(keep_vars=True)
    if list(s_sd) != list(t_sd):
        odd = sorted(set(s_sd) ^ set(t_sd))
        raise RuntimeError("OptimTail: student and teacher do not hold the same entries (%s)" % (", ".join(odd[:6]) or "order differs"))
    pairs = []
    for name, s in s_sd.items():
        t = t_sd[name]
        if s.shape != t.shape or s.dtype != t.dtype or s.device != t.device:
            raise RuntimeError("OptimTail: %s is %s %s on %s in the student, %s %s on %s in the teacher"
                               % (name, tuple(s.shape), s.dtype, s.device, tuple(t.shape), t.dtype, t.device))
        if s.dtype not in (torch.float32, torch.int64):
            raise RuntimeError("OptimTail: %s is %s; the EMA takes float32 entries and copies int64 ones" % (name, s.dtype))
        if not (s.is_contiguous() and t.is_contiguous()):
            raise RuntimeError("OptimTail: %s is not contiguous" % name)
        if s.data_ptr() == t.data_ptr() and s.numel():
            raise RuntimeError("OptimTail: %s is the same tensor in student and teacher" % name)
        pairs.append((s, t, name))
    return pairs


class OptimTail:
    def __init__(self, optimizers, clip_params=None, max_norm=None, teacher=None, student=None, ema_decay=None, accumulate=1):
        """optimizers: torch.optim.AdamW objects, stepped in order, at most 4 parameter groups together (amsgrad / maximize
        groups are refused).  clip_params + max_norm: the parameters whose gradients clip_grad_norm_ would see, and its
        max_norm; max_norm None: no clipping, no norm sweep.  teacher + student + ema_decay: the teacher's state_dict() entries
        follow the student's -- float32 entries (parameters, BatchNorm running statistics) by t = d t + (1 - d) s with the
        constant d = ema_decay, int64 entries (num_batches_tracked) by copy.  accumulate = k: every k-th step() updates, with
        the sum of the gradients of the k calls (module docstring); 1: every call, nothing is allocated for it."""
        self.accumulate = check_accumulate(accumulate, "OptimTail: accumulate")
        self.optimizers = list(optimizers)
        need(self.optimizers, "OptimTail: no optimizer")
        self.groups = []                      # (optimizer, its group dict)
        for opt in self.optimizers:
            if not isinstance(opt, torch.optim.AdamW):
                raise RuntimeError("OptimTail: %s is not a torch.optim.AdamW" % type(opt).__name__)
            for group in opt.param_groups:
                if group.get("amsgrad") or group.get("maximize"):
                    raise RuntimeError("OptimTail: amsgrad / maximize are not supported")
                self.groups.append((opt, group))
        if len(self.groups) > MAX_GROUPS:
            raise RuntimeError("OptimTail: %d parameter groups, the kernels take %d" % (len(self.groups), MAX_GROUPS))
        self.params = []                      # (parameter, optimizer, group index), in stepping order
        for gi, (opt, group) in enumerate(self.groups):
            for p in group["params"]:
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                    raise RuntimeError("OptimTail: parameters must be contiguous float32 tensors on the GPU")
                self.params.append((p, opt, gi))
        need(self.params, "OptimTail: the optimizers hold no parameter")
        self.device = self.params[0][0].device
        need(all(p.device == self.device for p, _, _ in self.params), "OptimTail: all parameters must live on one device")
        if len({id(p) for p, _, _ in self.params}) != len(self.params):
            raise RuntimeError("OptimTail: a parameter appears in two groups")
        self.max_norm = None if max_norm is None else float(max_norm)
        self.clip_params = list(clip_params) if clip_params is not None else []
        if self.max_norm is not None and not self.clip_params:
            raise RuntimeError("OptimTail: max_norm without clip_params")
        clipped = {id(p) for p in self.clip_params} if self.max_norm is not None else set()
        self._clipped = [id(p) in clipped for p, _, _ in self.params]
        owned = {id(p) for p, _, _ in self.params}
        if any(p.requires_grad and id(p) not in owned for p in self.clip_params):
            raise RuntimeError("OptimTail: a clipped parameter that takes a gradient belongs to none of the optimizers")
        self.pairs = []
        self.ema_decay = None
        if teacher is not None or student is not None or ema_decay is not None:
            if teacher is None or student is None or ema_decay is None:
                raise RuntimeError("OptimTail: teacher, student and ema_decay go together")
            if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)) or not 0.0 <= float(ema_decay) < 1.0:
                raise RuntimeError("OptimTail: 0 <= ema_decay < 1, got %r" % (ema_decay,))
            self.ema_decay = float(ema_decay)
            self.pairs = teacher_pairs(student, teacher)
            need(all(s.device == self.device for s, _, _ in self.pairs), "OptimTail: the teacher must live on the parameters' device")
        self._teacher_of = {id(s): t for s, t, _ in self.pairs}
        self.steps = torch.zeros(len(self.params), dtype=torch.float32, device=self.device)      # every step counter
        self._step_views = [None] * len(self.params)
        self._bound = None                    # the active set whose state is known to be bound
        self._states = [None] * len(self.optimizers)       # the optimizers' state dicts the views were bound into
        self.scalars = torch.zeros(2, dtype=torch.float32, device=self.device)
        self.scalars[1] = 1.0
        self.total_norm = self.scalars[0]     # device scalars, rewritten by every step()
        self.clip_coef = self.scalars[1]
        self._active = None                   # indices into self.params of the cached table
        self._table = None
        self._slots = None
        self._plan = None
        self._group_table = np.zeros(len(self.groups), dtype=GROUP)
        self.launches = 0                     # kernel launches of the last step()
        self.accumulator = self.window = None
        self._kept = {}                       # composite(): parameter index -> the gradient summed so far
        self._calls = self._composite_calls = 0       # the host's view of the window (which records an update holds)
        self._pending = set()                 # parameter indices with a gradient in the open window
        if self.accumulate > 1:
            offsets, at = [], 0
            for p, _, _ in self.params:       # every stretch starts on 16 bytes: the dwordx4 path
                offsets.append(at)
                at += -(-p.numel() // 4) * 4
            self.accumulator = torch.zeros(max(at, 4), dtype=torch.float32, device=self.device)
            self._acc_offsets = torch.tensor(offsets, dtype=torch.int64, device=self.device)       # written once, here
            self._gate = torch.zeros(2, dtype=torch.int32, device=self.device)
            self.window = self._gate[0]       # calls of the open window, a device int

    # ---- state ------------------------------------------------------------------------------------------------------------
    def _bind_state(self, active):
        """exp_avg / exp_avg_sq / step of the active parameters: created as torch.optim.AdamW would, or adopted; every step
        a view of self.steps.  Creating or adopting issues fills and copies: not under graph capture."""
        rebound = [opt.state is not self._states[k] for k, opt in enumerate(self.optimizers)]
        if not any(rebound) and self._bound == tuple(active):
            return False
        todo = []
        for i in active:
            p, opt, _ = self.params[i]
            k = self.optimizers.index(opt)
            st = opt.state.get(p)
            if st is None or "step" not in st or "exp_avg" not in st or rebound[k] or st["step"] is not self._step_views[i]:
                todo.append(i)
        self._bound = tuple(active)
        if not todo:
            return False
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("OptimTail: optimizer state has to be created or adopted under graph capture -- run the step "
                               "eagerly once before capturing it")
        for i in todo:
            p, opt, _ = self.params[i]
            st = opt.state[p]
            view = self.steps[i]
            if "step" in st and "exp_avg" in st and "exp_avg_sq" in st:
                old = st["step"]
                if torch.is_tensor(old):
                    if old.data_ptr() != view.data_ptr():
                        view.copy_(old.to(device=self.device, dtype=torch.float32))
                else:
                    view.fill_(float(old))
                for key in ("exp_avg", "exp_avg_sq"):
                    t = st[key]
                    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == p.shape):
                        raise RuntimeError("OptimTail: the optimizer's %s is not a contiguous float32 tensor like its parameter" % key)
            else:
                view.zero_()
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] = view
            self._step_views[i] = view
        self._states = [opt.state for opt in self.optimizers]
        return True

    def create_state(self, indices):
        """The state of these parameters (indices into self.params), as the first step() that finds their gradients creates
        it: what a load fills in a fresh tail (geot_amd/checkpoint.py)."""
        self._bind_state(sorted(set(indices) | set(self._bound or ())))

    def state_dict(self):
        """What the tail keeps beside the optimizers' state (which the optimizers' entries of a step's state hold, step
        counters included): total_norm / clip_coef, and under accumulate > 1 the open window -- the accumulator, the device
        counter `window` and the host's view of it (_calls, _pending).  Copies on the current stream, no synchronisation."""
        from . import checkpoint as ck
        ck.refuse_capture("OptimTail")
        if self._kept:
            raise RuntimeError("OptimTail.state_dict: composite() holds the gradients of an open window (the oracle's own "
                               "form of accumulate > 1, which no step runs: not saved)")
        out = {"accumulate": self.accumulate, "total_norm": ck.copied(self.total_norm), "clip_coef": ck.copied(self.clip_coef)}
        if self.accumulate > 1:
            out.update(accumulator=ck.copied(self.accumulator), window=ck.copied(self.window), _calls=self._calls,
                       _pending=sorted(self._pending))
        return out

    def restore(self, r, state, key="tail"):
        """The first half of load_state_dict: check `state` and hand the writes to r (a checkpoint.Restore)."""
        windowed = ("accumulator", "window", "_calls", "_pending") if self.accumulate > 1 else ()
        r.keys(state, ("accumulate", "total_norm", "clip_coef") + windowed, key)
        if state["accumulate"] != self.accumulate:
            raise ValueError("%s.accumulate: the state was saved with %r, the tail is built with %r"
                             % (key, state["accumulate"], self.accumulate))
        r.tensor(key + ".total_norm", self.total_norm, state["total_norm"])
        r.tensor(key + ".clip_coef", self.clip_coef, state["clip_coef"])
        if not windowed:
            return
        r.tensor(key + ".accumulator", self.accumulator, state["accumulator"])
        r.tensor(key + ".window", self.window, state["window"])
        # The host's view of the window is followed by eager calls only: a state taken behind replays carries the view of the
        # last call that ran in python.  The device counter is the truth, and a load may read it (a state on the device: one
        # synchronisation): the host resumes from it.  _pending stays the saved set -- with a fixed set of parameters, the one
        # case a replay serves, it is the set of every call.
        pending = state["_pending"]
        calls = int(state["window"])
        for name, v in (("_calls", r.number(key + "._calls", state["_calls"], int)), ("window", calls)):
            if not 0 <= v < self.accumulate:
                raise ValueError("%s.%s: %r is no call of a window of %d" % (key, name, v, self.accumulate))
        if not isinstance(pending, list) or any(isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < len(self.params)
                                                for i in pending):
            raise ValueError("%s._pending: expected a list of parameter indices below %d, got %r" % (key, len(self.params), pending))

        def host():
            self._calls, self._pending = calls, set(pending)
            self._composite_calls, self._kept = calls, {}          # (as restart(window=calls) leaves the oracle's count)
        r.then(host)

    def load_state_dict(self, state):
        """state_dict()'s counterpart: checked first (ValueError naming the key), then copied into the tensors that exist --
        a captured graph holds the accumulator, the counter and the scalars."""
        from . import checkpoint as ck
        r = ck.Restore()
        self.restore(r, state)
        r.commit()

    # ---- the table ----------------------------------------------------------------------------------------------------------
    def _build(self, active, grads):
        """The record table for these active parameters (pointers of p, m, v, t cached; g filled per call)."""
        recs = []
        has_grad = set()
        for i in active:
            p, opt, gi = self.params[i]
            st = opt.state[p]
            t = self._teacher_of.get(id(p))
            recs.append((p.data_ptr(), 0, st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                         0 if t is None else t.data_ptr(), p.numel(), 0, gi, CLIPPED if self._clipped[i] else 0, i))
            has_grad.add(id(p))
        for s, t, _ in self.pairs:
            if id(s) in has_grad:
                continue
            recs.append((s.data_ptr(), 0, 0, 0, t.data_ptr(), s.numel(), 0, 0, INT64 if s.dtype == torch.int64 else EMA_ONLY, 0))
        table = np.array(recs, dtype=RECORD)
        self._n_active = len(active)
        self._table, self._active = table, tuple(active)
        self._plan = None

    def _plan_for(self, table):
        aligned = np.ones(len(table), dtype=np.int32)
        for key in ("p", "g", "m", "v", "t"):
            aligned &= (table[key] % 16 == 0)
        return plan(table["n"], aligned, table["flags"])

    def _groups_now(self):
        gt = self._group_table
        for k, (_, group) in enumerate(self.groups):
            lr = group["lr"]
            if torch.is_tensor(lr):
                if not (lr.is_cuda and lr.dtype == torch.float32 and lr.numel() == 1 and lr.device == self.device):
                    raise RuntimeError("OptimTail: a tensor lr must be one float32 on the parameters' device")
                gt[k]["lr"], gt[k]["lr_ptr"] = 0.0, lr.data_ptr()
            else:
                gt[k]["lr"], gt[k]["lr_ptr"] = float(lr), 0
            gt[k]["beta1"], gt[k]["beta2"] = group["betas"]
            gt[k]["eps"], gt[k]["weight_decay"] = group["eps"], group["weight_decay"]
        return gt

    def restart(self, drop=False, window=0):
        """accumulate > 1: the window counter returns to `window` (0) and the sum accumulated so far STAYS -- the reference
        restarts num_iter at every epoch (train.py:435) but zeroes its gradients only behind an update (train.py:664), so a
        window that the end of an epoch cuts off joins the next epoch's first update.  drop=True also clears the sum.
        accumulate == 1: nothing is issued."""
        if self.accumulate == 1:
            return
        window = int(window)
        need(0 <= window < self.accumulate, "OptimTail.restart: 0 <= window < accumulate")
        self.window.fill_(window)
        self._calls = self._composite_calls = window
        if drop:
            self.accumulator.zero_()
            self._pending = set()
            self._kept = {}

    def _grad_ptr(self, g, p):
        if g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape or g.device != self.device or g.is_sparse:
            raise RuntimeError("OptimTail: gradients must be dense contiguous float32 tensors like their parameters")
        return g.data_ptr()

    def _step_window(self, sync=None):
        """step() with accumulate > 1: accumulate sweep, gated finish, gated update sweep -- the same launches every call."""
        k = self.accumulate
        capturing = torch.cuda.is_current_stream_capturing()
        grads = {i: p.grad for i, (p, _, _) in enumerate(self.params) if p.grad is not None}
        union = sorted(set(grads) | self._pending)
        if capturing and union != sorted(grads):
            raise RuntimeError("OptimTail: a captured call fixes the parameters of its window's update, and the open window "
                               "holds the gradient of one that has none in this call -- capture behind an update, or restart(drop=True)")
        rebuilt = self._bind_state(union)
        if rebuilt or self._active != tuple(union):
            self._build(union, None)
        table = self._table
        table["g"][:len(union)] = [self._grad_ptr(grads[i], self.params[i][0]) if i in grads else 0 for i in union]
        aligned = np.ones(len(table), dtype=np.int32)
        for key in ("p", "g", "m", "v", "t"):
            aligned &= (table[key] % 16 == 0)
        pl = acc_plan(table["n"], aligned, table["flags"])
        clip = self.max_norm is not None
        if clip and (self._slots is None or self._slots.numel() < max(pl["slots"], 1)):
            self._slots = torch.empty(max(pl["slots"], 1), dtype=torch.float32, device=self.device)
        dev, t, host = self.device, len(table), table.ctypes.data
        acc, offs, gate = self.accumulator, self._acc_offsets, self._gate

        def accumulate():
            call("geot_optim_tail_accumulate", dev, t, host, acc.data_ptr(), offs.data_ptr(), acc.numel(), offs.numel(),
                 self._slots.data_ptr() if clip else None, self._slots.numel() if clip else 0)
        accumulate()
        sweeps = 1
        update_call = self._calls + 1 >= k
        if sync is not None and update_call:
            if capturing:
                raise NotImplementedError("OptimTail: the gradient exchange of an accumulated window cannot be gated inside a graph")
            sync.exchange(acc)
            if clip:                          # the norm of the exchanged sum: the same sweep with nothing to add
                table["g"][:len(union)] = 0
                accumulate()
                sweeps = 2
        call("geot_optim_tail_acc_finish", dev, t, host, int(clip), pl["slots"] if clip else 0,
             self._slots.data_ptr() if clip else None, self.max_norm if clip else 0.0, self.steps.data_ptr(),
             self.steps.numel(), self.scalars.data_ptr(), gate.data_ptr(), k)
        groups = self._groups_now()
        call("geot_optim_tail_acc_update", dev, t, host, len(groups), groups.ctypes.data, self.scalars.data_ptr(),
             self.steps.data_ptr(), self.steps.numel(), self.ema_decay if self.ema_decay is not None else 0.0,
             acc.data_ptr(), offs.data_ptr(), acc.numel(), gate.data_ptr())
        self._calls = 0 if update_call else self._calls + 1
        self._pending = set() if update_call else set(union)
        self.launches = sweeps * pl["acc_launches"] + pl["finish_launches"] + pl["update_launches"]
        self.last_plan = pl
        return self.total_norm

    def step(self, sync=None):
        """clip + AdamW + EMA on the current stream.  The gradients are read, not scaled in place: drop them afterwards.
        accumulate > 1: the gradients join the window's sum, and call k of the window updates with it; total_norm is the norm
        of the sum of the last COMPLETED window (update calls write it, the calls in between leave it).  The records of an
        update are those of every parameter that had a gradient in any call of its window.  sync: an object whose
        exchange(flat tensor) averages the accumulator over the ranks (train_step.GradSync), called on update calls only."""
        if self.accumulate > 1:
            return self._step_window(sync)
        active, grads = [], []
        for i, (p, _, _) in enumerate(self.params):
            g = p.grad
            if g is not None:
                active.append(i)
                grads.append(g)
        rebuilt = self._bind_state(active)
        if rebuilt or self._active != tuple(active):
            self._build(active, grads)
        table = self._table
        ptrs = []
        for g, i in zip(grads, active):
            p = self.params[i][0]
            if g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape or g.device != self.device or g.is_sparse:
                raise RuntimeError("OptimTail: gradients must be dense contiguous float32 tensors like their parameters")
            ptrs.append(g.data_ptr())
        table["g"][:len(ptrs)] = ptrs
        pl = self._plan_for(table)
        clip = self.max_norm is not None
        if clip and (self._slots is None or self._slots.numel() < max(pl["slots"], 1)):
            self._slots = torch.empty(max(pl["slots"], 1), dtype=torch.float32, device=self.device)
        dev, t, host = self.device, len(table), table.ctypes.data
        if clip:
            call("geot_optim_tail_norm", dev, t, host, self._slots.data_ptr(), self._slots.numel())
        call("geot_optim_tail_finish", dev, t, host, int(clip), pl["slots"] if clip else 0,
             self._slots.data_ptr() if clip else None, self.max_norm if clip else 0.0, self.steps.data_ptr(),
             self.steps.numel(), self.scalars.data_ptr())
        groups = self._groups_now()
        call("geot_optim_tail_update", dev, t, host, len(groups), groups.ctypes.data, self.scalars.data_ptr(),
             self.steps.data_ptr(), self.steps.numel(), self.ema_decay if self.ema_decay is not None else 0.0)
        n_adamw = self._n_active
        steps_cap = _lib.OPTIM_TAIL_STEP_CAP
        self.launches = (pl["norm_launches"] if clip else 0) + max(1, -(-n_adamw // steps_cap)) + pl["update_launches"]
        self.last_plan = pl
        return self.total_norm

    # ---- the same semantics in torch ops ----------------------------------------------------------------------------------------
    def composite(self):
        """clip_grad_norm_ + optimizer.step() + torch._foreach_lerp_ (+ a kernel copy for integer buffers) -> total_norm
        (None without a clip).  The optimizers keep whatever state they have (a state the fused step bound stays bound).
        accumulate > 1: the gradients are added in place into kept ones (torch._foreach_add_); call k of a window hands
        the sums back as .grad and runs the above, the calls before it return None and leave every state alone."""
        total = None
        if self.accumulate > 1:
            with torch.no_grad():
                have = [(i, p.grad) for i, (p, _, _) in enumerate(self.params) if p.grad is not None]
                for i, g in have:
                    if i not in self._kept:
                        self._kept[i] = torch.zeros_like(g)
                if have:
                    torch._foreach_add_([self._kept[i] for i, _ in have], [g for _, g in have])
            self._composite_calls += 1
            if self._composite_calls < self.accumulate:
                return None
            self._composite_calls = 0
            for i, (p, _, _) in enumerate(self.params):
                p.grad = self._kept.get(i)
            self._kept = {}
        if self.max_norm is not None:
            total = torch.nn.utils.clip_grad_norm_(self.clip_params, self.max_norm)
        for opt in self.optimizers:
            opt.step()
        if self.pairs:
            with torch.no_grad():
                fs = [s.detach() for s, t, _ in self.pairs if s.dtype == torch.float32]
                ft = [t.detach() for s, t, _ in self.pairs if s.dtype == torch.float32]
                if ft:
                    torch._foreach_lerp_(ft, fs, 1.0 - self.ema_decay)
                for s, t, _ in self.pairs:
                    if s.dtype == torch.int64:
                        torch.add(s.detach(), 0, out=t.detach())       # (a kernel: copy_ would be a memcpy node under capture)
        return total
