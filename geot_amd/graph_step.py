"""The training steps of train_step.py replayed from hipGraphs: per iteration the host issues a handful of small copies and
TWO graph launches instead of ~1100 (supervised) / ~1500 (FixMatch+NTM) kernel launches with their autograd bookkeeping
(18-24 ms of host time per iteration -- at one or two clouds per step, the whole step).

    step    = SupervisedStep(model)                      # or build_fixmatch(...)
    graphed = GraphedSupervisedStep(step)                # or GraphedFixMatchStep(step)
    loss    = graphed(pos, cls, target, next_pos=...)    # same call, same results, bit for bit

An iteration is two SINGLE-STREAM graphs (geot_amd/streams.py: on ROCm 7.0 a graph with fork / join branches costs the host
6-17 ms per launch, a single-stream one of the same kernels 0.3 ms):

* **P** -- the step's `lookahead_work()`: everything that depends on a batch and on frozen state alone.  Supervised step:
  the batch's geometry (Group, the 8192-sample FPS, the index plan).  FixMatch+NTM: the student's and the teacher's
  geometry, the frozen teacher's forward -> pseudo labels, the kNN graph and Morton order of the 3-D loss; after the
  step's switch_ep (FixMatchNTMStep.set_epoch) the student's geometry and the kNN graph / order only -- each phase has a
  P and an M of its own ("P" / "M" and "P@2" / "M@2"), captured on first use, and a look-ahead made under one phase is
  never handed to the other's M (P then runs in line, same results).  With cfg ema_teacher the teacher moves with every
  update, so its forward cannot run beside the update before it: before switch_ep that step has a third phase ("P@e" /
  "M@e") whose P holds the student's and the teacher's geometry, the kNN graph / order and the refine table -- no pseudo
  labels, no teacher feature -- and whose M starts with the teacher's forward and ends with the tail that moves it; after
  switch_ep the teacher no longer runs and "P@2" / "M@2" are what they were, M@2 with the tail at its end.  The step says
  which phase it is in and which batch keys its look-ahead reads there; its product (train_step.BatchWork) is only handed on.
* **M** -- the training iteration proper over P's product: forward, losses, backward, AdamW (capturable=True; under
  fused=True the step counters live on the device either way: the same kernel), the EMA transition matrix updated in
  its buffer.

With `next_pos` / `next_batches` given, P of the NEXT batch replays on a side stream beside M of the current one -- the
overlap the eager steps build from side streams inside the iteration, here between two graphs; its product is copied into
M's input buffers at the head of the next call, behind M.  Whether that product describes the batch a call passes is
checked on the host (the very tensors the previous call announced, unedited); otherwise -- the first call, a reshuffled
loader, no look-ahead at all -- P runs for the current batch on the current stream before M.

A learning-rate schedule reaches a captured AdamW step through memory: make `lr` a float32 device tensor in the optimizer's
parameter groups and fill_ it between calls (tests/test_graph_step_gpu.py; geot_amd/schedule.py LrSchedule does both for the
configured schedule, and fit.py installs it before the first call); a python float is baked into the graph.
Inputs are copied into static buffers before every replay; shapes are fixed by the first call (another shape is an error:
build another wrapper).  The first `warmup` executions of each graph's body run eagerly over the same buffers, the next
one captures.  N > 1: DistributedDataParallel itself is not captured (its reducer is host logic); a step built on the bare
SyncBatchNorm-converted modules with a gradient exchange of its own (train_step.sync_only / GradSync: one flat RCCL
all-reduce between backward and optimizer, a kernel node) replays like the single-GPU one -- SyncBatchNorm's statistic
all-reduces and the anchor all-gather of the class transition are captured where they stand.

cfg step_per_update = k > 1 (train.py:435, 440, 463, 657-669) with the fused tail replays the graphs of k = 1: the tail gates its
update on a counter in device memory, every call issues the same launches, and the warm-up calls are calls of the window like
the replays.  Without fused_tail the schedule is host logic and the wrappers refuse the step; with a GradSync (N > 1) they
raise NotImplementedError -- the exchange belongs to update calls alone and a captured collective cannot be gated.

Mirrors the loop body of examples/segmentation/train.py:410-669; the reference never leaves eager mode.
"""
import copy
import os

import torch

from . import streams


# ---- structure helpers: P's product is a tree of dicts / tuples (plain and named) of tensors, python scalars and objects
# that say themselves which of their attributes are buffers and which identities (`tree_fields()`: Geometry, ReverseIndex, the FixMatch step's BatchWork) ----
def _rebuilt(obj, items):
    return type(obj)(*items) if hasattr(obj, "_fields") else type(obj)(items)      # (a namedtuple takes its items one by one)


def _tree_map(obj, leaf, keep_identities):
    """The tree rebuilt (containers and tree_fields() objects) with leaf(tensor) for every tensor, everything else as it is."""
    if torch.is_tensor(obj):
        return leaf(obj)
    if isinstance(obj, dict):
        return {k: _tree_map(v, leaf, keep_identities) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return _rebuilt(obj, [_tree_map(v, leaf, keep_identities) for v in obj])
    if hasattr(obj, "tree_fields"):
        buffers, identities = obj.tree_fields()
        new = copy.copy(obj)
        for k in buffers:
            setattr(new, k, _tree_map(getattr(obj, k), leaf, keep_identities))
        for k in () if keep_identities else identities:
            setattr(new, k, None)
        return new
    return obj


def tree_clone(obj):
    """Fresh buffers with the same contents; identities (tensors matched by `is`, events) dropped."""
    return _tree_map(obj, lambda t: t.detach().clone(), False)


def tree_detach(obj):
    """The same buffers without their autograd history."""
    return _tree_map(obj, torch.Tensor.detach, True)


def tree_copy_(dst, src, path="pre"):
    """Copy every tensor of `src` into the matching buffer of `dst`; the structure (and every python scalar) must agree."""
    if torch.is_tensor(dst):
        if not torch.is_tensor(src) or dst.shape != src.shape or dst.dtype != src.dtype:
            raise RuntimeError("%s: the captured buffer does not fit (shape / dtype changed)" % path)
        dst.copy_(src)
    elif isinstance(dst, dict):
        for k, v in dst.items():
            tree_copy_(v, src[k], "%s[%r]" % (path, k))
    elif isinstance(dst, (list, tuple)):
        if not isinstance(src, (list, tuple)) or len(dst) != len(src):
            raise RuntimeError("%s: structure changed" % path)
        for i, (d, s) in enumerate(zip(dst, src)):
            tree_copy_(d, s, "%s[%d]" % (path, i))
    elif hasattr(dst, "tree_fields"):
        if type(src) is not type(dst):
            raise RuntimeError("%s: structure changed" % path)
        buffers, identities = dst.tree_fields()
        for k in vars(dst):
            if k in buffers:
                tree_copy_(getattr(dst, k), getattr(src, k), "%s.%s" % (path, k))
            elif k not in identities and getattr(dst, k) != getattr(src, k):
                raise RuntimeError("%s.%s: %r became %r" % (path, k, getattr(dst, k), getattr(src, k)))
    elif dst is not src and (torch.is_tensor(src) or dst != src):
        raise RuntimeError("%s: %r became %r" % (path, dst, src))


def _fits(dst, src, what):
    if dst.shape != src.shape or dst.dtype != src.dtype:
        raise RuntimeError("graphed step: %s is %s %s, captured for %s %s" % (what, tuple(src.shape), src.dtype,
                                                                              tuple(dst.shape), dst.dtype))


class _Graphed:
    """P / M bookkeeping shared by the two steps; subclasses supply the static buffers and the two bodies."""

    def __init__(self, step, warmup=2, agree=None):
        """agree(ok: bool) -> bool, for N > 1: called after every capture, BEFORE its first replay, with this rank's verdict;
        returns the verdict of all ranks (e.g. an all-reduce MIN).  A capture one rank refuses is then refused by all of
        them at the same point of the collective sequence -- the ranks fall back to the eager step together instead of
        meeting each other with different collectives."""
        self.agree = agree
        # step_per_update = k > 1: the fused tail gates its update on a counter in device memory, so the graphs captured for
        # k = 1 serve every call of a window (the warm-up calls are calls of the window like any other).  The torch form
        # decides "update or not" in python, which a capture would bake in; a captured collective cannot be gated either.
        if getattr(step, "step_per_update", 1) > 1:
            tail = getattr(step, "tail", None)
            if tail is None or tail.accumulate != step.step_per_update:
                raise RuntimeError("graph_step: step_per_update=%d without fused_tail updates on a count kept in python, which "
                                   "a captured graph would fix at one answer -- build the step with fused_tail=True (its tail "
                                   "gates the update on a device counter)" % step.step_per_update)
            if getattr(step, "grad_sync", None) is not None:
                raise NotImplementedError("graph_step: step_per_update=%d with a gradient exchange of the step's own -- the "
                                          "exchange belongs to update calls alone, and a captured collective cannot be "
                                          "gated; run N > 1 with accumulation eagerly" % step.step_per_update)
        for net in (getattr(step, n, None) for n in ("model", "model_t", "T_predictor")):
            if isinstance(net, torch.nn.parallel.DistributedDataParallel):
                raise RuntimeError(
                    "graph_step: a DistributedDataParallel model is not captured -- its reducer is host logic, and it keeps "
                    "every parameter's AccumulateGrad node on the stream of its construction, which forks the captured "
                    "backward (a crash in hipStreamEndCapture on this runtime).  For N > 1 hand the step the bare "
                    "SyncBatchNorm-converted modules and a gradient exchange of its own: train_step.sync_only + GradSync "
                    "(build_fixmatch(graph_sync=True)); over RCCL its one flat all-reduce is a kernel node of the graph")
        if getattr(step, "grad_sync", None) is not None:
            import torch.distributed as dist
            if dist.get_backend(step.grad_sync.group) != "nccl":
                raise RuntimeError("graph_step: the step's gradient exchange runs over the %r backend -- on the host, not "
                                   "capturable; run N > 1 eagerly or over nccl (RCCL)" % dist.get_backend(step.grad_sync.group))
        import geot_amd
        # (see geot_amd/__init__.py) packet capture exported off by the launcher: anything replays; otherwise (fast mode, or the
        # switch set by the package itself, which cannot be verified) only graphs of kernel nodes do -- checked per graph
        self.kernel_only = not geot_amd.graph_replay_is_safe()
        self.step = step
        self.warmup = int(warmup)
        self.calls = 0
        self.device = None
        self.graphs = {}          # "P" / "M" (/ "M1" / "M2"; + "@2" for FixMatch's second phase) -> (CUDAGraph, static outputs)
        self.node_types = {}      # same keys -> {"kernel": n, ...} of the captured graph
        self._eager_runs = {"P": 0, "M": 0}
        self.side = None          # the stream P replays on beside M
        self.pre = None           # P's product in M's input buffers (of the phase that runs now)
        self._pres = {}           # phase tag -> its M's input buffers
        self._pre_next = None     # P's product as P left it (for the batch `_announced` describes)
        self._pre_tag = None      # the phase tag P ran under for _pre_next
        self._announced = None
        self._pending = False     # a P is in flight on the side stream
        for opt in step.optimizers():
            for group in opt.param_groups:
                group["capturable"] = True   # fused AdamW: the step counter is a device tensor already; same kernel
        # a python-float lr is baked into the captured AdamW step: remember it and refuse a call that finds another value
        # (a torch LR scheduler replaces group["lr"] every step -- the replay would silently train at the first one)
        self._float_lrs = [(group, group["lr"]) for opt in step.optimizers() for group in opt.param_groups
                           if not torch.is_tensor(group["lr"])]

    def _check_lr(self):
        for group, lr in self._float_lrs:
            if not torch.is_tensor(group["lr"]) and group["lr"] != lr:
                raise RuntimeError(
                    "graph_step: a parameter group's lr changed from %r to %r, but a python float is baked into the captured "
                    "AdamW step -- the replay would keep training at %r.  Make lr a float32 device tensor in the optimizer's "
                    "parameter groups before wrapping the step and fill_ it between calls (module docstring)" % (lr, group["lr"], lr))

    def _run(self, name, fn, pool_of=None):
        """fn() = a graph's body over the static buffers.  Eager for its first `warmup` executions, then captured once
        (into the memory pool of graph `pool_of`, if given) and replayed on the current stream."""
        if name not in self.graphs:
            if self._eager_runs.get(name, 0) < self.warmup:
                self._eager_runs[name] = self._eager_runs.get(name, 0) + 1
                return fn()
            torch.cuda.synchronize(self.device)
            # Dead python cycles can hold an earlier iteration's autograd graph -- eager steps taken before this wrapper, the
            # warm-up runs -- and with it every parameter's AccumulateGrad node, bound to the stream of THAT iteration; a
            # backward under capture would hop to that stream and back: a fork inside the capture, which this runtime answers
            # with a crash in hipStreamEndCapture (seen at 2 clouds after three eager steps; torch.cuda.graph collected
            # unconditionally until 2.x made it optional).  Collect before every capture: three times in a wrapper's life.
            import gc
            gc.collect()
            graph = torch.cuda.CUDAGraph(keep_graph=True)         # (the hipGraph_t stays: node_types below)
            pool = self.graphs[pool_of][0].pool() if pool_of is not None else None
            refusal = None
            try:
                with streams.capture(graph, self.device, pool=pool):
                    out = fn()
                self.node_types[name] = kinds = streams.node_types(graph)
                if self.kernel_only and set(kinds) - {"kernel"} and os.environ.get("GEOT_GRAPH_UNSAFE") != "1":
                    import geot_amd
                    refusal = RuntimeError(
                        "graph_step: graph %s holds %s; unless the launcher exported %s=0 (before the HIP runtime initialises) "
                        "only kernel nodes are known to replay correctly: with graph packet capture on, eager launches between "
                        "two replays corrupt a graph's memset / memcpy nodes -- wrong gradients, no error "
                        "(geot_amd/__init__.py).  tools/lab/find_nonkernel_ops.py names the operators that issue "
                        "hipMemsetAsync / hipMemcpyAsync" % (name, kinds, geot_amd.GRAPH_PACKET_CAPTURE_ENV))
            except RuntimeError as e:
                if self.agree is None:
                    raise
                refusal = e
            if self.agree is not None and not self.agree(refusal is None) and refusal is None:
                refusal = RuntimeError("graph_step: another rank refused its capture of graph %s; all ranks run eagerly" % name)
            if refusal is not None:
                del graph
                raise refusal
            self.graphs[name] = (graph, out)
        graph, out = self.graphs[name]
        graph.replay()
        return out

    @property
    def captured(self):
        """A P and an M (or M2) of the same phase are captured."""
        tags = {k[k.index("@"):] if "@" in k else "" for k in self.graphs}
        return any(("M" + t in self.graphs or "M2" + t in self.graphs) and "P" + t in self.graphs for t in tags)

    def state_dict(self):
        """The wrapped step's state_dict() (refused under capture, like the step's)."""
        return self.step.state_dict()

    def load_state_dict(self, state):
        """The wrapped step's load_state_dict(): every tensor is restored in place, so the captured graphs go on reading and
        writing the restored memory; nothing is captured anew.  A look-ahead in flight is waited for (it reads what the load
        writes) and, once the state has been accepted, dropped: the next call runs P in line for its batch -- same results."""
        self._join_pending()
        self.step.load_state_dict(state)
        self._pre_next = self._pre_tag = self._announced = None

    def _join_pending(self):
        """The current stream waits for the P of the previous call (its product, and its reads of P's static inputs)."""
        if self._pending:
            torch.cuda.current_stream(self.device).wait_stream(self.side)
            self._pending = False

    def _iterate(self, announced_now, next_src, load_next, lookahead, train, tag=""):
        """announced_now: does the pending look-ahead describe the batch that was just copied in?  next_src: the tensors
        of the announced next batch (None: no look-ahead); load_next(current: bool): fill P's static inputs from the
        current batch / the announced one; lookahead() / train(): the bodies of P / M; tag: the phase, appended to the
        graph names (each phase its own P and M, and its own M input buffers).  (_join_pending() has run.)"""
        dev = self.device
        main = torch.cuda.current_stream(dev)
        if self.side is None:
            self.side = torch.cuda.Stream(device=dev)
        if not (announced_now and self._pre_next is not None and self._pre_tag == tag):
            # nobody looked ahead for this batch (first call, an unannounced batch, no look-ahead, a look-ahead made under
            # the other phase): P now, in line
            load_next(True)
            self._pre_next = self._run("P" + tag, lookahead)
        with torch.no_grad():
            pre = self._pres.get(tag)
            if pre is None:
                self._pres[tag] = pre = tree_clone(self._pre_next)
            else:
                tree_copy_(pre, self._pre_next)
            self.pre = pre
        self._pre_next = self._pre_tag = None
        self._announced = None
        mid = None
        if isinstance(train, tuple):                 # (forward, backward): P starts between the two, beside the backward
            mid = self._run("M1" + tag, train[0])
        if next_src is not None:
            load_next(False)
            self.side.wait_stream(main)              # behind the copies above (and behind M's previous replay)
            with torch.cuda.stream(self.side):
                self._pre_next = self._run("P" + tag, lookahead)
            self._pre_tag = tag
            self._pending = True
            self._announced = tuple((t, t._version) for t in next_src)
        m1, m2 = "M1" + tag, "M2" + tag
        fresh = isinstance(train, tuple) and m2 not in self.graphs
        out = self._run(m2, lambda: train[1](mid), pool_of=m1) if isinstance(train, tuple) else self._run("M" + tag, train)
        if fresh and m2 in self.graphs:
            # M1's stored product (the cut: tensors with the capture-time iteration's autograd graph behind them) has done its
            # job -- M2 is captured and a replay never runs the python backward again.  Kept as it was, it would hold that
            # graph, every parameter's AccumulateGrad node with it (created on the capture stream), for the life of the
            # wrapper, and an eager step afterwards (bench.py's other leg) would find them on the wrong stream.
            g1, o1 = self.graphs[m1]
            self.graphs[m1] = (g1, tree_detach(o1))
        self.calls += 1
        return out

    def _split(self, args):
        """The pair _iterate takes for a split capture: the step's forward_backward_head(*args()) / backward_rest_update.  M1's
        product is what is left of the backward, as data (tree_detach releases it); the step's result waits here for M2."""
        def head():
            self._result, rest = self.step.forward_backward_head(*args())
            return rest

        def rest_update(rest):
            self.step.backward_rest_update(rest)
            return self._result
        return head, rest_update

    def _is_announced(self, tensors):
        a = self._announced
        return a is not None and len(a) == len(tensors) and all(t is s and t._version == v for t, (s, v) in zip(tensors, a))


class GraphedSupervisedStep(_Graphed):
    """SupervisedStep.__call__ from hipGraphs (see the module docstring).  The returned loss is a static tensor the next
    call overwrites: clone it to keep it."""

    def __init__(self, step, warmup=2, split=None, agree=None):
        """split: capture the iteration as two graphs sharing a memory pool -- M1 = forward, loss and the backward of the
        head and the decoder, M2 = the backward of the transformer blocks and the patch encoder + AdamW (the model cuts its
        autograd graph between the two: SupervisedStep.forward_backward_head) -- and start P between them: beside the
        blocks' small GEMMs, where the eager step queues its look-ahead, instead of beside the forward.  Same bits.  It pays
        when what follows the cut outlasts P (~6.3 ms whatever the batch: its FPS runs one cloud per CU): at 8 clouds the
        replay goes from 0.45 ms behind the eager step to level, at 4 clouds 21.95 -> 21.08 ms, at 3 19.37 -> 18.59; at 1 / 2
        clouds M2 is shorter than P and the step waits for it (10.1 -> 12.4, 13.6 -> 15.2 ms).  Default (None):
        GEOT_GRAPH_SPLIT=1 / 0 if set, else split batches of at least 3 clouds.  agree: see _Graphed."""
        super().__init__(step, warmup, agree)
        env = os.environ.get("GEOT_GRAPH_SPLIT")
        self.split = bool(split) if split is not None else (None if env is None else env == "1")
        self.x = None            # static (pos, cls, target[, class_weights])
        self.next_pos = None     # static coordinates P works on

    def __call__(self, pos, cls, target, next_pos=None, class_weights=None):
        weighted = getattr(self.step, "criterion_name", None) == "Weight_CELoss"
        if weighted and class_weights is None:
            raise RuntimeError("graphed step: SupervisedStep(criterion='Weight_CELoss') needs the batch's class_weights")
        batch = (pos, cls, target) + ((class_weights,) if weighted else ())
        names = ("pos", "cls", "target", "class_weights")
        if self.x is None:
            self.device = pos.device
            self.x = (pos.detach().clone().contiguous(),) + tuple(t.detach().clone() for t in batch[1:])
            self.next_pos = torch.empty_like(self.x[0])
            if self.split is None:
                self.split = pos.shape[0] >= 3
        for dst, src, name in zip(self.x, batch, names):
            _fits(dst, src, name)
        if next_pos is not None:
            _fits(self.next_pos, next_pos, "next_pos")
        self._check_lr()
        announced_now = self._is_announced((pos,))
        self._join_pending()
        for dst, src in zip(self.x, batch):
            dst.copy_(src)
        cw = self.x[3] if weighted else None

        def load_next(current):
            self.next_pos.copy_(self.x[0] if current else next_pos)

        def lookahead():
            return self.step.lookahead_work(self.next_pos)

        def train():
            return self.step.iteration(self.x[0], self.x[1], self.x[2], self.pre, None, cw)[0]
        if self.split:
            train = self._split(lambda: (self.x[0], self.x[1], self.x[2], self.pre, cw))
        return self._iterate(announced_now, None if next_pos is None else (next_pos,), load_next, lookahead, train)


class GraphedFixMatchStep(_Graphed):
    """FixMatchNTMStep.__call__ from hipGraphs.  The returned losses are static tensors the next call overwrites.  The phase
    follows the wrapped step's epoch (step.set_epoch, or set_epoch here): a P and an M per phase, each captured on first use.
    With the step's meters on, data_u["y"] is copied into the static buffers like every other key, and the meters' two
    kernels are nodes of M."""

    def __init__(self, step, warmup=2, split=None, agree=None):
        """split: as GraphedSupervisedStep -- M1 ends where the backward reaches the student's transformer blocks, P starts
        there.  Same bits, but a loss here: P is 10 ms (the teacher's forward is in it) and does not fit beside M2 -- 29.0 ->
        30.4 ms per iteration (bench.py --workload fixmatch, alternating).  Off unless split=True / GEOT_GRAPH_SPLIT=1."""
        super().__init__(step, warmup, agree)
        self.split = bool(split) if split is not None else os.environ.get("GEOT_GRAPH_SPLIT") == "1"
        self.data = self.data_u = None       # static batch dicts
        self.next = None                     # static inputs of P

    def __call__(self, data, data_u, next_batches=None):
        step = self.step
        step.check_meter_batch(data_u)
        if self.data is None:
            self.device = data["pos"].device
            self.data = {k: v.detach().clone().contiguous() for k, v in data.items() if torch.is_tensor(v)}
            self.data_u = {k: v.detach().clone().contiguous() for k, v in data_u.items() if torch.is_tensor(v) and k != "T"}
            self.next = tuple({k: torch.empty_like(d[k]) for k in keys}
                              for d, keys in zip((self.data, self.data_u), step.lookahead_keys("")))      # (the widest phase's)
        for dst, src, what in ((self.data, data, "data"), (self.data_u, data_u, "data_u")):
            for k, v in dst.items():
                _fits(v, src[k], "%s[%r]" % (what, k))
        self._check_lr()
        p_keys = step.lookahead_keys()
        announced_now = self._is_announced([b[k] for b, keys in zip((data, data_u), p_keys) for k in keys])
        self._join_pending()
        for dst, src in ((self.data, data), (self.data_u, data_u)):
            for k, v in dst.items():
                v.copy_(src[k])

        def load_next(current):
            srcs = (self.data, self.data_u) if current else next_batches
            for dst, src, keys in zip(self.next, srcs, p_keys):
                for k in keys:
                    _fits(dst[k], src[k], "next[%r]" % k)
                    dst[k].copy_(src[k])

        def lookahead():
            return step.lookahead_work(self.next[0], self.next[1])

        def train():
            return step.student_iteration(self.data, self.data_u, self.pre)
        if self.split:
            train = self._split(lambda: (self.data, self.data_u, self.pre))
        next_src = None if next_batches is None else [b[k] for b, keys in zip(next_batches, p_keys) for k in keys]
        return self._iterate(announced_now, next_src, load_next, lookahead, train, step.phase)

    def set_epoch(self, epoch):
        """The wrapped step's set_epoch."""
        self.step.set_epoch(epoch)
