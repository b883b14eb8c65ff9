"""The eval-mode forward pass replayed from hipGraphs -- what graph_step.py does for the training steps, for the whole-scan
path of validation.py (validate_scans, validate_scans_voted, vote_scans with graph=True):

    fwd = GraphedForward(model)                              # model: WholePartSeg in eval mode, under torch.no_grad()
    geometry = fwd.lookahead([batch["pos"]])                 # the batch's coordinate-only work, on the side stream
    logits, _, _ = fwd(batch, geometry.slice(0, b))          # same call, same bits as model(batch)

A pass is two SINGLE-STREAM graphs of kernel nodes (geot_amd/streams.py: a graph with branches costs the host 6-17 ms per
launch on ROCm 7.0, a single-stream one 0.3 ms), one pair per signature, captured on first use after `warmup` eager runs:

* **P** -- `model.prefetch_geometry(positions, inline=True)`: Group, the largest downsample_targets FPS and the index plan of
  one or SEVERAL passes' positions concatenated along the batch axis (FPS costs the same per launch whether it holds 2 clouds
  or 20).  Keyed by the shape of the concatenated positions.
* **F** -- `model(data, geometry=<one pass's slice of P's product>)`.  Keyed by the keys, shapes, dtypes and device of the
  tensors in `data` and the geometry's python scalars.

`fwd(data, geometry, next_positions=[...])` copies the pass's inputs and its geometry into F's fixed buffers
(graph_step.tree_copy_), THEN starts P for the announced positions on the side stream, then replays F: the look-ahead runs
beside the forward pass, as GraphedSupervisedStep's P runs beside its M; its product (`fwd.ahead`) stays in P's own buffers
until the next P of the same shape, and the next call's copy is queued before that.  No graph has parallel branches.

What a caller has to know:

* The returned logits are a VIEW OF A FIXED BUFFER: the next call with the same signature overwrites it.  Use it (or clone
  it) before the next call; validation._passes' consumers do.
* The geometry is static (Geometry.static): a replay has no tensor identities to check, so the CALLER vouches that the slice
  it hands over was computed from this batch's positions (validation._passes checks object and version on the host).
* Parameters and buffers are read in place: a training step, an EMA update or a load_state_dict between two validations is
  seen by the next replay.  If the address, shape or dtype of one changed (a new tensor was assigned), the F graphs are
  dropped and captured again.
* A captured graph that holds anything but kernel nodes is refused (with packet capture on, memset / memcpy nodes replay
  wrongly: geot_amd/__init__.py): that signature then runs eagerly -- same results -- and the refusal is remembered in
  `refused`, not retried.  A pass without a static geometry (a group's short last batch, a model that has no
  prefetch_geometry product) runs eagerly too.
* Training mode and enabled grad raise RuntimeError before anything is captured: a replay would neither update BatchNorm
  statistics nor record an autograd graph.
"""
import weakref

import numpy as np
import torch

from . import streams
from .graph_step import tree_clone, tree_copy_

MAX_LOOKAHEAD = 64      # passes drawn ahead (validation.py's `lookahead`): batches and one concatenated geometry stay resident


def tree_tensors(obj, path=""):
    """(path, tensor) for every tensor in a tree of dicts, lists, tuples (plain and named) and tree_fields() objects
    (Geometry): the buffers, not the identities."""
    if torch.is_tensor(obj):
        yield path, obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            yield from tree_tensors(v, "%s[%r]" % (path, k))
    elif isinstance(obj, (list, tuple)):
        names = getattr(obj, "_fields", None)
        for i, v in enumerate(obj):
            yield from tree_tensors(v, "%s.%s" % (path, names[i]) if names else "%s[%d]" % (path, i))
    elif hasattr(obj, "tree_fields"):
        for k in obj.tree_fields()[0]:
            yield from tree_tensors(getattr(obj, k), "%s.%s" % (path, k))


def _census(graph):
    """The node kinds of a captured graph (streams.node_types); the one place the capture check reads them."""
    return streams.node_types(graph)


def _int(value, what, lo, hi):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise TypeError("%s must be an int, got %r" % (what, value))
    if not lo <= int(value) <= hi:
        raise ValueError("%s must lie in %d..%d, got %r" % (what, lo, hi, value))
    return int(value)


class GraphedForward:
    """model(data, geometry=...) of an eval-mode model from hipGraphs (module text).  graphs / node_types: name -> the
    captured graph and its static outputs / its node kinds, name = ("F", signature) or ("P", positions shape); refused:
    name -> why that signature runs eagerly; replays: graph launches so far; ahead: the product of the last look-ahead."""

    def __init__(self, model, warmup=2):
        self.warmup = _int(warmup, "GraphedForward: warmup", 0, 1 << 20)
        self.model = model
        self.graphs, self.node_types, self.refused = {}, {}, {}
        self.inputs = {}          # F name -> (static data dict, static Geometry); P name -> static positions
        self.replays = 0
        self.ahead = None
        self.device = None
        self.side = None          # the stream P runs on beside F
        self._runs = {}           # name -> eager executions so far
        self._pending = False     # a P is in flight on the side stream
        self._params = None       # (address, shape, dtype) of every parameter and buffer the F graphs were captured over

    # ---- host-side keys --------------------------------------------------------------------------------------------------
    @staticmethod
    def signature(data, geometry=None):
        """The key of F's graph for this call: the keys, shapes, dtypes and devices of the tensors in `data`, and the
        geometry's python scalars.  Two batches of equal shapes share a key; another N, B or key set is another graph."""
        tensors = tuple(sorted((str(k), tuple(v.shape), str(v.dtype), str(v.device)) for k, v in data.items() if torch.is_tensor(v)))
        scalars = None
        if geometry is not None:
            buffers, identities = geometry.tree_fields()
            scalars = tuple(sorted((k, v) for k, v in vars(geometry).items() if k not in buffers and k not in identities))
        return tensors, scalars

    def _fingerprint(self):
        return tuple((t.data_ptr(), tuple(t.shape), t.dtype) for group in (self.model.parameters(), self.model.buffers()) for t in group)

    def _refuse_modes(self):
        if self.model.training:
            raise RuntimeError("GraphedForward: the model is in training mode -- a replay would not update its BatchNorm "
                               "statistics and repeats one dropout mask; call model.eval() first")
        if torch.is_grad_enabled():
            raise RuntimeError("GraphedForward: grad is enabled -- a replay records no autograd graph; call under torch.no_grad()")

    # ---- capture and replay ----------------------------------------------------------------------------------------------
    def _run(self, name, fn):
        """fn() = a graph's body over its fixed buffers: eager for its first `warmup` executions, then captured once and
        replayed on the current stream.  A capture that holds anything but kernel nodes is refused for good: fn() runs
        eagerly (a capture executes nothing, so this call's results come from that run too)."""
        if name in self.refused:
            return fn()
        if name not in self.graphs:
            if self._runs.get(name, 0) < self.warmup:
                self._runs[name] = self._runs.get(name, 0) + 1
                return fn()
            torch.cuda.synchronize(self.device)
            graph = torch.cuda.CUDAGraph(keep_graph=True)         # (the hipGraph_t stays: the node census)
            with streams.capture(graph, self.device):
                out = fn()
            kinds = _census(graph)
            if set(kinds) - {"kernel"}:
                self.refused[name] = ("GraphedForward: graph %s holds %s; only kernel nodes are known to replay correctly "
                                      "(geot_amd/__init__.py) -- this signature runs eagerly" % (name[0], kinds))
                del graph, out
                return fn()
            self.graphs[name], self.node_types[name] = (graph, out), kinds
        graph, out = self.graphs[name]
        graph.replay()
        self.replays += 1
        return out

    def join(self):
        """The current stream waits for the P in flight: its product, and its reads of P's fixed positions."""
        if self._pending:
            torch.cuda.current_stream(self.device).wait_stream(self.side)
            self._pending = False

    def _check_params(self):
        now = self._fingerprint()
        if now != self._params:
            if self._params is not None and any(n[0] == "F" for n in self.graphs):
                torch.cuda.synchronize(self.device)               # a replay may still be reading the old tensors
                for n in [n for n in self.graphs if n[0] == "F"]:
                    del self.graphs[n], self.node_types[n]
            self._params = now

    def lookahead(self, positions):
        """P for the passes whose (b, N, 3) positions are listed, concatenated along the batch axis, on the side stream behind
        everything queued on the current one -> a static Geometry of all their clouds (pass k's is .slice(k b, (k + 1) b)),
        or None when the model has none to give.  The product lives in P's buffers: the next look-ahead of the same shape
        overwrites it.  The current stream waits for it at the head of the next call."""
        self._refuse_modes()
        positions = list(positions)
        first = positions[0]
        if not (first.is_cuda and hasattr(self.model, "prefetch_geometry")):
            return None
        self.device = first.device
        self.join()
        rows = sum(int(p.shape[0]) for p in positions)
        name = ("P", (rows,) + tuple(first.shape[1:]), str(first.dtype), str(first.device))
        buf = self.inputs.get(name)
        if buf is None:
            buf = self.inputs[name] = torch.empty((rows,) + tuple(first.shape[1:]), dtype=first.dtype, device=first.device)
        at = 0
        for p in positions:
            if p.shape[1:] != first.shape[1:] or p.dtype != first.dtype:
                raise RuntimeError("GraphedForward.lookahead: positions of one shape and dtype, got %s %s and %s %s" %
                                   (tuple(first.shape), first.dtype, tuple(p.shape), p.dtype))
            buf[at:at + p.shape[0]].copy_(p)
            at += p.shape[0]
        main = torch.cuda.current_stream(self.device)
        if self.side is None:
            self.side = torch.cuda.Stream(device=self.device)
        self.side.wait_stream(main)                  # behind the copies above (and behind every reader of P's last product)
        with torch.cuda.stream(self.side):
            geometry = self._run(name, lambda: self.model.prefetch_geometry(buf, inline=True))
            if geometry is None:
                self.refused.setdefault(name, "GraphedForward: the model has no geometry for these positions")
            elif name not in self.graphs:            # an eager product: fresh side-stream memory the current stream will read
                for _, t in tree_tensors(geometry):
                    t.record_stream(main)
        self._pending = True
        return geometry

    def __call__(self, data, geometry=None, next_positions=None):
        """model(data, geometry=geometry) -> (logits, ...), replayed for a static geometry; next_positions: a list of
        positions for lookahead(), started between this call's copies and its forward pass (-> self.ahead)."""
        self._refuse_modes()
        pos = data["pos"]
        self.ahead = None
        graphable = geometry is not None and geometry.static and pos.is_cuda
        name = ("F", self.signature(data, geometry)) if graphable else None
        if name is None or name in self.refused:
            # nothing to replay: no static geometry (a short last batch, a model without one), or a refused signature
            if pos.is_cuda:
                self.device = pos.device
                self.join()
            if geometry is None:
                if next_positions:
                    self.ahead = self.lookahead(next_positions)
                return self.model(data)
            out = self.model(data, geometry=geometry)       # reads P's product where it lies: the next P starts behind it
            if next_positions:
                self.ahead = self.lookahead(next_positions)
            return out
        self.device = pos.device
        self._check_params()
        self.join()
        tensors = {k: v for k, v in data.items() if torch.is_tensor(v)}
        static = self.inputs.get(name)
        if static is None:
            static = self.inputs[name] = ({k: v.detach().clone().contiguous() for k, v in tensors.items()}, tree_clone(geometry))
        else:
            tree_copy_(static[0], tensors, "data")
            tree_copy_(static[1], geometry, "geometry")
        if next_positions:
            self.ahead = self.lookahead(next_positions)
        return self._run(name, lambda: self.model(static[0], geometry=static[1]))


_WRAPPERS = weakref.WeakKeyDictionary()     # model -> its GraphedForward (graph=True keeps the captures from epoch to epoch)


def graphed_forward(model):
    """The GraphedForward of `model`, made on first use and kept while the model lives (it reaches the model through a weak
    proxy: the table must not keep its own keys alive)."""
    if model not in _WRAPPERS:
        _WRAPPERS[model] = GraphedForward(weakref.proxy(model))
    return _WRAPPERS[model]
