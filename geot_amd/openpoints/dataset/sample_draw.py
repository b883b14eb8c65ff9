"""The batchers' vertex sample drawn on the GPU (geot_sample_draw, csrc/sample_draw.hip): what the reference draws per item
on the host with np.random.choice(N_i, m, replace=N_i < m) (openpoints/dataset/tooth_semi/tooth_dataset.py:134-135,
340-341) -- numpy permutes the whole scan to keep m indices, milliseconds of serial host time per item -- for every slot of
a batch in one launch.

These are NOT numpy's draws: the kernel is a counter-based generator (Philox4x32-10 under a keyed bijection, the contract is
in include/geot_hip.h), so a row depends on (seed, draw id) alone and is the same in every process, on every device, in any
launch order.  The batchers' default stays the reference's host draws; they take `draws=DeviceDraws(seed)` to switch.

Covering draws (geot_sample_draw_cover): sample_draw_cover(..., p) is window p of the draw id's permutation of the whole scan,
so cover_passes(sizes, m) = max ceil(n / m) passes show a model every vertex once (ScanBatcher.cover, validation.cover_scans).
"""
import contextlib

import numpy as np
import torch

from ...ext._common import call, need, ptr
from .scan_set import DeviceScanSet

_MASK64 = (1 << 64) - 1


def _draw(entry, scans, scan_ids, m, seed, draw_base, *more):
    """The arguments and outputs geot_sample_draw and geot_sample_draw_cover share; more: what follows draw_base."""
    need(isinstance(scans, DeviceScanSet), "%s: scans must be a DeviceScanSet" % entry)
    dev = scans.device
    if scan_ids is None:
        ids_dev, s = None, len(scans)
    elif isinstance(scan_ids, torch.Tensor):
        need(scan_ids.dtype == torch.int64 and scan_ids.dim() == 1 and scan_ids.device == dev and scan_ids.is_contiguous(),
             "%s: scan_ids as a tensor must be (S,) int64, contiguous, on the scans' device" % entry)
        ids_dev, s = scan_ids, int(scan_ids.shape[0])
    else:
        ids = np.ascontiguousarray(np.asarray(scan_ids, dtype=np.int64).reshape(-1))
        ids_dev, s = torch.from_numpy(ids).pin_memory().to(dev, non_blocking=True), ids.size
    m = int(m)
    need(1 <= s <= 65535, "%s: 1 to 65535 slots, got %d" % (entry, s))
    need(m >= 1, "%s: m >= 1" % entry)
    sel = torch.empty((s, m), dtype=torch.int64, device=dev)
    bad = torch.empty(s, dtype=torch.int32, device=dev)
    call("geot_" + entry, dev, s, m, len(scans), int(scans.points.shape[0]), ptr(scans.offsets), ptr(ids_dev),
         int(seed) & _MASK64, int(draw_base) & _MASK64, *more, ptr(sel), ptr(bad))
    return sel, bad


def sample_draw(scans, scan_ids, m, seed, draw_base):
    """geot_sample_draw: scans a DeviceScanSet; scan_ids: the set scan of every slot -- S ints on the host, an (S,) int64
    tensor on the scans' device (used as it is) or None (slot i is scan i, S = len(scans)); slot i draws m vertex indices
    of its scan with the draw id draw_base + i -> (sel (S, m) int64, bad (S,) int32), both on the device, queued on the
    current stream without a host synchronisation.  A slot whose id lies outside the set gets a row of zeros and bad = 2
    (nothing is checked on the host: the sizes live on the device)."""
    return _draw("sample_draw", scans, scan_ids, m, seed, draw_base)


MAX_PASS = (1 << 31) - 1        # include/geot_hip.h geot_sample_draw_cover


def sample_draw_cover(scans, scan_ids, m, seed, draw_base, p):
    """geot_sample_draw_cover: sample_draw's arguments and results for pass p (0 .. 2^31 - 1) of a covering draw -- slot i's
    row holds positions p m .. p m + m - 1 (mod n_i) of ONE permutation of its scan's n_i vertices, the permutation of the
    draw id draw_base + i.  Passes 0 .. cover_passes([n_i], m) - 1 of the same ids name every vertex of every slot; for
    n_i >= m pass 0 is sample_draw's row.  Positions past n_i are wrap-around fill (the start of the permutation again)."""
    need(isinstance(p, (int, np.integer)) and not isinstance(p, bool) and 0 <= int(p) <= MAX_PASS,
         "sample_draw_cover: the pass must be an int in 0..%d, got %r" % (MAX_PASS, p))
    return _draw("sample_draw_cover", scans, scan_ids, m, seed, draw_base, int(p))


def cover_passes(sizes, m):
    """How many passes of m samples cover scans of `sizes` vertices: max ceil(n / m) (host arithmetic)."""
    sizes, m = [int(n) for n in sizes], int(m)
    need(m >= 1 and len(sizes) >= 1 and all(n >= 1 for n in sizes), "cover_passes: m >= 1 and at least one scan of n >= 1 vertices")
    return max(-(-n // m) for n in sizes)


class DeviceDraws:
    """The seed and the draw counter of the device-side sampling.  A batcher called with `draws=` takes ONE draw id per
    batch slot from it, in slot order -- FixMatchBatcher: the labelled slots first, then the unlabelled ones -- whenever it
    draws at least one row of the batch itself (with every row given explicitly, sel= / sel_l= and sel_u=, nothing is
    taken).  Slot i of that batch is row `sample_draw(..., seed, base)[i]` with base = the counter before the batch, so
    two objects with the same seed and counter yield the same batches, and one id is never used twice while the counter
    has not wrapped (2^64 ids).

    take(count) returns the current counter and advances it by count; state() / set_state() save and restore
    (seed, counter), e.g. in a checkpoint, so that a resumed run continues the sequence.

    views=True: the batchers draw the transform lists' parameters on the device too (view_draw.py: geot_view_draw) --
    every view parameter, jitter noise row and per-point colour mask of slot i comes from the SAME draw id as its vertex
    sample, under counter words of their own, so a batch depends on (seed, counter) alone and no host generator is read.
    The counter advances as without the flag: one id per slot.  views=False (the default) is the vertex sample alone.
    state() carries the flag when it is set; set_state() takes either form."""

    def __init__(self, seed, counter=0, views=False):
        self.seed, self.counter, self.views = int(seed) & _MASK64, int(counter) & _MASK64, bool(views)

    def take(self, count):
        count = int(count)
        need(count >= 0, "DeviceDraws.take: count >= 0")
        base = self.counter
        self.counter = (base + count) & _MASK64
        return base

    def state(self):
        out = {"seed": self.seed, "counter": self.counter}
        if self.views:
            out["views"] = True
        return out

    def set_state(self, state):
        self.seed, self.counter = int(state["seed"]) & _MASK64, int(state["counter"]) & _MASK64
        self.views = bool(state.get("views", False))


class ViewDrawHandle:
    """What a batcher's draw() returns in place of host parameters under DeviceDraws(views=True): the seed, the first
    draw id and the number of slots.  batch(params=handle) draws the very same view parameters again (on the device)."""

    def __init__(self, seed, base, count):
        self.seed, self.base, self.count = int(seed) & _MASK64, int(base) & _MASK64, int(count)

    def __repr__(self):
        return "ViewDrawHandle(seed=%d, base=%d, count=%d)" % (self.seed, self.base, self.count)


def on_stream(stream):
    """The batchers' `with`: their side stream, or nothing (the current stream) without one."""
    return contextlib.nullcontext() if stream is None else torch.cuda.stream(stream)


def draw_batch_sel(scans, ids, m, draws, given=(), base=None):
    """The device half of a batcher's sampling: one id per slot taken from `draws`, one geot_sample_draw launch on the
    current stream -> (sel (S, m) int64 on the device, the scan ids on the device).  given: (first slot, host rows or None)
    pairs -- rows a caller passed explicitly replace the drawn ones (pinned copy, no synchronisation).  base: the first
    draw id when the caller has taken the ids itself."""
    need(isinstance(draws, DeviceDraws), "draws must be a DeviceDraws (or None: the reference's host draws)")
    ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
    ids_dev = torch.from_numpy(ids).pin_memory().to(scans.device, non_blocking=True)
    sel, _ = sample_draw(scans, ids_dev, m, draws.seed, draws.take(ids.size) if base is None else base)
    for first, rows in given:
        if rows is not None and len(rows):
            host = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).pin_memory()
            sel[first:first + len(rows)].copy_(host, non_blocking=True)
    return sel, ids_dev
