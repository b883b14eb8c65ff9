"""What the three batchers (fixmatch_batch, supervised_batch, val_batch) share: a batch is the host half -- every slot's
vertex sample and view parameters, given, drawn on the host in the reference's per-item order or left to the device
(sample_draw.DeviceDraws) -- then geot_cloud_sample_batch (5 launches), ONE views launch, one gather of the jaw flags, all
on the batcher's stream and without a host synchronisation.  A batcher itself says only which scans its slots read
(the `ids` it hands over), which view jobs a batch has (_jobs) and which dict it returns (_result)."""
import numpy as np
import torch

from ...ext._common import need
from .sample_draw import DeviceDraws, ViewDrawHandle, draw_batch_sel, on_stream
from .scan_set import DeviceScanSet, _to_device, check_curvature, cloud_sample_batch, curvature_sample, raise_bad_index
from .view_draw import DrawLayout, view_program_draw, view_program_views_drawn
from .view_program import pack_program_jobs, view_program_views


class Batcher:
    """The shared body (module text).  A batcher defines _jobs(*shape) -> (jobs [(source row, output row, program)], rows of
    raw, output rows, view number per job or None, slot per job or None) and _result(sampled, views, cls, ids, *shape) -> what
    batch() returns; one whose views do not all run on geot_view_program overrides _pack and _views.
    curvatures=True (every batcher's constructor; default False: not one launch, allocation, key or bit differs): every dict
    of a batch also holds "curvatures" (B, m) float32 -- the set's curvature (DeviceScanSet.compute_curvature) at the slots'
    sampled vertices, as the reference's datasets make data['curvatures'] (tooth_dataset.py:156-160, 320-359): abs, min-max
    over the WHOLE scan, gathered at the sample; 0 for a scan whose max equals its min.  One more launch
    (geot_curvature_sample) on the batcher's stream.  A set without computed curvature, or a scan of the batch without a mesh,
    is a ValueError before any device call; check=True also raises for an index outside its scan seen by that launch."""

    stream = draws = None    # (the constructor's; None: the current stream, the reference's host draws)
    curvatures = False

    def __init__(self, scans, num_points, num_classes, stream, draws, curvatures=False):
        who = type(self).__name__
        need(isinstance(scans, DeviceScanSet), "%s: scans must be a DeviceScanSet" % who)
        need(scans.device.type == "cuda", "%s: CPU not supported (the scans must live on the GPU)" % who)
        need(int(num_points) >= 1, "%s: num_points >= 1" % who)
        need(1 <= int(num_classes) <= 4096, "%s: num_classes must be in [1, 4096]" % who)
        self.scans, self.device = scans, scans.device
        self.m, self.c, self.stream, self.draws = int(num_points), int(num_classes), stream, draws
        self.curvatures = bool(curvatures)
        self._layouts = {}          # batch shape -> DrawLayout (templates and plans on the device, built once)
        if stream is not None:      # once: the scans are ready; a batch itself depends on nothing the current stream does
            stream.wait_stream(torch.cuda.current_stream(self.device))

    def _draw(self, ids, given, params, draws, draw_slot):
        """The host half of a batch.  ids: the set scan of every slot; given: (name, rows or None, count) per run of slots,
        in slot order -- the vertex indices a caller passed; params: the view parameters a caller passed (one entry per
        slot), a ViewDrawHandle, or None; draws: a DeviceDraws for this call (default: the constructor's); draw_slot(slot):
        that slot's view parameters from the host generators.  Everything not given is drawn: on the host per item in the
        reference's order, np.random.choice (tooth_dataset.py:134-135, 340-341) and then the item's views, or with a
        DeviceDraws by geot_sample_draw on the batcher's stream -- ONE draw id per slot, whatever it serves.
        -> (sel (S, m) int64, host array or device tensor; params; the scan ids on the device when the device drew)"""
        draws = self.draws if draws is None else draws
        need(draws is None or isinstance(draws, DeviceDraws), "draws must be a DeviceDraws (or None: the reference's host draws)")
        if self.curvatures:
            check_curvature(self.scans, ids, type(self).__name__)
        runs, first = [], 0
        for name, rows, count in given:
            if rows is not None:
                rows = np.asarray(rows.cpu() if isinstance(rows, torch.Tensor) else rows)
                need(rows.shape == (count, self.m) and rows.dtype.kind in "iu", "%s must be (%d, %d) integers" % (name, count, self.m))
                rows = rows.astype(np.int64)
            runs.append((first, rows))
            first += count
        if isinstance(params, ViewDrawHandle):
            need(params.count == len(ids), "params: the handle was drawn for %d slots" % params.count)
        elif params is not None:
            need(len(params) == len(ids), "params: one entry per slot (%d)" % len(ids))
        on_device = draws is not None and any(rows is None for _, rows in runs)
        device_views = draws is not None and draws.views and params is None
        base = draws.take(len(ids)) if on_device or device_views else None
        if device_views:
            params = ViewDrawHandle(draws.seed, base, len(ids))
        ids_dev, missing = None, np.zeros(len(ids), dtype=bool)
        if on_device:
            with on_stream(self.stream):
                sel, ids_dev = draw_batch_sel(self.scans, ids, self.m, draws, runs, base=base)
        else:
            sel = np.empty((len(ids), self.m), dtype=np.int64)
            for (first, rows), (_, _, count) in zip(runs, given):
                if rows is None:
                    missing[first:first + count] = True
                else:
                    sel[first:first + count] = rows
        drawn = []
        for slot, scan in enumerate(ids):
            if missing[slot]:
                n = self.scans.sizes[scan]
                sel[slot] = np.random.choice(n, self.m, replace=n < self.m)
            if params is None:
                drawn.append(draw_slot(slot))
        if params is None:
            params = drawn
        return sel, (params if isinstance(params, ViewDrawHandle) else list(params)), ids_dev

    def _layout(self, *shape):
        """The templates and draw plans of a batch of this shape, on the device (the views' parameters drawn there)."""
        if shape not in self._layouts:
            jobs, n_rows, n_out, views, slots = self._jobs(*shape)
            self._layouts[shape] = DrawLayout(jobs, n_rows, n_out, self.m, self.device, views, slots)
        return self._layouts[shape]

    def _pack(self, shape, params):
        """Host parameters, one entry per job, checked and packed before anything is queued -> what _views takes."""
        jobs, n_rows, n_out = self._jobs(*shape)[:3]
        jobs = [job + (p,) for job, p in zip(jobs, params)]
        return jobs, n_out, pack_program_jobs(jobs, n_rows, n_out, self.m)

    def _views(self, raw, packed):
        return view_program_views(raw, packed[0], packed[1], packed[2])

    def _batch(self, ids, shape, sel, params, ids_dev, check, affine=False):
        """Queue one batch: params a ViewDrawHandle or one host entry per JOB.  check=True reads the bad-index flags back
        (one host sync) and raises IndexError.  affine=True: the batcher's _affine(views, *shape) is added to the result --
        tensors the views launch writes anyway, so the batch costs the same."""
        handle = isinstance(params, ViewDrawHandle)
        packed = None if handle else self._pack(shape, params)
        with on_stream(self.stream):
            if self.curvatures:     # the sample on the device once, for both launches that read it
                sel = (sel.to(self.device).contiguous() if isinstance(sel, torch.Tensor)
                       else _to_device(np.ascontiguousarray(sel), self.device))
            s = cloud_sample_batch(self.scans, ids, sel, self.c, check=False, ids_dev=ids_dev)
            if handle:      # the parameters are drawn where they are used
                layout = self._layout(*shape)
                v = view_program_views_drawn(s["raw"], layout, view_program_draw(layout, params.seed, params.base))
            else:
                v = self._views(s["raw"], packed)
            out = self._result(s, v, self.scans.cls.index_select(0, s["scan_ids"]).view(-1, 1), ids, *shape)
            if affine:
                out.update(self._affine(v, *shape))
            if self.curvatures:
                cur, cur_bad = curvature_sample(self.scans, s["scan_ids"], sel)
                self._add_curvatures(out, cur, *shape)
        if check:
            if self.stream is not None:
                self.stream.synchronize()
            raise_bad_index(s["bad"], ids)
            if self.curvatures:
                raise_bad_index(cur_bad, ids)
        return out

    def _add_curvatures(self, out, cur, *shape):
        """Put the (slots, m) curvatures into what _result returned (a batcher that returns several dicts splits them)."""
        out["curvatures"] = cur

    def _join(self, tensors):
        """Hand a batch built on the side stream to the CURRENT stream: it waits for the side stream, and the caching
        allocator is told that the batch's memory is in use here (train_step._join does the same for the steps' side streams)."""
        if self.stream is None:
            return
        cur = torch.cuda.current_stream(self.device)
        cur.wait_stream(self.stream)
        for t in tensors:
            t.record_stream(cur)
