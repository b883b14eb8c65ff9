"""The transform lists' random draws on the GPU (geot_view_draw, csrc/view_draw.hip): what ViewProgram.draw draws per item on
the host from the global torch-CPU, numpy and python `random` generators -- a handful of scalars per view, an (m, 3) normal
row per jittering transform, an (m,) uniform row per ChromaticPerDropGPU, finished on the host and uploaded through pinned
staging -- in ONE launch in front of geot_view_program, which then reads its job table, noise and masks from device buffers.

These are NOT torch's or numpy's draws: the kernel is a counter-based generator (Philox4x32-10; the contract is in
include/geot_hip.h), so every value depends on (seed, draw id, view, place in the list, quantity, point) alone, is the same
in every process and on every device, and is restated bit for bit in numpy float32 by tests/_view_draw_ref.py.

    layout = DrawLayout(jobs, n_rows, n_out, m, device, views, slots)    # once per (programs, batch layout): no draws in it
    drawn = view_program_draw(layout, seed, draw_base)                   # table, noise, mask on the device
    out = view_program_views_drawn(raw, layout, drawn)                   # geot_view_program on those buffers

The batchers do this when their `draws=` is a DeviceDraws(seed, views=True) (sample_draw.py)."""
import numpy as np
import torch

from ... import _lib
from ...ext._common import call, f32, need, ptr
from .view_program import pack_fixed_jobs

_MASK64 = (1 << 64) - 1


class DrawLayout:
    """The templates and draw plans of one batch layout: jobs a sequence of (source row, output row, program) -- or
    (.., program, None) -- views / slots per job as in pack_fixed_jobs.  Built on the host with nothing random in it and
    copied to the device ONCE; a batcher keeps one per batch shape."""

    def __init__(self, jobs, n_rows, n_out, m, device, views=None, slots=None):
        jobs = [(job[0], job[1], job[2], None) for job in jobs]
        self.m, self.n_rows, self.n_out, self.j = int(m), int(n_rows), int(n_out), len(jobs)
        self.tmpl, self.plans, noise, mask = pack_fixed_jobs(jobs, n_rows, n_out, m, views, slots)
        self.n_noise, self.n_mask = int(noise.shape[0]), int(mask.shape[0])
        self.has_heights = any(job[2].has_heights for job in jobs)
        self.device = torch.device(device)
        need(self.device.type == "cuda", "DrawLayout: CPU not supported (the draws happen on the GPU)")
        both = np.concatenate([self.tmpl.reshape(-1), self.plans.reshape(-1)])
        dev = torch.from_numpy(both).to(self.device)
        self.tmpl_dev, self.plans_dev = dev[:self.tmpl.size], dev[self.tmpl.size:]


def view_draw(layout, seed, draw_base):
    """The bare call: geot_view_draw on the current stream -> (table (J, VIEW_PROGRAM_JOB_WORDS) int32, noise (n_noise, m, 3),
    mask (n_mask, m)) on the device, no host synchronisation.  Job j draws with the draw id draw_base + its slot."""
    need(isinstance(layout, DrawLayout), "view_draw: layout must be a DrawLayout")
    dev = layout.device
    table = torch.empty((layout.j, _lib.VIEW_PROGRAM_JOB_WORDS), dtype=torch.int32, device=dev)
    noise = torch.empty((layout.n_noise, layout.m, 3), dtype=torch.float32, device=dev)
    mask = torch.empty((layout.n_mask, layout.m), dtype=torch.float32, device=dev)
    call("geot_view_draw", dev, layout.j, layout.m, layout.n_noise, layout.n_mask, layout.tmpl.ctypes.data,
         layout.plans.ctypes.data, ptr(layout.tmpl_dev), ptr(layout.plans_dev), int(seed) & _MASK64, int(draw_base) & _MASK64,
         ptr(table), ptr(noise) if layout.n_noise else None, ptr(mask) if layout.n_mask else None)
    return table, noise, mask


def view_program_draw(layout, seed, draw_base):
    """view_draw as a dict, for inspection: table, noise, mask (device tensors) and the layout they belong to."""
    table, noise, mask = view_draw(layout, seed, draw_base)
    return {"table": table, "noise": noise, "mask": mask, "layout": layout}


def view_program_views_drawn(raw, layout, drawn):
    """geot_view_program on what view_program_draw made: raw (n_rows, m, 3) CUDA float32 -> the dict of
    view_program_views.  The template table is what the entry point checks on the host; the kernel checks the drawn
    records themselves.  No host-to-device copy, no host synchronisation."""
    raw = f32(raw, "raw", 3)
    need(tuple(raw.shape) == (layout.n_rows, layout.m, 3) and raw.device == layout.device,
         "view_program_views_drawn: raw must be (%d, %d, 3) on %s" % (layout.n_rows, layout.m, layout.device))
    need(drawn["layout"] is layout, "view_program_views_drawn: these draws belong to another layout")
    dev, n_out, m = layout.device, layout.n_out, layout.m
    out = {"pos": torch.empty((n_out, m, 3), dtype=torch.float32, device=dev),
           "x": torch.empty((n_out, 3, m), dtype=torch.float32, device=dev),
           "heights": torch.empty((n_out, m, 1), dtype=torch.float32, device=dev) if layout.has_heights else None,
           "view_center": torch.empty((layout.j, 3), dtype=torch.float32, device=dev),
           "view_scale": torch.empty(layout.j, dtype=torch.float32, device=dev)}
    call("geot_view_program", dev, layout.j, m, layout.n_rows, n_out, layout.n_noise, layout.n_mask, ptr(raw),
         layout.tmpl.ctypes.data, ptr(drawn["table"]), ptr(drawn["noise"]) if layout.n_noise else None,
         ptr(drawn["mask"]) if layout.n_mask else None, ptr(out["pos"]), ptr(out["x"]), ptr(out["heights"]),
         ptr(out["view_center"]), ptr(out["view_scale"]))
    return out
