"""Transform lists compiled into per-view programs for geot_view_program (csrc/view_program.hip) -- the reference composes a
list of transform classes per item on a CPU worker (openpoints/transforms/point_transformer_gpu.py, built by
build_transforms_from_cfg: every class receives the WHOLE kwargs dict and takes its own defaults for absent keys).

    program = ViewProgram(["PointsToTensor", "PointCloudScaling", "PointCloudCenterAndNormalize", "PointCloudJitter",
                           "ChromaticDropGPU"], {"scale": [0.8, 1.2], "gravity_dim": 1, "jitter_sigma": 0.001, ...})
    params = program.draw(m)                 # one view's random draws: host, the reference's statements in its order
    out = view_program_views(raw, [(src_row, out_row, program, params), ...], n_out)

Supported (the point count must not change):

    PointsToTensor, PointCloudToTensor                  nothing
    PointCloudScaling(_s)                               pos *= scale                          in place
    PointCloudCenterAndNormalize                        heights; pos = pos - mean; pos = pos / max norm   rebinds pos
    PointCloudXYZAlign                                  pos -= mean; pos[:, g] -= min         in place
    PointCloudTranslation(_s)                           pos += rand * shift                   in place
    PointCloudScaleAndTranslate(_s)                     pos = mul(pos, scale) + t             rebinds pos
    PointCloudJitter(_s)                                pos += clamp(noise * std)             in place
    PointCloudScaleAndJitter                            pos = mul(pos, scale) + noise         rebinds pos
    PointCloudRotation(_s)                              pos = pos @ R.T                       rebinds pos
    RandomHorizontalFlip                                pos[:, ax] = max(pos) - pos[:, ax]    in place
    ChromaticDropGPU                                    x[:, :3] = 0                          in place, on x
    ChromaticPerDropGPU                                 x[:, :3] *= mask                      in place, on x

The aliasing quirk of the reference is kept: the dataset sets data['x'] = data['pos'] (ONE tensor), so an in-place transform
changes both, and a transform that rebinds data['pos'] separates them for the rest of the list.  What the compiler makes of
that: once x has separated from pos only the two chromatic transforms can still touch it, and they depend on the draws
alone -- so x is written exactly ONCE, by a STORE_X op in front of the separating op, with every later zero / mask folded
into that store.  A list that never rebinds has x = the final pos: the chromatic transforms then act on pos at their place
in the list and STORE_X is the last op.

By default the random numbers stay on the host (view_draw.py draws them on the device instead: compile_fixed below is the
layout it fills in).  draw() consumes the GLOBAL torch-CPU, numpy and python `random` generators exactly as
the classes do; noise and per-point masks are finished on the host with torch's own randn_like / rand, multiply and clamp_
and travel as (m, 3) / (m,) fp32 rows, together with the job records, through one pinned staging buffer per launch.
"""
import random

import numpy as np
import torch

from ... import _lib
from ...ext._common import call, f32, need, ptr

# op kinds of include/geot_hip.h geot_view_program
SCALE, CENTER_NORM, XYZ_ALIGN, TRANSLATE, SCALE_TRANSLATE, JITTER, SCALE_JITTER, ROTATE, FLIP, ZERO, MASK, STORE_X = range(1, 13)
_HEADER_WORDS, _OP_WORDS = 8, 14

_SUFFIXED = {"PointCloudScaling_s": "PointCloudScaling", "PointCloudTranslation_s": "PointCloudTranslation",
             "PointCloudScaleAndTranslate_s": "PointCloudScaleAndTranslate", "PointCloudJitter_s": "PointCloudJitter",
             "PointCloudRotation_s": "PointCloudRotation"}
_NOTHING = ("PointsToTensor", "PointCloudToTensor")
_REBINDING = ("PointCloudScaleAndTranslate", "PointCloudScaleAndJitter", "PointCloudRotation")
_REFUSED = {"RandomDropout": "it changes the point count", "ChromaticNormalize": "colour statistics on real colour channels"}
_SCALE_DEFAULT = [2. / 3, 3. / 2]
_ONE, _ZERO3, _EYE9 = np.ones(3, np.float32), np.zeros(3, np.float32), np.eye(3, dtype=np.float32).reshape(9)   # (read only)


def _axis_rotation(axis, theta):
    if theta == 0:
        return np.eye(3)                 # expm(0) exactly; the configured case needs no scipy
    from scipy.linalg import expm, norm  # the reference's own routine: its Pade approximant is part of R's bits
    return expm(np.cross(np.eye(3), axis / norm(axis) * theta))


class _Step:
    """One transform of a list: its base class name, the keyword values it read and whether it rebinds data['pos']."""

    def __init__(self, name, kwargs):
        self.name = name
        base = _SUFFIXED.get(name, name)
        sfx = "_s" if name in _SUFFIXED else ""
        self.base, kw = base, (lambda key, default: kwargs[key] if key in kwargs else default)
        self.rebinds = base in _REBINDING
        if base in _NOTHING:
            return
        if base in ("PointCloudScaling", "PointCloudScaleAndTranslate", "PointCloudScaleAndJitter"):
            key = "scale" + sfx
            self.scale_min, self.scale_max = np.array(kw(key, _SCALE_DEFAULT)).astype(np.float32)
            self.anisotropic = bool(kw("anisotropic", True))
            self.scale_xyz = [bool(v) for v in kw("scale_xyz", [True, True, True])]
            need(len(self.scale_xyz) == 3, "%s: scale_xyz has three entries" % name)
            need(self.anisotropic or all(self.scale_xyz[1:]), "%s: anisotropic=False with scale_xyz[1:] unset indexes a "
                 "one-element scale in the reference" % name)
            self.mirror = torch.from_numpy(np.array(kw("mirror", [0, 0, 0])))
            need(tuple(self.mirror.shape) == (3,), "%s: mirror has three entries" % name)
            self.use_mirroring = bool(torch.sum(self.mirror > 0) != 0)
            need(self.anisotropic or not (self.use_mirroring or base == "PointCloudScaleAndJitter"),
                 "%s: mirroring needs anisotropic=True" % name)
        if base == "PointCloudScaleAndTranslate":
            self.shift = torch.from_numpy(np.array(kw("shift" + sfx, [0.2, 0.2, 0.2]))).to(torch.float32)
        if base == "PointCloudTranslation":
            self.shift = torch.from_numpy(np.array(kw("shift" + sfx, [0.2, 0.2, 0.]))).to(torch.float32)
        if base in ("PointCloudTranslation", "PointCloudScaleAndTranslate"):
            need(tuple(self.shift.shape) == (3,), "%s: shift has three entries" % name)
        if base in ("PointCloudJitter", "PointCloudScaleAndJitter"):
            self.noise_std, self.noise_clip = kw("jitter_sigma" + sfx, 0.01), kw("jitter_clip" + sfx, 0.05)
        if base == "PointCloudRotation":
            self.angle = np.array(kw("angle" + sfx, [0, 0, 0])) * np.pi
            self.angle_pi = np.array(kw("angle" + sfx, [0, 0, 0]), dtype=np.float32)     # the bound in units of pi (view_draw)
            need(self.angle.shape == (3,), "%s: angle has three entries" % name)
        if base in ("PointCloudCenterAndNormalize", "PointCloudXYZAlign"):
            self.gravity_dim = int(kw("gravity_dim", 2))
            need(self.gravity_dim in (0, 1, 2), "%s: gravity_dim must be 0, 1 or 2" % name)
        if base == "PointCloudCenterAndNormalize":
            if kw("append_xyz", False):
                raise NotImplementedError("PointCloudCenterAndNormalize(append_xyz=True) is not supported: heights would be (m, 3)")
            self.centering, self.normalize = bool(kw("centering", True)), bool(kw("normalize", True))
            self.rebinds = self.centering or self.normalize
        if base == "RandomHorizontalFlip":
            need("upright_axis" in kwargs, "RandomHorizontalFlip needs upright_axis ('x', 'y' or 'z')")
            upright = {"x": 0, "y": 1, "z": 2}[str(kwargs["upright_axis"]).lower()]
            self.horz_axes = set(range(3)) - set([upright])
            self.aug_prob = kw("aug_prob", 0.95)
        if base in ("ChromaticDropGPU", "ChromaticPerDropGPU"):
            self.color_drop = kw("color_drop", 0.2)

    # ---- the draws: the classes' own statements, in their order
    def _draw_scale(self, jitter_mirror):
        scale = torch.rand(3 if self.anisotropic else 1, dtype=torch.float32) * (self.scale_max - self.scale_min) + self.scale_min
        if jitter_mirror:                        # PointCloudScaleAndJitter: always drawn, weighted by `mirror`
            mirror = torch.round(torch.rand(3)) * 2 - 1
            mirror = mirror * self.mirror + (1 - self.mirror)
            scale *= mirror
        elif self.use_mirroring:
            mirror = (torch.rand(3) > self.mirror).to(torch.float32) * 2 - 1
            scale *= mirror
        for i, s in enumerate(self.scale_xyz):
            if not s:
                scale[i] = 1
        return np.broadcast_to(scale.numpy(), (3,)).astype(np.float32)

    def _draw_noise(self, m):
        noise = torch.randn_like(torch.empty(m, 3, dtype=torch.float32)) * self.noise_std
        return noise.clamp_(-self.noise_clip, self.noise_clip).numpy()

    def draw(self, m):
        base = self.base
        if base == "PointCloudScaling":
            return {"scale": self._draw_scale(False)}
        if base == "PointCloudTranslation":
            return {"t": (torch.rand(3, dtype=torch.float32) * self.shift).numpy()}
        if base == "PointCloudScaleAndTranslate":
            scale = self._draw_scale(False)
            return {"scale": scale, "t": ((torch.rand(3, dtype=torch.float32) - 0.5) * 2 * self.shift).numpy()}
        if base == "PointCloudJitter":
            return {"noise": self._draw_noise(m)}
        if base == "PointCloudScaleAndJitter":
            scale = self._draw_scale(True)
            return {"scale": scale, "noise": self._draw_noise(m)}
        if base == "PointCloudRotation":
            mats = []
            for ax, bound in enumerate(self.angle):
                axis = np.zeros(3)
                axis[ax] = 1
                mats.append(_axis_rotation(axis, np.random.uniform(-bound, bound)))
            np.random.shuffle(mats)
            return {"R": torch.tensor(mats[0] @ mats[1] @ mats[2], dtype=torch.float32).numpy()}
        if base == "RandomHorizontalFlip":
            flips = []
            if random.random() < self.aug_prob:
                for ax in self.horz_axes:
                    if random.random() < 0.5:
                        flips.append(ax)
            return {"flip": flips}
        if base == "ChromaticDropGPU":
            return {"drop": bool(torch.rand(1) < self.color_drop)}
        if base == "ChromaticPerDropGPU":
            return {"mask": (torch.rand((m, 1)) > self.color_drop).to(torch.float32).numpy().reshape(m)}
        return {}


class ViewProgram:
    """A transform list, given by the reference's class names and the kwargs dict every class receives, compiled for
    geot_view_program.  Raises NotImplementedError -- naming the transform, before any device call -- for RandomDropout,
    ChromaticNormalize, append_xyz=True and unknown names.

    x_is_pos: nothing in the list rebinds data['pos'], so x is the final pos (and the chromatic drops hit pos too).
    has_heights: the list has a PointCloudCenterAndNormalize, the only transform that makes data['heights']."""

    def __init__(self, transform_names, kwargs=None):
        kwargs = {} if kwargs is None else dict(kwargs)
        self.names, self.kwargs, self.steps = list(transform_names), kwargs, []
        for name in self.names:
            base = _SUFFIXED.get(name, name)
            if base in _REFUSED:
                raise NotImplementedError("ViewProgram: %s is not supported (%s)" % (name, _REFUSED[base]))
            if base not in _NOTHING + _REBINDING + ("PointCloudScaling", "PointCloudCenterAndNormalize", "PointCloudXYZAlign",
                                                    "PointCloudTranslation", "PointCloudJitter", "RandomHorizontalFlip",
                                                    "ChromaticDropGPU", "ChromaticPerDropGPU"):
                raise NotImplementedError("ViewProgram: unknown transform %r" % (name,))
            self.steps.append(_Step(name, kwargs))
        self.x_is_pos = not any(s.rebinds for s in self.steps)
        self.has_heights = any(s.base == "PointCloudCenterAndNormalize" for s in self.steps)
        worst = sum(2 if s.base == "RandomHorizontalFlip" else 0 if s.base in _NOTHING else 1 for s in self.steps) + 1
        need(worst <= _lib.VIEW_MAX_OPS, "ViewProgram: the list may need %d ops, the kernel takes %d" % (worst, _lib.VIEW_MAX_OPS))

    def draw(self, m):
        """One view's parameters: a list with one dict per transform of the list (empty for those that draw nothing), drawn
        from the GLOBAL torch-CPU, numpy and python `random` generators with the reference's statements in its order."""
        m = int(m)
        need(m >= 1, "ViewProgram.draw: m >= 1")
        return [s.draw(m) for s in self.steps]

    def compile(self, params, m):
        """The ops of one view -> (ops, noise rows, mask rows): ops a list of (kind, arg, floats), rows lists of (m, 3) / (m,)
        float32 arrays the ops' args index.  Everything is checked here, on the host."""
        walked = self._walk(params, m, False)
        return walked["ops"], walked["noise"], walked["masks"]

    def compile_fixed(self, params=None, m=None):
        """The list in the FIXED layout geot_view_draw works on (view_draw.py): one op sequence for every draw, so that
        the device can fill it in.  Against compile(): every RandomHorizontalFlip is two ops (FLIP, or SCALE by 1 when that
        axis is not flipped), a ChromaticDropGPU on pos is one op (ZERO, or SCALE by 1), and when a per-point mask can reach
        x the combined mask row exists whether or not a drop overrides it -- SCALE by (1, 1, 1) is a bit-exact no-op, so the
        views equal compile()'s.  params None: the TEMPLATE -- the worst case (both flips, the zeroing, the masked store)
        with every drawn float neutral -- else the record a view with these draws has.
        -> dict(ops, n_noise, n_mask, noise, masks, store_at, steps); steps: the draw plan, tuples (kind, op index or -1,
        position in the list, flags, constants) in the layout of include/geot_hip.h geot_view_draw."""
        return self._walk(params, m, True)

    def _walk(self, params, m, fixed):
        """compile() and compile_fixed(): one pass over the list that keeps the aliasing books (module text) -> the dict of
        compile_fixed.  fixed: that layout, and the draw plan with it; params may then be None (the template)."""
        tmpl = fixed and params is None
        need(tmpl or (isinstance(params, (list, tuple)) and len(params) == len(self.steps)),
             "ViewProgram: parameters are a list with one dict per transform (%d), see draw()" % len(self.steps))
        one, zero3 = _ONE, _ZERO3
        ops, steps, noise, masks, x_masks = [], [], [], [], []
        aliased, store_at, x_zero, masked_x, n_noise, n_mask = True, -1, False, False, 0, 0

        def vec(p, key, what, neutral, shape=(3,)):       # (the messages are formatted only when they are raised: this
            if tmpl:                                      # runs per job of every batch)
                return neutral
            if not (isinstance(p, dict) and key in p):
                need(False, "%s: the parameters lack %r (ViewProgram.draw)" % (what, key))
            v = np.asarray(p[key], dtype=np.float32)
            if v.shape != shape:
                need(False, "%s: %s must be %s" % (what, key, shape))
            return v

        def row(p, key, shape, what, into):
            if tmpl:
                return
            if not (isinstance(p, dict) and key in p):
                need(False, "%s: the parameters lack %r (ViewProgram.draw)" % (what, key))
            v = np.ascontiguousarray(p[key], dtype=np.float32)
            if m is not None and v.shape != shape:
                need(False, "%s: %s must be %s, got %s" % (what, key, shape, v.shape))
            into.append(v)

        def plan_scale(step, op, pos, form):
            flags = (1 if step.anisotropic else 0) | sum(2 << k for k in range(3) if step.scale_xyz[k]) | (form << 4)
            mirror = step.mirror.to(torch.float32).numpy()
            steps.append((1, op, pos, flags, [step.scale_min, np.float32(step.scale_max - step.scale_min)] + list(mirror)))

        for pos, step in enumerate(self.steps):
            base, what, p = step.base, step.name, (None if tmpl else params[pos])
            if step.rebinds and aliased:         # x leaves pos here: it is stored once, in front of this op
                store_at, aliased = len(ops), False
                ops.append(None)
            at = len(ops)
            if base == "PointCloudScaling":
                ops.append((SCALE, 0, vec(p, "scale", what, one)))
                if fixed:
                    plan_scale(step, at, pos, 1 if step.use_mirroring else 0)
            elif base == "PointCloudCenterAndNormalize":
                ops.append((CENTER_NORM, (1 if step.centering else 0) | (2 if step.normalize else 0) | (step.gravity_dim << 2), []))
            elif base == "PointCloudXYZAlign":
                ops.append((XYZ_ALIGN, step.gravity_dim, []))
            elif base == "PointCloudTranslation":
                ops.append((TRANSLATE, 0, vec(p, "t", what, zero3)))
                if fixed:
                    steps.append((2, at, pos, 0, list(step.shift.numpy())))
            elif base == "PointCloudScaleAndTranslate":
                ops.append((SCALE_TRANSLATE, 0, np.concatenate([vec(p, "scale", what, one), vec(p, "t", what, zero3)])))
                if fixed:
                    plan_scale(step, at, pos, 1 if step.use_mirroring else 0)
                if fixed:
                    steps.append((2, at, pos, 1, list(step.shift.numpy())))
            elif base in ("PointCloudJitter", "PointCloudScaleAndJitter"):
                if base == "PointCloudJitter":
                    ops.append((JITTER, n_noise, []))
                else:
                    ops.append((SCALE_JITTER, n_noise, vec(p, "scale", what, one)))
                    if fixed:
                        plan_scale(step, at, pos, 2)
                if fixed:
                    steps.append((3, at, pos, 0, [step.noise_std, step.noise_clip]))
                row(p, "noise", (m, 3), what, noise)
                n_noise += 1
            elif base == "PointCloudRotation":
                ops.append((ROTATE, 0, vec(p, "R", what, _EYE9, (3, 3)).reshape(9)))
                if fixed:
                    steps.append((4, at, pos, 0, list(step.angle_pi)))
            elif base == "RandomHorizontalFlip":
                need(tmpl or (isinstance(p, dict) and "flip" in p), "%s: the parameters lack 'flip' (ViewProgram.draw)" % what)
                flips = [] if tmpl else [int(ax) for ax in p["flip"]]
                for ax in flips:
                    need(ax in step.horz_axes, "%s: axis %r is not a horizontal axis" % (what, ax))
                for ax in (step.horz_axes if fixed else flips):      # fixed: a place for either axis, flipped or not
                    ops.append((FLIP, int(ax), []) if tmpl or ax in flips else (SCALE, 0, one))
                if fixed:
                    steps.append((5, at, pos, 0, [step.aug_prob]))
            elif base == "ChromaticDropGPU":
                need(tmpl or (isinstance(p, dict) and "drop" in p), "%s: the parameters lack 'drop' (ViewProgram.draw)" % what)
                drop = tmpl or bool(p["drop"])
                if not aliased:
                    x_zero = x_zero or (drop and not tmpl)
                elif drop or fixed:
                    ops.append((ZERO, 0, []) if drop else (SCALE, 0, one))
                if fixed:
                    steps.append((6, at if aliased else -1, pos, 0, [step.color_drop]))
            elif base == "ChromaticPerDropGPU":
                if aliased:
                    ops.append((MASK, n_mask, []))
                    row(p, "mask", (m,), what, masks)
                    n_mask += 1
                else:
                    masked_x = True
                    row(p, "mask", (m,), what, x_masks)
                if fixed:
                    steps.append((7, at if aliased else -1, pos, 0, [step.color_drop]))
        if aliased:
            ops.append((STORE_X, 0, []))
        else:
            ops[store_at] = (STORE_X, 1 if x_zero else (2 | (n_mask << 2)) if masked_x else 0, [])
            if masked_x and (fixed or not x_zero):   # 0 / 1 masks: their product, applied once, is the chain of multiplies
                n_mask += 1
                if not tmpl:
                    combined = x_masks[0]
                    for extra in x_masks[1:]:
                        combined = combined * extra
                    masks.append(combined)
        need(len(ops) <= _lib.VIEW_MAX_OPS, "ViewProgram: %d ops, the kernel takes %d" % (len(ops), _lib.VIEW_MAX_OPS))
        if fixed:
            need(len(steps) <= _lib.VIEW_DRAW_MAX_STEPS, "ViewProgram: the list draws %d quantities, geot_view_draw takes %d"
                 % (len(steps), _lib.VIEW_DRAW_MAX_STEPS))
            need(len(self.steps) <= 4096, "ViewProgram: geot_view_draw takes lists of up to 4096 transforms")
        return {"ops": ops, "n_noise": n_noise, "n_mask": n_mask, "noise": noise, "masks": masks,
                "store_at": -1 if aliased else store_at, "steps": steps}

    def pack(self, jobs, n_rows, n_out, m):
        """jobs: sequence of (source row, output row, params) of THIS program -> pack_program_jobs."""
        need(all(len(job) == 3 for job in jobs), "ViewProgram.pack: a job is (source row, output row, params)")
        return pack_program_jobs([(job[0], job[1], self, job[2]) for job in jobs], n_rows, n_out, m)


def _pack_jobs(jobs, n_rows, n_out, m, who, fixed):
    """The job and row checks and the record writer of pack_program_jobs and pack_fixed_jobs -> (table, noise, masks, what
    ViewProgram._walk made of every job)."""
    need(len(jobs) >= 1, "%s: at least one job" % who)
    m = int(m)
    need(m >= 1, "%s: m >= 1" % who)
    table = np.zeros((len(jobs), _lib.VIEW_PROGRAM_JOB_WORDS), dtype=np.int32)
    as_f = table.view(np.float32)
    noise, masks, walked, n_noise, n_mask, seen = [], [], [], 0, 0, set()
    for j, job in enumerate(jobs):
        need(len(job) == 4 and isinstance(job[2], ViewProgram), "%s: a job is (source row, output row, program, params)" % who)
        src, dst = int(job[0]), int(job[1])
        need(0 <= src < n_rows, "%s: job %d reads row %d of %d" % (who, j, src, n_rows))
        need(0 <= dst < n_out and dst not in seen, "%s: job %d writes row %d (of %d; each row once)" % (who, j, dst, n_out))
        seen.add(dst)
        w = job[2]._walk(job[3], m, fixed)
        table[j, :5] = src, dst, len(w["ops"]), n_noise, n_mask
        for o, (kind, arg, floats) in enumerate(w["ops"]):
            at = _HEADER_WORDS + o * _OP_WORDS
            table[j, at], table[j, at + 1] = kind, arg
            as_f[j, at + 2:at + 2 + len(floats)] = floats
        n_noise += w["n_noise"]
        n_mask += w["n_mask"]
        noise += w["noise"] if job[3] is not None else [np.zeros((m, 3), np.float32)] * w["n_noise"]      # (the template's)
        masks += w["masks"] if job[3] is not None else [np.zeros(m, np.float32)] * w["n_mask"]
        walked.append(w)
    noise = np.stack(noise) if noise else np.zeros((0, m, 3), np.float32)
    masks = np.stack(masks) if masks else np.zeros((0, m), np.float32)
    return table, noise, masks, walked


def pack_program_jobs(jobs, n_rows, n_out, m):
    """jobs: sequence of (source row of raw, output row, program, params) -> (table (J, VIEW_PROGRAM_JOB_WORDS) int32, noise
    (n_noise, m, 3) float32, mask (n_mask, m) float32) in the record layout of include/geot_hip.h geot_view_program.
    Everything is checked here, on the host."""
    return _pack_jobs(jobs, n_rows, n_out, m, "view_program_views", False)[:3]


def pack_fixed_jobs(jobs, n_rows, n_out, m, views=None, slots=None):
    """jobs: sequence of (source row, output row, program, params or None) in ViewProgram.compile_fixed's layout ->
    (table (J, VIEW_PROGRAM_JOB_WORDS) int32, plans (J, VIEW_DRAW_PLAN_WORDS) int32, noise (n_noise, m, 3), mask (n_mask, m)
    float32): with params None the template table geot_view_draw starts from (noise and mask rows zero), else the records and
    rows these draws give.  views / slots: per job the view of its slot (0 only or labelled, 1 weak, 2 strong) and the slot
    whose draw id it uses; default 0 and the job's number."""
    table, noise, masks, walked = _pack_jobs(jobs, n_rows, n_out, m, "view_draw", True)
    plans = np.zeros((len(jobs), _lib.VIEW_DRAW_PLAN_WORDS), dtype=np.int32)
    plans_f = plans.view(np.float32)
    for j, fixed in enumerate(walked):
        view, slot = (0 if views is None else int(views[j])), (j if slots is None else int(slots[j]))
        need(view in (0, 1, 2) and 0 <= slot < 2 ** 31, "view_draw: a view is 0, 1 or 2, a slot a non-negative int")
        plans[j, :4] = view, slot, len(fixed["steps"]), fixed["store_at"]
        for k, (kind, op, pos, flags, consts) in enumerate(fixed["steps"]):
            at = 8 + 12 * k
            plans[j, at:at + 4] = kind, op, pos, flags
            plans_f[j, at + 4:at + 4 + len(consts)] = np.asarray(consts, dtype=np.float32)
    return table, plans, noise, masks


def view_program_views(raw, jobs, n_out=None, packed=None):
    """raw (S, m, 3) CUDA float32; jobs: sequence of (source row, output row, program, params) with params from
    program.draw(m) -> dict(pos (n_out, m, 3), x (n_out, 3, m), heights (n_out, m, 1) or None when no job's list has a
    PointCloudCenterAndNormalize, view_center (J, 3), view_scale (J,)); n_out defaults to len(jobs).  The counterpart of
    fixmatch_views: one launch, one pinned staging buffer and one host-to-device copy, no host synchronisation.  Rows of the
    outputs no job names stay uninitialised, and so do the heights rows of jobs whose list makes none.  packed: what
    pack_program_jobs made of these very jobs, when the caller has already checked them that way."""
    raw = f32(raw, "raw", 3)
    need(raw.shape[2] == 3 and raw.shape[0] >= 1 and raw.shape[1] >= 1, "raw must be (S>=1, m>=1, 3)")
    rows, m = raw.shape[0], raw.shape[1]
    n_out = len(jobs) if n_out is None else int(n_out)
    table, noise, masks = pack_program_jobs(jobs, rows, n_out, m) if packed is None else packed
    need(table.shape == (len(jobs), _lib.VIEW_PROGRAM_JOB_WORDS) and noise.shape[1:] == (m, 3) and masks.shape[1:] == (m,),
         "view_program_views: packed does not belong to these jobs")
    dev = raw.device
    # one staging buffer: [records | noise rows | mask rows], 32-bit words
    parts = (table.reshape(-1).view(np.float32), noise.reshape(-1), masks.reshape(-1))
    sizes = [p.size for p in parts]
    stage = torch.empty(sum(sizes), dtype=torch.float32, pin_memory=True)
    host = stage.numpy()
    np.concatenate(parts, out=host)
    on_dev = stage.to(dev, non_blocking=True)
    jobs_dev, noise_dev, mask_dev = on_dev[:sizes[0]], on_dev[sizes[0]:sizes[0] + sizes[1]], on_dev[sizes[0] + sizes[1]:]
    heights = any(job[2].has_heights for job in jobs)
    out = {"pos": torch.empty((n_out, m, 3), dtype=torch.float32, device=dev),
           "x": torch.empty((n_out, 3, m), dtype=torch.float32, device=dev),
           "heights": torch.empty((n_out, m, 1), dtype=torch.float32, device=dev) if heights else None,
           "view_center": torch.empty((len(jobs), 3), dtype=torch.float32, device=dev),
           "view_scale": torch.empty(len(jobs), dtype=torch.float32, device=dev)}
    call("geot_view_program", dev, len(jobs), m, rows, n_out, len(noise), len(masks), ptr(raw), stage.data_ptr(), ptr(jobs_dev),
         ptr(noise_dev) if len(noise) else None, ptr(mask_dev) if len(masks) else None, ptr(out["pos"]), ptr(out["x"]),
         ptr(out["heights"]), ptr(out["view_center"]), ptr(out["view_scale"]))
    return out
