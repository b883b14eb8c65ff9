"""FixMatch training batches built on the GPU from scans that already live there -- what the reference's two training
loaders do per item on CPU workers (openpoints/dataset/tooth_semi/tooth_dataset.py:116-206, 308-415, the transform lists of
cfgs/tooth_semi/transformer_finetune_fixmatch_ntm.yaml in openpoints/transforms/point_transformer_gpu.py, default collation
in openpoints/dataset/build.py:128-189) plus the `.cuda()` / `transpose` lines of train.py:442-445, 465-467, 482-486:

    labelled   PointCloudScaling, PointCloudCenterAndNormalize                                            "train"
    weak       PointCloudCenterAndNormalize                                                               "train_w"
    strong     PointCloudScaling_s, PointCloudCenterAndNormalize, PointCloudRotation_s, PointCloudTranslation_s   "train_s"

A batch costs a constant number of launches (geot_cloud_sample_batch: 5, geot_fixmatch_views: 1, one gather of the jaw flags,
three small pinned host-to-device copies) and never synchronises with the host.  By default the random numbers stay on the
host and are drawn with the reference's statements in the reference's order (draw_view_params), so a caller who seeds numpy
and torch as the reference's worker did gets the reference's views.  `draws=DeviceDraws(seed)` moves the one expensive draw,
the np.random.choice of every item, into one more launch (sample_draw.py: geot_sample_draw; not numpy's stream); the view
parameters, a handful of scalars per item, stay host draws unless it is a DeviceDraws(seed, views=True): then one
geot_view_draw launch (view_draw.py) draws them from the slots' own draw ids and every view runs on geot_view_program.

Three things of the reference a user may not expect, all kept:

1. PointCloudRotation_s reads the keyword `angle_s`; the yaml only gives `angle`.  The configured rotation bound is therefore
   [0, 0, 0] and the strong view's R is exactly the identity -- but the three np.random.uniform draws and the
   np.random.shuffle still consume numpy's stream.  Pass kwargs with an `angle_s` entry for real rotations.
2. The dataset sets data['x'] = data['pos'] (the same tensor), PointCloudScaling* scales it in place and
   PointCloudCenterAndNormalize rebinds data['pos']: x / x_s are the SCALED, un-centred clouds, x_w is the sampled cloud.
3. The unlabelled dataset deep-copies the sample before transforming: the un-suffixed pos / x / y / cls / class_weights of
   the unlabelled batch are the untransformed sample; every key of the transformed copies reappears with _w / _s.
"""
import numpy as np
import torch

from ... import _lib
from ...ext._common import call, f32, need, ptr
from .batcher import Batcher
from .sample_draw import DeviceDraws, ViewDrawHandle, draw_batch_sel, on_stream  # noqa: F401  (importable from here, as ever)
from .scan_set import DeviceScanSet, _to_device, cloud_sample_batch, raise_bad_index  # noqa: F401
from .view_program import ViewProgram, _axis_rotation, pack_program_jobs, view_program_views  # noqa: F401

# cfgs/tooth_semi/transformer_finetune_fixmatch_ntm.yaml datatransforms.kwargs, the entries the three lists read.
# `angle` is what the file says (its second entry; a yaml loader keeps the last duplicate) and NOTHING reads it:
# PointCloudRotation_s takes `angle_s`, which is absent -> its default [0, 0, 0] (quirk 1 above).
TOOTH_VIEW_KWARGS = {
    "scale": [0.9, 1.1],
    "gravity_dim": 1,
    "scale_s": [0.8, 1.2],
    "shift_s": [0.2, 0.2, 0.2],
    "angle": [1, 1, 1],
}
KINDS = ("train", "train_w", "train_s")
# the three configured lists as ViewProgram takes them: the same bits as geot_fixmatch_views (tests/test_view_program_gpu.py)
CONFIGURED_LISTS = {"train": ["PointCloudScaling", "PointCloudCenterAndNormalize"],
                    "train_w": ["PointCloudCenterAndNormalize"],
                    "train_s": ["PointCloudScaling_s", "PointCloudCenterAndNormalize", "PointCloudRotation_s",
                                "PointCloudTranslation_s"]}
_DEFAULTS = {"scale": [2. / 3, 3. / 2], "scale_s": [2. / 3, 3. / 2], "shift_s": [0.2, 0.2, 0.], "angle_s": [0, 0, 0],
             "gravity_dim": 2}         # the transform classes' own defaults for absent keywords


def _kw(kwargs, key):
    return kwargs[key] if key in kwargs else _DEFAULTS[key]


def _draw_scale(bounds):
    lo, hi = np.array(bounds).astype(np.float32)
    return (torch.rand(3, dtype=torch.float32) * (hi - lo) + lo).numpy()


def draw_view_params(kind, kwargs=TOOTH_VIEW_KWARGS):
    """The random parameters of one view, drawn on the host from the GLOBAL torch-CPU and numpy generators with the
    reference's statements in the reference's order -> dict(kind, s (3,), R (3,3), t (3,) float32, rotate, translate).

      "train"    s = torch.rand(3) * (hi - lo) + lo over kwargs["scale"]
      "train_w"  nothing is drawn
      "train_s"  s over kwargs["scale_s"]; three np.random.uniform(-b, b) with b = kwargs["angle_s"] * pi (absent: 0, see the
                 module text), one np.random.shuffle of the three axis rotations, R = float32 of their product;
                 t = torch.rand(3) * kwargs["shift_s"]
    """
    need(kind in KINDS, "draw_view_params: kind must be one of %s, got %r" % (KINDS, kind))
    out = {"kind": kind, "s": np.ones(3, np.float32), "R": np.eye(3, dtype=np.float32), "t": np.zeros(3, np.float32),
           "rotate": False, "translate": False}
    if kind == "train":
        out["s"] = _draw_scale(_kw(kwargs, "scale"))
    elif kind == "train_s":
        out["s"] = _draw_scale(_kw(kwargs, "scale_s"))
        mats = []
        for ax, bound in enumerate(np.array(_kw(kwargs, "angle_s")) * np.pi):
            axis = np.zeros(3)
            axis[ax] = 1
            mats.append(_axis_rotation(axis, np.random.uniform(-bound, bound)))
        np.random.shuffle(mats)
        out["R"] = torch.tensor(mats[0] @ mats[1] @ mats[2], dtype=torch.float32).numpy()
        shift = torch.from_numpy(np.array(_kw(kwargs, "shift_s"))).to(torch.float32)
        out["t"] = (torch.rand(3, dtype=torch.float32) * shift).numpy()
        out["rotate"] = out["translate"] = True
    return out


def _check_params(p):
    need(isinstance(p, dict) and all(k in p for k in ("s", "R", "t")), "view parameters: a dict with s, R, t "
         "(draw_view_params)")
    s, r, t = (np.asarray(p[k], dtype=np.float32) for k in ("s", "R", "t"))
    need(s.shape == (3,) and r.shape == (3, 3) and t.shape == (3,), "view parameters: s (3,), R (3,3), t (3,)")
    return s, r, t, bool(p.get("rotate", True)), bool(p.get("translate", True))


def pack_view_jobs(jobs, n_rows, n_out):
    """jobs: sequence of (source row of raw, output row, params) -> (J, VIEW_JOB_WORDS) int32 host array in the record
    layout of include/geot_hip.h geot_fixmatch_views.  Everything is checked here, on the host."""
    need(len(jobs) >= 1, "fixmatch_views: at least one job")
    table = np.zeros((len(jobs), _lib.VIEW_JOB_WORDS), dtype=np.int32)
    as_f = table.view(np.float32)
    seen = set()
    for j, job in enumerate(jobs):
        need(len(job) == 3, "fixmatch_views: a job is (source row, output row, params)")
        src, dst = int(job[0]), int(job[1])
        need(0 <= src < n_rows, "fixmatch_views: job %d reads row %d of %d" % (j, src, n_rows))
        need(0 <= dst < n_out and dst not in seen, "fixmatch_views: job %d writes row %d (of %d; each row once)" % (j, dst, n_out))
        seen.add(dst)
        s, r, t, rot, tr = _check_params(job[2])
        table[j, 0], table[j, 1], table[j, 2] = src, dst, (1 if rot else 0) | (2 if tr else 0)
        as_f[j, 4:7], as_f[j, 7:16], as_f[j, 16:19] = s, r.reshape(9), t
    return table



def fixmatch_views(raw, jobs, gravity_dim=1, n_out=None):
    """raw (S, m, 3) CUDA float32; jobs: sequence of (source row, output row, params) with params from draw_view_params (or
    any dict with s, R, t and optionally rotate / translate, default True) -> dict(pos (n_out, m, 3), x (n_out, 3, m),
    heights (n_out, m, 1), view_center (J, 3), view_scale (J,)); n_out defaults to len(jobs).  One launch, no host
    synchronisation; rows of the outputs no job names stay uninitialised."""
    raw = f32(raw, "raw", 3)
    need(raw.shape[2] == 3 and raw.shape[0] >= 1 and raw.shape[1] >= 1, "raw must be (S>=1, m>=1, 3)")
    need(gravity_dim in (0, 1, 2), "gravity_dim must be 0, 1 or 2")
    rows, m = raw.shape[0], raw.shape[1]
    n_out = len(jobs) if n_out is None else int(n_out)
    table = pack_view_jobs(jobs, rows, n_out)
    dev = raw.device
    out = {"pos": torch.empty((n_out, m, 3), dtype=torch.float32, device=dev),
           "x": torch.empty((n_out, 3, m), dtype=torch.float32, device=dev),
           "heights": torch.empty((n_out, m, 1), dtype=torch.float32, device=dev),
           "view_center": torch.empty((len(jobs), 3), dtype=torch.float32, device=dev),
           "view_scale": torch.empty(len(jobs), dtype=torch.float32, device=dev)}
    jobs_dev = _to_device(table, dev)
    call("geot_fixmatch_views", dev, len(jobs), m, rows, n_out, int(gravity_dim), ptr(raw), ptr(jobs_dev), ptr(out["pos"]),
         ptr(out["x"]), ptr(out["heights"]), ptr(out["view_center"]), ptr(out["view_scale"]))
    return out



class FixMatchBatcher(Batcher):
    """Replaces the reference's two training DataLoaders: `batch(idx_l, idx_u)` returns (data, data_u) with the keys,
    shapes and dtypes train_one_epoch works on after its `.cuda()` and `transpose` lines,

        data    pos (B_l, m, 3)  x (B_l, 3, m)  heights (B_l, m, 1)  y (B_l, m) int64  cls (B_l, 1) int64  class_weights (B_l, C)
        data_u  pos / x / raw_pos (B_u, m, 3)  y (B_u, m)  cls (B_u, 1)  class_weights (B_u, C)     (the untransformed sample)
                pos_w, pos_s (B_u, m, 3)  x_w, x_s (B_u, 3, m)  heights_w, heights_s (B_u, m, 1)  and y / cls / class_weights
                with _w and _s

    in freshly allocated tensors (FixMatchNTMStep's look-ahead matches batches by identity and version).  Keys the reference
    fills with equal values share one tensor here (data_u pos / x / raw_pos; y, cls, class_weights and their _w / _s forms):
    clone before writing into one of them.  The two sets are copied into one concatenated set at construction.

    transforms: None keeps the three configured lists on geot_fixmatch_views.  A dict {"train": [...], "train_w": [...],
    "train_s": [...]} of the reference's transform class names routes every view through geot_view_program instead
    (view_program.ViewProgram; each class reads `kwargs`); params are then ViewProgram.draw results.  The deep-copy quirk
    (3) does not depend on the lists.  Given the configured lists the program kernel produces the hard-wired kernel's bits
    but takes 1.7 times its time at m = 16 000 and 24 000 and 2.1 times at m = 30 000 (a whole batch: 1.2 times;
    profiles/view_program_timing.txt), which is why None keeps the hard-wired kernel.

    stream: queue every batch on that side stream.  A batch depends on the scans alone, so it does NOT wait for what the
    current stream has queued: it runs beside the iteration in flight.  Call `batcher.join(data, data_u)` before the
    current stream (or a step: `next_batches=`) reads the tensors; the wait it queues sits behind the running iteration
    and costs that iteration nothing.

    draws: None keeps the reference's per-item np.random.choice on the host (numpy's global stream, milliseconds per item).
    A sample_draw.DeviceDraws draws every slot's vertex sample in one geot_sample_draw launch on the batcher's stream
    instead -- one draw id per slot, the labelled slots first -- and np.random.choice is not called; given here it serves
    every batch, given to batch() / draw() that call.  Explicit sel_l / sel_u rows still win.
    With DeviceDraws(seed, views=True) the view parameters are device draws too (geot_view_draw, from the slot's own draw
    id: view 0 labelled, 1 weak, 2 strong), no host generator is read, and with transforms=None the three configured lists
    run as ViewPrograms, which give the bits of geot_fixmatch_views.  draw() then returns a ViewDrawHandle in place of the
    parameters, batch(params=handle) replays it, and explicit params= still win.

    curvatures=True: data and data_u each hold "curvatures" (Batcher's class text); both sets must hold their curvature, of one
    radius, BEFORE the batcher is built (it copies the two sets into one), or call batcher.scans.compute_curvature().
    """

    programs = None          # kind -> ViewProgram when `transforms` routes the views through geot_view_program

    def __init__(self, labelled, unlabelled, num_points, num_classes=17, kwargs=TOOTH_VIEW_KWARGS, stream=None, transforms=None,
                 draws=None, curvatures=False):
        need(isinstance(labelled, DeviceScanSet) and isinstance(unlabelled, DeviceScanSet),
             "FixMatchBatcher: labelled and unlabelled must be DeviceScanSets")
        need(int(_kw(kwargs, "gravity_dim")) in (0, 1, 2), "FixMatchBatcher: gravity_dim must be 0, 1 or 2")
        self.n_l, self.n_u, self.kwargs = len(labelled), len(unlabelled), kwargs
        if transforms is not None:
            need(isinstance(transforms, dict) and set(transforms) == set(KINDS),
                 "FixMatchBatcher: transforms is a dict with the lists %s" % (KINDS,))
            self.programs = {kind: ViewProgram(transforms[kind], kwargs) for kind in KINDS}
            need(all(p.has_heights for p in self.programs.values()),
                 "FixMatchBatcher: every list needs a PointCloudCenterAndNormalize (heights is a feature key)")
        self._draw_programs = self.programs      # the lists device view draws run on (None: built when first needed)
        super().__init__(DeviceScanSet._merged(labelled, unlabelled), num_points, num_classes, stream, draws, curvatures)

    def _add_curvatures(self, out, cur, bl, bu):
        """data's and data_u's: the weak and the strong view of an unlabelled item share its sample, so data_u gets one tensor."""
        out[0]["curvatures"], out[1]["curvatures"] = cur[:bl], cur[bl:bl + bu]

    def _draw_view(self, kind):
        return draw_view_params(kind, self.kwargs) if self.programs is None else self.programs[kind].draw(self.m)

    def draw(self, idx_l, idx_u, sel_l=None, sel_u=None, params=None, draws=None):
        """The host half of batch(): (sel (B_l + B_u, m) int64, params) with everything not given drawn in the reference's
        per-item order -- per labelled item np.random.choice then the "train" draw, per unlabelled item np.random.choice then
        "train_w" (draws nothing) and "train_s".  params: list of B_l dicts followed by B_u (weak, strong) pairs.
        With draws (a DeviceDraws; default: the constructor's) the rows not given are drawn by geot_sample_draw, queued on
        the batcher's stream, and sel is that (B_l + B_u, m) int64 DEVICE tensor; only the view parameters are host draws."""
        return self._draw_slots(idx_l, idx_u, sel_l, sel_u, params, draws)[:2]

    def _draw_slots(self, idx_l, idx_u, sel_l, sel_u, params, draws):
        """draw() and, third, the scan ids on the device when the device drew (None otherwise)."""
        bl, bu = len(idx_l), len(idx_u)
        if params is not None and not isinstance(params, ViewDrawHandle):
            need(len(params) == bl + bu and all(len(p) == 2 for p in params[bl:]),
                 "params: %d labelled dicts followed by %d (weak, strong) pairs" % (bl, bu))
        ids = [int(i) for i in idx_l] + [self.n_l + int(i) for i in idx_u]
        return self._draw(ids, (("sel_l", sel_l, bl), ("sel_u", sel_u, bu)), params, draws, lambda slot: self._draw_view(
            "train") if slot < bl else (self._draw_view("train_w"), self._draw_view("train_s")))

    @staticmethod
    def _rows(bl, bu):
        """(source row, output row, list) per view job: output rows [0, B_l) labelled, [B_l, B_l + B_u) weak, then strong."""
        rows = [(i, i, "train") for i in range(bl)] + [(bl + i, bl + i, "train_w") for i in range(bu)]
        return rows + [(bl + i, bl + bu + i, "train_s") for i in range(bu)]

    def _jobs(self, bl, bu):
        """A slot's two views draw under the slot's id as views 1 and 2."""
        if self._draw_programs is None:           # the configured lists as programs: the bits of geot_fixmatch_views
            self._draw_programs = {k: ViewProgram(CONFIGURED_LISTS[k], self.kwargs) for k in KINDS}
        jobs = [(src, dst, self._draw_programs[kind]) for src, dst, kind in self._rows(bl, bu)]
        return jobs, bl + bu, bl + 2 * bu, [0] * bl + [1] * bu + [2] * bu, list(range(bl)) + 2 * list(range(bl, bl + bu))

    def _pack(self, shape, params):
        if self.programs is not None:
            return super()._pack(shape, params)
        bl, bu = shape
        jobs = [(src, dst, p) for (src, dst, _), p in zip(self._rows(bl, bu), params)]
        pack_view_jobs(jobs, bl + bu, bl + 2 * bu)        # checks the parameters before anything is queued
        return jobs, bl + 2 * bu, None

    def _views(self, raw, packed):
        if self.programs is not None:
            return super()._views(raw, packed)
        return fixmatch_views(raw, packed[0], int(_kw(self.kwargs, "gravity_dim")), packed[1])

    def batch(self, idx_l, idx_u, sel_l=None, sel_u=None, params=None, check=False, draws=None):
        """idx_l / idx_u: scan numbers within the labelled / unlabelled set (what the samplers would yield); sel_* (B, m)
        vertex indices per scan and params (see draw()) default to the reference's draws; draws: a DeviceDraws for this
        call (default: the constructor's; see the class text).  check=True reads the bad-index flags back (one host sync)
        and raises IndexError."""
        idx_l, idx_u = [int(i) for i in idx_l], [int(i) for i in idx_u]
        bl, bu = len(idx_l), len(idx_u)
        need(bl >= 1 and bu >= 1, "FixMatchBatcher.batch: at least one labelled and one unlabelled scan")
        need(all(0 <= i < self.n_l for i in idx_l), "idx_l must lie in [0, %d)" % self.n_l)
        need(all(0 <= i < self.n_u for i in idx_u), "idx_u must lie in [0, %d)" % self.n_u)
        sel, params, ids_dev = self._draw_slots(idx_l, idx_u, sel_l, sel_u, params, draws)
        if not isinstance(params, ViewDrawHandle):        # per job: the labelled views, the weak ones, the strong ones
            params = params[:bl] + [p[0] for p in params[bl:]] + [p[1] for p in params[bl:]]
        return self._batch(idx_l + [self.n_l + i for i in idx_u], (bl, bu), sel, params, ids_dev, check)

    def _result(self, s, v, cls, ids, bl, bu):
        lab, unl = slice(0, bl), slice(bl, bl + bu)
        data = {"pos": v["pos"][:bl], "x": v["x"][:bl], "heights": v["heights"][:bl], "y": s["y"][lab], "cls": cls[lab],
                "class_weights": s["class_weights"][lab]}
        raw_u = s["raw"][unl]
        data_u = {"pos": raw_u, "x": raw_u, "raw_pos": raw_u}
        for suffix in ("", "_w", "_s"):
            data_u["y" + suffix], data_u["cls" + suffix] = s["y"][unl], cls[unl]
            data_u["class_weights" + suffix] = s["class_weights"][unl]
        for suffix, rows in (("_w", slice(bl, bl + bu)), ("_s", slice(bl + bu, bl + 2 * bu))):
            for key in ("pos", "x", "heights"):
                data_u[key + suffix] = v[key][rows]
        return data, data_u

    def join(self, data, data_u):
        """Hand a batch built on the side stream to the CURRENT stream (Batcher._join)."""
        self._join(list(data.values()) + list(data_u.values()))
