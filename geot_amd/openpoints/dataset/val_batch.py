"""Validation batches built on the GPU from scans that already live there -- what the reference's validation loader does
per item on CPU workers and in its collation (openpoints/dataset/tooth_semi/tooth_dataset.py:116-188 for split in ['val',
'test'], the `val` list [PointsToTensor, PointCloudCenterAndNormalize] of cfgs/tooth_semi/transformer_finetune_fixmatch_ntm.yaml,
openpoints/dataset/build.py:30-50 collate_fn_val) plus validate's `.cuda()` and `transpose` lines (train.py:731-739):

    pos (B, m, 3)   x (B, 3, m)   y (B, m) int64   cls (B, 1) int64   center (B, 3)   scale (B,)
    points / labels   lists of B views into the set's vertices (N_i, 3) fp32 and labels (N_i,) int32: nothing is copied
    scan_ids (B,) int64 on the device, scans (the set), sizes (the B vertex counts) and mandible (validate's `cls[ii] == 0`)
    as host values; for a set that holds faces or keeps neighbour tables (DeviceScanSet(faces=), keep_tables()) also ids, the
    scan numbers as host values: what validation.mesh_neighbours and the set's table cache go by

The `val` list is the weak view's list: geot_cloud_sample_batch (5 launches) and geot_fixmatch_views with the "train_w"
parameters (1), one gather of the jaw classes, two small pinned host-to-device copies -- the same number for every batch,
and no host synchronisation.  With `draws=DeviceDraws(seed)` the per-item np.random.choice becomes one geot_sample_draw launch
in front of them (sample_draw.py; not numpy's stream).  validation.SegMetrics.update_from_scans / predict_scans / validate_scans take such a batch; it
also carries every key the existing validate() and get_pred_whole() read.

One thing of the reference a user may not expect, kept: the dataset's pc_norm centres and scales the scan (`center`,
`scale`), the sampled points then go through PointCloudCenterAndNormalize, which centres and scales the SAMPLE once more
(x stays the sampled cloud: data['x'] is data['pos'] until the transform rebinds pos) -- and get_pred_whole de-normalises
`pos` with pc_norm's center and scale alone (`point * s + c`).  The sampled points it searches are therefore not exactly
on the scan.  validation.py reproduces that statement for statement.
"""
import numpy as np
import torch

from ...ext._common import need
from .batcher import Batcher
from .fixmatch_batch import TOOTH_VIEW_KWARGS, _kw, draw_view_params, fixmatch_views
from .sample_draw import DeviceDraws, cover_passes, on_stream, sample_draw_cover
from .scan_set import check_curvature


def draw_val_sel(sizes, num_points):
    """The host half of a batch: per item exactly one np.random.choice(N_i, m, replace=N_i < m) from numpy's GLOBAL
    generator (tooth_dataset.py:134-135), in item order; the `val` transform list draws nothing -> (B, m) int64."""
    m = int(num_points)
    need(m >= 1, "draw_val_sel: num_points >= 1")
    sel = np.empty((len(sizes), m), dtype=np.int64)
    for slot, n in enumerate(sizes):
        n = int(n)
        need(n >= 1, "draw_val_sel: a scan has at least one vertex")
        replace = False if n >= m else True
        sel[slot] = np.random.choice(n, m, replace=replace)
    return sel


class ScanBatcher(Batcher):
    """What the batchers of whole scans (ValBatcher, vote_batch.VoteBatcher) share: the jaw classes, read from the device once,
    here; the zero-copy views of every scan's vertices and labels; the idx checks; the keys of a batch that describe its scans;
    `join` over the class's tensor keys."""

    join_keys = ("pos", "x", "y", "cls", "center", "scale", "scan_ids")

    def __init__(self, scans, num_points, num_classes, kwargs, stream, draws, curvatures=False):
        super().__init__(scans, num_points, num_classes, stream, draws, curvatures)
        self.kwargs = kwargs
        self.cls_host = [int(v) for v in scans.cls.cpu().tolist()]       # the one copy: validate's `cls[ii] == 0` per scan
        self._points = list(torch.split(scans.points, scans.sizes))      # views
        self._labels = list(torch.split(scans.labels, scans.sizes))

    def __len__(self):
        return len(self.scans)

    def _ids(self, idx):
        ids, who = [int(i) for i in idx], type(self).__name__
        need(len(ids) >= 1, "%s.batch: at least one scan" % who)
        need(all(0 <= i < len(self.scans) for i in ids), "%s.batch: idx must lie in [0, %d)" % (who, len(self.scans)))
        return ids

    def _scan_keys(self, s, cls, ids):
        """Every key of a batch but the views' (pos, x, ...)."""
        keys = {"y": s["y"], "cls": cls, "center": s["center"], "scale": s["scale"],
                "points": [self._points[i] for i in ids], "labels": [self._labels[i] for i in ids],
                "scan_ids": s["scan_ids"], "scans": self.scans, "sizes": [self.scans.sizes[i] for i in ids],
                "mandible": [self.cls_host[i] == 0 for i in ids]}
        if getattr(self.scans, "faces", None) is not None or getattr(self.scans, "_keep", False):
            keys["ids"] = list(ids)         # only where something goes by them: a set without meshes and tables keeps its key set
        return keys

    def join(self, batch):
        """Hand a batch built on the side stream to the CURRENT stream (Batcher._join)."""
        self._join(batch[key] for key in self.join_keys + tuple(k for k in ("sel", "view_center", "view_scale", "curvatures") if k in batch))

    def _affine(self, v, b):
        """The `val` view's centre-and-normalise of every slot, as the views launch wrote it: pos = (raw - view_center) /
        view_scale per coordinate (for a VoteBatcher: pos_search).  With pc_norm's center / scale in front it takes ANY vertex
        of the slot's scan to the model's coordinates (validation.decode_scans, geot_scan_decode_front)."""
        return {"view_center": v["view_center"][:b], "view_scale": v["view_scale"][:b]}

    def cover(self, idx, rounds=1, draws=None):
        """The covering batches of the scans `idx`: a generator of rounds * P batches, P = cover_passes(their sizes, m), per
        round in pass order.  Each is what batch() returns for the same idx plus "sel" -- the (B, m) int64 device tensor of the
        pass's vertex indices (geot_sample_draw_cover) -- and "cover" = (pass, P, round).  The samples of a round's P passes
        partition every scan: each vertex is sample j of exactly one pass with pass * m + j < its scan's size (the positions
        past that are wrap-around fill, which keeps every cloud at m points); validation.ScanCover puts the model's output
        for a sample on the vertex it names.
        draws: a DeviceDraws (default: the constructor's) -- there is no host-draw form, ValueError without one, before any
        device call.  len(idx) draw ids are taken once per round, when the round's first batch is built; a slot keeps its id
        for all P passes, so the counter advances by len(idx) * rounds over the whole generator.  Under
        DeviceDraws(views=True) a VoteBatcher's vote parameters are drawn from the slot's id as in batch(): one view per round,
        shared by its passes; otherwise the vote list draws on the host per pass, as in batch()."""
        ids, who = self._ids(idx), type(self).__name__
        draws = self.draws if draws is None else draws
        if self.curvatures:
            check_curvature(self.scans, ids, who)
        if not isinstance(draws, DeviceDraws):
            raise ValueError("%s.cover: a covering draw is a device draw -- pass draws=DeviceDraws(seed) here or to the "
                             "constructor (there is no host-draw form), got %r" % (who, draws))
        if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)) or int(rounds) < 1:
            raise ValueError("%s.cover: rounds must be an int >= 1, got %r" % (who, rounds))
        return self._cover(ids, int(rounds), draws)

    def _cover(self, ids, rounds, draws):
        passes = cover_passes([self.scans.sizes[i] for i in ids], self.m)
        ids_dev = None
        for rnd in range(rounds):
            base = draws.take(len(ids))
            for p in range(passes):
                with on_stream(self.stream):
                    if ids_dev is None:
                        ids_dev = torch.from_numpy(np.asarray(ids, dtype=np.int64)).pin_memory().to(self.device, non_blocking=True)
                    sel, _ = sample_draw_cover(self.scans, ids_dev, self.m, draws.seed, base, p)
                out = self._batch(ids, (len(ids),), sel, self._cover_params(ids, draws, base), ids_dev, False)
                out["sel"], out["cover"] = sel, (p, passes, rnd)
                yield out


class ValBatcher(ScanBatcher):
    """Replaces the reference's validation DataLoader: `batch(idx)` returns the dict described in the module text for the
    scans `idx` of the set (what the sequential sampler would yield), in freshly allocated tensors.

    The jaw classes are read from the device once, here.  stream: queue every batch on that side stream; it depends on
    the scans alone, so it runs beside whatever the current stream has in flight.  Call `join(batch)` before the current
    stream reads the tensors.

    draws: None keeps the reference's np.random.choice per item on the host (draw_val_sel); a sample_draw.DeviceDraws draws
    the vertex samples of a batch in one geot_sample_draw launch on the batcher's stream (one draw id per slot) and
    np.random.choice is not called.  Given here it serves every batch, given to batch() that call; sel= still wins.
    DeviceDraws(seed, views=True) is accepted and changes nothing: the `val` list draws no view parameter.

    curvatures=True adds "curvatures" (B, m) float32 to every batch, the covering ones too (Batcher's class text)."""

    def __init__(self, scans, num_points, num_classes=17, kwargs=TOOTH_VIEW_KWARGS, stream=None, draws=None, curvatures=False):
        super().__init__(scans, num_points, num_classes, kwargs, stream, draws, curvatures)
        need(int(_kw(kwargs, "gravity_dim")) in (0, 1, 2), "ValBatcher: gravity_dim must be 0, 1 or 2")

    def batch(self, idx, sel=None, check=False, draws=None, affine=False):
        """idx: scan numbers within the set; sel (B, m) vertex indices per scan, default the reference's draws
        (draw_val_sel's statements) or, with draws (a DeviceDraws; default: the constructor's), geot_sample_draw's.
        check=True reads the bad-index flags back (one host sync) and raises IndexError.  affine=True adds the slots' view
        affine (ScanBatcher._affine): view_center (B, 3), view_scale (B,); the default key set is unchanged."""
        ids = self._ids(idx)
        weak = draw_view_params("train_w", self.kwargs)                   # the `val` list: nothing is drawn
        sel, params, ids_dev = self._draw(ids, (("sel", sel, len(ids)),), [weak] * len(ids), draws, None)
        return self._batch(ids, (len(ids),), sel, params, ids_dev, check, affine)

    def _cover_params(self, ids, draws, base):
        return [draw_view_params("train_w", self.kwargs)] * len(ids)    # as batch(): the `val` list draws nothing

    def _pack(self, shape, params):
        return [(i, i, p) for i, p in enumerate(params)]

    def _views(self, raw, jobs):
        return fixmatch_views(raw, jobs, int(_kw(self.kwargs, "gravity_dim")), len(jobs))

    def _result(self, s, v, cls, ids, b):
        return {"pos": v["pos"], "x": v["x"], **self._scan_keys(s, cls, ids)}
