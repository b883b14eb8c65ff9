"""The validation path of examples/segmentation/train.py:716-832.

``get_pred_whole`` (:781-800): per scan, de-normalise the N sampled points, take the 3 nearest sampled points of every
full-resolution vertex, inverse-distance interpolate the class probabilities and arg-max.  Same kernels as the training
path (three_nn / three_interpolate) at m ~ 1e5 unknown vertices; scans keep their own vertex counts, so the loop over
scans stays (each launch already fills the GPU).

``get_seg_metrics`` (:802-832), ``validate`` (:716-779) and ``SegMetrics``: the reference's per-scan accuracy, mIoU and
DSC and their jaw and whole means, from integer counts made on the device (csrc/seg_metrics.hip):

    metrics = SegMetrics(num_classes, device)
    for data in val_loader:                                  # collate_fn_val batches
        ...
        metrics.update_from_logits(logits, data["pos"], data["points"], data["center"], data["scale"], data["labels"], cls)
    out = metrics.read()                                     # one device-to-host copy: out["whole_miou"], out["miou_list"], ...
    metrics.reset()                                          # the next epoch

update_from_logits runs get_pred_whole's soft-max and three_nn, then interpolates, arg-maxes and counts in one launch per
batch: no (C, M) probabilities, no per-vertex prediction, no host synchronisation.  read() executes the reference's torch /
numpy statements on CPU int64 tensors built from the counts, so every value, NaN and dtype is the reference's.
"""
import logging

import numpy as np
import torch
import torch.nn.functional as F

from .ext._common import call, knn_workspace, need, ptr
from .pointnet2 import pointnet2_utils as pt_utils

MAX_VERTICES = (1 << 31) - 1        # per scan (include/geot_hip.h geot_seg_confusion)


@torch.no_grad()
def get_pred_whole(logits, points, points_whole, center, scale):
    """logits (B,C,N); points (B,N,3) normalised; points_whole: list of (M_i,3); center/scale: per-scan
    tensors broadcastable to (1,N,3) -> list of (1, M_i) int64 predicted labels."""
    logits = F.softmax(logits, dim=1)
    dev = logits.device
    preds_whole = []
    for index in range(logits.shape[0]):
        logit = logits[index].unsqueeze(0).contiguous()
        point = points[index].unsqueeze(0).contiguous()
        s = torch.as_tensor(scale[index]).to(dev).unsqueeze(0).contiguous()
        c = torch.as_tensor(center[index]).to(dev).unsqueeze(0).contiguous()
        point_whole = torch.as_tensor(points_whole[index]).to(dev).unsqueeze(0).contiguous()
        point = (point * s + c).contiguous()
        dist, idx = pt_utils.three_nn(point_whole.float(), point.float())
        dist_recip = 1.0 / (dist + 1e-8)
        weight = dist_recip / torch.sum(dist_recip, dim=2, keepdim=True)
        logit_whole = pt_utils.three_interpolate(logit, idx, weight)
        preds_whole.append(logit_whole.argmax(dim=1))
    return preds_whole


def seg_metrics_from_counts(counts, num_classes, mandible):
    """read()'s host half (no device needed): counts (S, C (C + 1) + 1) int64 laid out as geot_seg_confusion writes them,
    mandible (S,) the jaw of every scan (validate's `cls[ii] == 0`) -> the dict SegMetrics.read() returns.  The reference's
    statements run on CPU int64 tensors made from the counts: get_seg_metrics (train.py:811-830) per scan, validate's
    aggregation (:747-763).  A label outside [0, C) raises: the reference's result would depend on how many distinct
    such values there were, which the counts do not keep."""
    c = int(num_classes)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, c * (c + 1) + 1)
    need(len(mandible) == counts.shape[0], "SegMetrics: %d jaw flags for %d scans" % (len(mandible), counts.shape[0]))
    bad = int(counts[:, -1].sum())
    if bad:
        raise RuntimeError("SegMetrics: %d labels outside [0, %d) this epoch" % (bad, c))
    acc_list, miou_list, mdsc_list = [], [], []
    for row in counts:
        conf = row[:-1].reshape(c, c + 1)           # (label, prediction); column c = prediction outside [0, C)
        n_label, n_pred, hit = conf.sum(1), conf[:, :c].sum(0), np.diagonal(conf)
        iou, dsc = [], []
        for jcls in range(1, c):                    # torch.unique(label) in ascending order, class 0 skipped
            if n_label[jcls] == 0:
                continue
            jcls_and = torch.tensor(int(hit[jcls]))
            jcls_or = torch.tensor(int(n_pred[jcls] + n_label[jcls] - hit[jcls]))
            iou.append((jcls_and / jcls_or).float())
            dsc.append((2 * iou[-1] / (1 + iou[-1])))
        acc = torch.tensor(int(hit.sum())) / int(n_label.sum())
        acc_list.append(acc)
        miou_list.append(np.array(iou).mean())
        mdsc_list.append(np.array(dsc).mean())
    out = dict(acc_list=acc_list, miou_list=miou_list, mdsc_list=mdsc_list, scans=len(acc_list), labels_out_of_range=bad)
    jaws = {}
    for jaw, lower in (("mandible", True), ("maxillary", False)):
        sel = [i for i, m in enumerate(mandible) if bool(m) == lower]
        jaws[jaw] = {k: [lst[i] for i in sel] for k, lst in (("acc", acc_list), ("miou", miou_list), ("dsc", mdsc_list))}
        out[jaw + "_macc"] = np.array(jaws[jaw]["acc"]).mean()
        out[jaw + "_miou"] = np.array(jaws[jaw]["miou"]).mean()
        out[jaw + "_mdsc"] = np.array(jaws[jaw]["dsc"]).mean()
    lo, up = jaws["mandible"], jaws["maxillary"]
    for key, name in (("acc", "whole_macc"), ("miou", "whole_miou"), ("dsc", "whole_mdsc")):
        out[name] = (np.array(lo[key]).sum() + np.array(up[key]).sum()) / (len(lo[key]) + len(up[key]))
    return out


def _mandible_flags(cls, b):
    """validate's `cls[ii] == 0` for the b scans of a batch, on the host (a device tensor costs one copy here)."""
    if torch.is_tensor(cls):
        cls = cls.detach().cpu()
    need(len(cls) == b, "SegMetrics: %d jaw classes (cls) for %d scans" % (len(cls), b))
    return [bool(cls[i] == 0) for i in range(b)]


class SegMetrics:
    """The validation metrics of one epoch, counted on the device: a (scans, C (C + 1) + 1) int64 buffer (its capacity
    doubles as scans arrive) and each scan's jaw, kept on the host.  Neither update synchronises with the host."""

    def __init__(self, num_classes, device):
        c = int(num_classes)
        need(1 <= c <= 32, "SegMetrics: 1..32 classes (include/geot_hip.h GEOT_NTM_MAX_C), got %d" % c)
        dev = torch.device(device)
        need(dev.type == "cuda", "SegMetrics: the counts live on a GPU, got device %s" % dev)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.c, self.slots, self.device = c, c * (c + 1) + 1, dev
        self.counts = torch.zeros((8, self.slots), dtype=torch.int64, device=dev)
        self.mandible = []

    @property
    def scans(self):
        return len(self.mandible)

    def reset(self):
        """A new epoch."""
        self.counts.zero_()
        self.mandible = []

    def _rows(self, b):
        """The (zero) count rows of the next b scans."""
        n0 = self.scans
        if n0 + b > self.counts.shape[0]:
            grown = torch.zeros((max(n0 + b, 2 * self.counts.shape[0]), self.slots), dtype=torch.int64, device=self.device)
            grown[:n0].copy_(self.counts[:n0])
            self.counts = grown
        return self.counts[n0:n0 + b]

    def _offsets(self, sizes):
        """(b + 1) int64 on the device; the caller keeps the tensor until its launch is queued."""
        for m in sizes:
            need(m <= MAX_VERTICES, "SegMetrics: %d vertices in one scan, at most %d" % (m, MAX_VERTICES))
        offs = torch.tensor(np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]), dtype=torch.int64)
        return offs.pin_memory().to(self.device, non_blocking=True)      # no synchronisation

    def _labels(self, labels_whole):
        labels = [torch.as_tensor(l).reshape(-1) for l in labels_whole]
        need(all(not l.is_floating_point() for l in labels), "SegMetrics: integer labels")
        return torch.cat([l.to(self.device, torch.int64) for l in labels]), [l.numel() for l in labels]

    def update(self, preds_whole, labels_whole, cls):
        """Count one batch from predictions: preds_whole / labels_whole lists of the b scans' per-vertex predictions (e.g.
        get_pred_whole's (1, M_i)) and labels (M_i,); cls the b jaw classes (0 = mandible), as the loader hands them over."""
        b = len(preds_whole)
        need(len(labels_whole) == b, "SegMetrics.update: %d prediction and %d label tensors" % (b, len(labels_whole)))
        flags = _mandible_flags(cls, b)
        if b == 0:
            return
        preds = [torch.as_tensor(p).reshape(-1) for p in preds_whole]
        need(all(not p.is_floating_point() for p in preds), "SegMetrics.update: integer predictions")
        label, sizes = self._labels(labels_whole)
        need([p.numel() for p in preds] == sizes, "SegMetrics.update: every scan needs one prediction per vertex")
        rows = self._rows(b)
        if sum(sizes):
            pred = torch.cat([p.to(self.device, torch.int64) for p in preds])
            offs = self._offsets(sizes)
            call("geot_seg_confusion", self.device, b, self.c, ptr(offs), ptr(pred), ptr(label), ptr(rows))
        self.mandible += flags

    def update_from_logits(self, logits, points, points_whole, center, scale, labels_whole, cls):
        """Count one batch from the model's logits (B, C, N) with get_pred_whole's arguments (points (B, N, 3) normalised,
        points_whole / center / scale per scan) plus the scans' labels and jaw classes: get_pred_whole's soft-max,
        de-normalisation and three_nn, then one launch that interpolates, arg-maxes and counts."""
        need(torch.is_tensor(logits) and logits.dim() == 3 and logits.shape[1] == self.c and logits.dtype == torch.float32,
             "SegMetrics.update_from_logits: fp32 logits (B, %d, N)" % self.c)
        need(logits.device == self.device, "SegMetrics.update_from_logits: logits on %s, the counts on %s" %
             (logits.device, self.device))
        b, _, n = logits.shape
        need(len(points_whole) == b and len(center) == b and len(scale) == b and len(labels_whole) == b,
             "SegMetrics.update_from_logits: one points_whole / center / scale / labels entry per scan")
        need(tuple(points.shape) == (b, n, 3), "SegMetrics.update_from_logits: points must be (B, N, 3)")
        flags = _mandible_flags(cls, b)
        if b == 0:
            return
        dev = self.device
        prob = F.softmax(logits, dim=1).contiguous()
        label, sizes = self._labels(labels_whole)
        total = sum(sizes)
        idx = torch.empty((total, 3), dtype=torch.int32, device=dev)
        dist2 = torch.empty((total, 3), dtype=torch.float32, device=dev)
        at = 0
        for index in range(b):
            # get_pred_whole's three_nn inputs, statement for statement; its output goes into this scan's slice
            point = points[index].unsqueeze(0).contiguous()
            s = torch.as_tensor(scale[index]).to(dev).unsqueeze(0).contiguous()
            c = torch.as_tensor(center[index]).to(dev).unsqueeze(0).contiguous()
            point_whole = torch.as_tensor(points_whole[index]).to(dev).unsqueeze(0).contiguous()
            point = (point * s + c).contiguous()
            unknown, known = point_whole.float().contiguous(), point.float().contiguous()
            m = unknown.shape[1]
            need(unknown.dim() == 3 and unknown.shape[2] == 3 and m == sizes[index],
                 "SegMetrics.update_from_logits: scan %d has %d labels for %s vertices" % (index, sizes[index],
                                                                                           tuple(point_whole.shape[1:])))
            if m:
                wp, wb, _keep = knn_workspace(dev, 1, m, n, 3)
                call("geot_three_nn_ws", dev, 1, m, n, ptr(unknown), ptr(known), ptr(dist2) + 12 * at, ptr(idx) + 12 * at,
                     wp, wb)
            at += m
        rows = self._rows(b)
        if total:
            offs = self._offsets(sizes)
            call("geot_seg_confusion_interp", dev, b, self.c, n, ptr(offs), ptr(prob), ptr(idx), ptr(dist2), ptr(label),
                 ptr(rows))
        self.mandible += flags

    def read(self):
        """The epoch so far, in one device-to-host copy: per scan "acc_list" (0-d fp32 tensors), "miou_list" / "mdsc_list"
        (numpy scalars: float32, or a float64 NaN for a scan with no label but 0), as get_seg_metrics returns them; per jaw
        and whole "mandible_macc" ... "whole_mdsc" as validate computes them; "scans", "labels_out_of_range".  Raises
        RuntimeError if a label outside [0, C) was seen."""
        return seg_metrics_from_counts(self.counts[:self.scans].cpu().numpy(), self.c, self.mandible)


@torch.no_grad()
def get_seg_metrics(preds_whole, labels_whole, num_classes=17):
    """train.py:802-832: (acc_list, miou_list, mdsc_list) of the scans, the reference's values and types."""
    p0 = preds_whole[0] if len(preds_whole) else None
    dev = p0.device if torch.is_tensor(p0) and p0.is_cuda else torch.device("cuda", torch.cuda.current_device())
    metrics = SegMetrics(num_classes, dev)
    metrics.update(preds_whole, labels_whole, [0] * len(preds_whole))
    out = metrics.read()
    return out["acc_list"], out["miou_list"], out["mdsc_list"]


def _cfg(cfg, key, default=None):
    return getattr(cfg, key) if hasattr(cfg, key) else (cfg.get(key, default) if hasattr(cfg, "get") else default)


@torch.no_grad()
def validate(model, val_loader, cfg, num_votes=0, data_transform=None):
    """train.py:716-779 over collate_fn_val batches (openpoints/dataset/build.py:30-50) -> (whole_macc, whole_miou,
    whole_mdsc), logging the reference's three lines.  cfg.num_classes (default 17) sizes the counts.  num_votes and
    data_transform are accepted and unused, as in the reference."""
    model.eval()
    metrics = SegMetrics(_cfg(cfg, "num_classes", 17), torch.device("cuda", torch.cuda.current_device()))
    for data in val_loader:
        cls = data["cls"]                  # the loader's CPU tensor: each scan's jaw, read before anything moves
        for key in data.keys():
            if isinstance(data[key], torch.Tensor):
                data[key] = data[key].cuda(non_blocking=True)
        data["x"] = data["x"].transpose(1, 2).contiguous()
        logits, _, _ = model(data)
        metrics.update_from_logits(logits, data["pos"], data["points"], data["center"], data["scale"], data["labels"], cls)
    out = metrics.read()
    epoch = "%s/%s" % (_cfg(cfg, "epoch"), _cfg(cfg, "epochs"))
    with np.printoptions(precision=2, suppress=True):
        logging.info(f"Test Epoch [{epoch}],Mandible mIoU {out['mandible_miou']:.5f}, "
                     f"Mandible DSC {out['mandible_mdsc']:.5f}, Mandible ACC {out['mandible_macc']:.5f}")
        logging.info(f"Test Epoch [{epoch}],Maxillary mIoU {out['maxillary_miou']:.5f}, "
                     f"Maxillary DSC {out['maxillary_mdsc']:.5f}, Maxillary ACC {out['maxillary_macc']:.5f}")
        logging.info(f"Test Epoch [{epoch}],mIoU {out['whole_miou']:.5f}, DSC {out['whole_mdsc']:.5f}, "
                     f"ACC {out['whole_macc']:.5f}")
    return out["whole_macc"], out["whole_miou"], out["whole_mdsc"]
