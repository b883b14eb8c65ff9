"""The epoch statistics of the FixMatch+NTM loop -- what train_one_epoch accumulates per iteration and returns
(examples/segmentation/train.py:599-644, 672-699, 701-715) -- kept on the device.

    step = FixMatchNTMStep(..., meters=True)             # built from the step's cfg, or:
    step = FixMatchNTMStep(..., meters=FixMatchMeters(num_classes, device, batch_size_l=2, batch_size_u=2, threshold=0.0))
    ...                                                  # the epoch's iterations, eager or replayed
    stats, values = step.meters.read()                   # one device-to-host copy; `values` in train_one_epoch's order
    step.meters.reset()                                  # the next epoch

Per iteration two kernels (geot_amd/csrc/meters.hip) and no host synchronisation, so a captured iteration carries them
(the reference pays ~3 C + 10 host round trips for them).  The values equal the reference's AverageMeter averages
bit for bit: the six tensor-valued meters in fp32 as torch computes them on a CUDA tensor, the loss meters and the three
per-class lists in double as Python does (include/geot_hip.h, geot_fixmatch_meters_*).  A pseudo or ground-truth label
outside [0, C) is left out of the per-class counts as in the reference, counted on the device and reported by read().
"""
import warnings

import torch

from . import _lib
from .ext._common import call, need, ptr

# train_one_epoch's return order (train.py:710-715)
RETURN_ORDER = ("train_loss", "train_loss_l", "train_loss_u", "th_percentage", "mean_pseudo_label_acc",
                "mean_pseudo_label_acc_classwise", "mean_th_meter_u_classwise", "mean_th_meter_u_classwise_recall",
                "teacher_acc", "student_acc", "over_th_wobg", "over_acc_wobg", "ema_t", "ema_t_corr",
                "manifold_loss_feat", "insT_identity_loss", "insT_threed_loss")
F32_NAMES = ("th_percentage", "mean_pseudo_label_acc", "teacher_acc", "student_acc", "over_th_wobg", "over_acc_wobg")
LOSS_NAMES = ("train_loss", "train_loss_l", "train_loss_u", "manifold_loss_feat", "insT_identity_loss", "insT_threed_loss")
CLASS_NAMES = ("mean_pseudo_label_acc_classwise", "mean_th_meter_u_classwise", "mean_th_meter_u_classwise_recall")
MAX_POINTS = 1 << 24      # below this many unlabelled points per iteration the reference's fp32 sums of 0 / 1 are exact


class FixMatchMeters:
    def __init__(self, num_classes, device, batch_size_l=2, batch_size_u=2, threshold=0.0, ema_t=None):
        """batch_size_l / batch_size_u: cfg.batch_size_l / cfg.batch_size_u, the `n` of every meter update (train.py:672-690);
        threshold: cfg.threshold (compared in fp32, as logits_u_aug.ge(torch.tensor(threshold)) does); ema_t: the step's
        (C, C) transition buffer, reported by read() (it is updated in place, never rebound; FixMatchNTMStep fills it in
        when it is None)."""
        c = int(num_classes)
        need(1 <= c <= _lib.NTM_MAX_C, "FixMatchMeters: 1..%d classes (include/geot_hip.h GEOT_NTM_MAX_C), got %d" % (_lib.NTM_MAX_C, c))
        self.c = c
        self.n_l, self.n_u = int(batch_size_l), int(batch_size_u)
        self.threshold = float(threshold)
        self.ema_t = ema_t
        dev = torch.device(device)
        need(dev.type == "cuda", "FixMatchMeters: the meters live on a GPU, got device %s" % dev)
        self.counts = torch.zeros(8 + 4 * c, dtype=torch.int32, device=dev)
        self.f32 = torch.zeros(18, dtype=torch.float32, device=dev)
        self.f64 = torch.zeros(18 + 9 * c, dtype=torch.float64, device=dev)
        self.i64 = torch.zeros(5, dtype=torch.int64, device=dev)
        self.ema_t_corr = torch.zeros((c, c), dtype=torch.float32, device=dev)

    def reset(self):
        """A new epoch: every meter back to zero (in place: a captured iteration holds these buffers)."""
        for t in (self.counts, self.f32, self.f64, self.i64):
            t.zero_()

    _BUFFERS = ("counts", "f32", "f64", "i64", "ema_t_corr")

    def state_dict(self):
        """The epoch so far: copies of the five device buffers, made on the current stream (no synchronisation).  ema_t is
        the step's buffer and travels with the step."""
        from . import checkpoint as ck
        ck.refuse_capture("FixMatchMeters")
        return {k: ck.copied(getattr(self, k)) for k in self._BUFFERS}

    def restore(self, r, state, key="meters"):
        """The first half of load_state_dict: check `state` and hand the writes to r (a checkpoint.Restore)."""
        r.keys(state, self._BUFFERS, key)
        for k in self._BUFFERS:
            r.tensor("%s.%s" % (key, k), getattr(self, k), state[k])

    def load_state_dict(self, state):
        """Checked first (ValueError naming the key), then copied into the buffers (a captured iteration holds them)."""
        from . import checkpoint as ck
        r = ck.Restore()
        self.restore(r, state)
        r.commit()

    def update(self, label_u_aug, logits_u_aug, y_u, prob_s, loss, sup, unsup, threed, ema_t_corr=None, feat=None,
               identity=None):
        """One iteration, on the current stream: label_u_aug (B_u, N) int64 pseudo labels, logits_u_aug (B_u, N) fp32 their
        confidence, y_u (B_u, N) or (B_u, N, 1) int64 ground truth (data_u["y"]), prob_s (B_u, C, N) fp32 the student's
        soft-max on the strong view; loss / sup / unsup / threed the iteration's fp32 scalar losses; ema_t_corr (C, C).
        feat / identity: the iteration's weighted feature-space / identity losses when cfg use_feat_loss / use_identity_loss
        are on (LOSS_NAMES[3:5]: manifold_loss_feat, insT_identity_loss; None: 0.0 is metered, as the reference does).
        Every tensor must live on the meters' GPU: anything else is refused before a kernel is launched."""
        dev = self.counts.device
        extra = [(name, s) for name, s in (("feat", feat), ("identity", identity)) if s is not None]
        scalars = (loss, sup, unsup, threed) + tuple(s for _, s in extra)
        named = [("label_u_aug", label_u_aug), ("logits_u_aug", logits_u_aug), ("data_u['y']", y_u), ("prob_s", prob_s),
                 ("loss", loss), ("sup", sup), ("unsup", unsup), ("threed", threed)] + extra
        if ema_t_corr is not None:
            named.append(("ema_t_corr", ema_t_corr))
        for name, t in named:
            need(torch.is_tensor(t), "FixMatchMeters: %s must be a torch.Tensor" % name)
            need(t.device == dev, "FixMatchMeters: %s is on %s, the meters on %s (CPU tensors are not read)" % (name, t.device, dev))
        need(label_u_aug.dim() == 2, "FixMatchMeters: label_u_aug must be (B_u, N), got %s" % (tuple(label_u_aug.shape),))
        b, n = label_u_aug.shape
        need(b * n < MAX_POINTS, "FixMatchMeters: %d unlabelled points per iteration; the reference's fp32 counts are exact "
                                 "below 2^24 only" % (b * n))
        need(label_u_aug.dtype == torch.int64 and y_u.dtype == torch.int64, "FixMatchMeters: int64 labels")
        need(y_u.numel() == b * n and tuple(y_u.shape[:2]) == (b, n) and y_u.dim() in (2, 3),
             "FixMatchMeters: data_u['y'] must be (B_u, N) or (B_u, N, 1), got %s" % (tuple(y_u.shape),))
        need(tuple(logits_u_aug.shape) == (b, n) and logits_u_aug.dtype == torch.float32, "FixMatchMeters: logits_u_aug (B_u, N) fp32")
        need(tuple(prob_s.shape) == (b, self.c, n) and prob_s.dtype == torch.float32, "FixMatchMeters: prob_s (B_u, C, N) fp32")
        need(all(s.numel() == 1 and s.dtype == torch.float32 for s in scalars), "FixMatchMeters: fp32 scalar losses")
        if ema_t_corr is not None:
            need(tuple(ema_t_corr.shape) == (self.c, self.c) and ema_t_corr.dtype == torch.float32, "FixMatchMeters: ema_t_corr (C, C)")
        t, conf, g, p = (x.detach().contiguous() for x in (label_u_aug, logits_u_aug, y_u, prob_s))
        call("geot_fixmatch_meters_count", dev, b, n, self.c, self.threshold, ptr(t), ptr(conf), ptr(g), ptr(p), ptr(self.counts))
        corr = None if ema_t_corr is None else ema_t_corr.detach().contiguous()
        tail = (ptr(corr), ptr(self.counts), ptr(self.f32), ptr(self.f64), ptr(self.i64),
                ptr(self.ema_t_corr) if corr is not None else None)
        four = tuple(ptr(s.detach()) for s in (loss, sup, unsup, threed))
        if extra:       # the six-loss entry point only when one of the two switched losses is given
            call("geot_fixmatch_meters_finalize6", dev, b, n, self.c, self.n_l, self.n_u, *four,
                 ptr(feat.detach()) if feat is not None else None, ptr(identity.detach()) if identity is not None else None, *tail)
        else:
            call("geot_fixmatch_meters_finalize", dev, b, n, self.c, self.n_l, self.n_u, *four, *tail)

    def read(self, strict=False):
        """-> (dict, tuple): the epoch's averages under train_one_epoch's names, plus "val" (the last iteration's values),
        "iterations" and "labels_out_of_range"; the tuple holds the 17 values in train_one_epoch's return order (per-class
        lists as Python lists, ema_t / ema_t_corr as (C, C) tensors).  One synchronising copy.  Labels outside [0, C) seen
        this epoch (an ignore label such as -1 or 255 in data_u["y"]) are left out of every per-class count, as the
        reference leaves them, counted in "labels_out_of_range" and reported with a RuntimeWarning; strict=True raises
        instead."""
        c = self.c
        f32, f64, i64 = self.f32.cpu(), self.f64.cpu(), self.i64.cpu()
        bad, iters = int(i64[3]), int(i64[4])
        if bad:
            msg = "FixMatchMeters: %d pseudo / ground-truth labels outside [0, %d) this epoch" % (bad, c)
            if strict:
                raise RuntimeError(msg)
            warnings.warn(msg + " (left out of the per-class counts, as the reference does)", RuntimeWarning, stacklevel=2)
        out, val = {}, {}
        for k, name in enumerate(F32_NAMES):
            val[name], out[name] = float(f32[k]), float(f32[12 + k])
        for k, name in enumerate(LOSS_NAMES):
            val[name], out[name] = float(f64[k]), float(f64[12 + k])
        cls = f64[18:].view(3, 3, c)          # (value / sum / avg, list, class)
        for k, name in enumerate(CLASS_NAMES):
            val[name], out[name] = cls[0, k].tolist(), cls[2, k].tolist()
        out["ema_t"] = self.ema_t.detach().clone() if self.ema_t is not None else None
        out["ema_t_corr"] = self.ema_t_corr.clone()
        values = tuple(out[k] for k in RETURN_ORDER)
        out.update(val=val, iterations=iters, labels_out_of_range=bad)
        return out, values
