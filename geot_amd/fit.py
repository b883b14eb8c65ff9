"""The training driver: the configured epochs, the learning-rate schedule, validation between epochs, checkpoints and
resume -- what main() and train_one_epoch() of examples/segmentation/train.py (:277-407, 434-437, 657-669) do around the loop
body that geot_amd/train_step.py holds.

    step    = build_fixmatch(device, cfg=..., meters=True)              # or SupervisedStep(model, ...): the first stage
    batcher = FixMatchBatcher(labelled, unlabelled, cfg.num_points, stream=torch.cuda.Stream(), draws=DeviceDraws(seed, views=True))
    out = fit(GraphedFixMatchStep(step), batcher, cfg, val=val_scans, ckpt_dir="runs/a")       # or the eager step
    out = fit(..., resume="runs/a/<run_name>_ckpt_latest.pt")                                    # continues bit for bit

It adds no kernel and nothing to an iteration: the loop is the one-batch look-ahead pipeline of INTEGRATION.md ("Training
batches"), the learning rates are device tensors the schedule fills between epochs (geot_amd/schedule.py), and the one host
synchronisation of an epoch is the read of its meters at its end.

Decisions of the driver (INTEGRATION.md section 7 states them with the two differences from main()):

* The look-ahead never crosses an epoch's end: an epoch's last call announces nothing, and the first call of the next epoch
  computes its batch work in line -- the same results, once per epoch.  At an epoch's end no look-ahead product is therefore
  outstanding, whatever follows: the meters' read, a validation, a save.
* A validation (and a test) leaves the training run's random streams as it found them: the host generators, the device's
  generator and the DeviceDraws counters are taken before it and put back after it.
* A checkpoint is written at an epoch's end only, behind schedule.step(epoch); the schedule itself is not saved: it is a
  function of the epoch.
"""
import itertools
import logging
import os
import sys
import time
import types

import torch
from torch.utils.data import BatchSampler, RandomSampler

from . import checkpoint
from .meters import CLASS_NAMES
from .schedule import LrSchedule

# the names examples/segmentation/train.py:304-330 logs and writes, for the values train_one_epoch returns under the names
# of geot_amd/meters.py (RETURN_ORDER)
LOG_NAMES = {"train_loss": "train_loss", "train_loss_l": "train_loss_l", "train_loss_u": "train_loss_u",
             "th_percentage": "th_percentage", "mean_pseudo_label_acc": "train_over_th_acc", "teacher_acc": "teacher_acc",
             "student_acc": "student_acc", "over_th_wobg": "over_th_wobg", "over_acc_wobg": "over_acc_wobg",
             "manifold_loss_feat": "manifold_loss_feat", "insT_identity_loss": "insT_identity_loss",
             "insT_threed_loss": "insT_threed_loss"}
CLASS_LOG_NAMES = dict(zip(CLASS_NAMES, ("train_over_th_acc_class_", "train_over_th_num_class_", "train_over_th_recall_class_")))


def _cfg(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def _inner(step):
    """The step inside a graph_step wrapper (the step itself when it is not wrapped)."""
    return getattr(step, "step", step)


def _is_fixmatch(step):
    return hasattr(step, "set_epoch")


def epoch_batches(n_l, n_u, batch_size_l, batch_size_u=None, generator=None):
    """The index batches one epoch of the reference's two training loaders yields: each loader's are
    BatchSampler(RandomSampler(range(n), generator=generator), batch_size, drop_last=True)
    (openpoints/dataset/build.py:105-123, 168-186: shuffle and drop_last for split 'train'), the labelled loader's first.  The
    labelled list is the epoch; one unlabelled batch is taken per labelled batch (train.py:436, 462) -> (labelled batches,
    unlabelled batches), lists of equal length; the unlabelled iterator is asked for exactly that many batches and not run to
    its end, as there (RandomSampler's closing draw is then never made).  An unlabelled loader that would run out first -- a StopIteration in the middle
    of the reference's epoch -- is a ValueError here, raised before anything is drawn.  n_u=None: the supervised stage's single
    list.  generator=None: each sampler seeds itself from torch's global generator, as the reference's do."""
    n_l, batch_size_l = int(n_l), int(batch_size_l)
    if batch_size_l < 1 or n_l < 0:
        raise ValueError("epoch_batches: n_l >= 0 and batch_size_l >= 1, got %r / %r" % (n_l, batch_size_l))
    if n_u is not None:
        n_u, batch_size_u = int(n_u), int(batch_size_l if batch_size_u is None else batch_size_u)
        if batch_size_u < 1 or n_u < 0:
            raise ValueError("epoch_batches: n_u >= 0 and batch_size_u >= 1, got %r / %r" % (n_u, batch_size_u))
        if n_u // batch_size_u < n_l // batch_size_l:
            raise ValueError("epoch_batches: the unlabelled loader runs out first -- %d batches of %d from %d scans against %d "
                             "labelled batches (the reference stops in mid-epoch with StopIteration)"
                             % (n_u // batch_size_u, batch_size_u, n_u, n_l // batch_size_l))
    labelled = list(BatchSampler(RandomSampler(range(n_l), generator=generator), batch_size_l, drop_last=True))
    if n_u is None:
        return labelled
    unlabelled = BatchSampler(RandomSampler(range(n_u), generator=generator), batch_size_u, drop_last=True)
    return labelled, list(itertools.islice(iter(unlabelled), len(labelled)))


def train_one_epoch(step, batcher, epoch, batches):
    """One epoch of `step` -- a FixMatchNTMStep over a FixMatchBatcher, a SupervisedStep over a SupervisedBatcher, or the
    graph_step wrapper of either (the same call) -- over `batches`, what epoch_batches returned.  Start: step.set_epoch(epoch)
    (SupervisedStep.new_epoch()), which restarts the step_per_update window, and the meters' reset().  The loop is the pipeline
    of INTEGRATION.md "Training batches": the next batch is queued on the batcher's stream, joined and announced as
    next_batches= / next_pos=; the epoch's last call announces nothing.  End: -> meters.read(), the one host synchronisation of
    the epoch; a step without meters returns None, a supervised step ({"last_loss": the last call's loss}, (that loss,))."""
    inner = _inner(step)
    fixmatch = _is_fixmatch(step)
    if fixmatch:
        idx_l, idx_u = batches
        if len(idx_l) != len(idx_u):
            raise ValueError("train_one_epoch: %d labelled and %d unlabelled batches" % (len(idx_l), len(idx_u)))
        plan = list(zip(idx_l, idx_u))
    else:
        plan = [(idx,) for idx in batches]
    if not plan:
        raise ValueError("train_one_epoch: the epoch has no batch (fewer scans than a batch holds: drop_last)")
    if fixmatch:
        step.set_epoch(epoch)
    else:
        inner.new_epoch()
    meters = getattr(inner, "meters", None)
    if meters is not None:
        meters.reset()

    def build(ids):
        out = batcher.batch(*ids)
        batcher.join(*out) if fixmatch else batcher.join(out)
        return out
    weighted = getattr(inner, "criterion_name", None) == "Weight_CELoss"
    out = None
    cur = build(plan[0])
    for it in range(len(plan)):
        nxt = build(plan[it + 1]) if it + 1 < len(plan) else None
        if fixmatch:
            out = step(cur[0], cur[1]) if nxt is None else step(cur[0], cur[1], next_batches=nxt)
        else:
            more = {"class_weights": cur["class_weights"]} if weighted else {}
            if nxt is not None:
                more["next_pos"] = nxt["pos"]
            out = step(cur["pos"], cur["cls"], cur["y"], **more)
        cur = nxt
    if meters is not None:
        return meters.read()
    if fixmatch:
        return None
    loss = float(out)
    return {"last_loss": loss}, (loss,)


def compute_prior(step, batcher, batches, num_classes=None):
    """train.py:276, 868-897: the class means `cm` over one pass of labelled batches with the student in eval mode
    (ntm.cal_mean_feature), copied IN PLACE into step.cm -- a captured graph reads that very tensor.  batches: an
    epoch_batches plan; the unlabelled half of every batch is built and not read (the batcher builds both)."""
    from . import ntm
    inner = _inner(step)
    model = inner.model
    idx_l, idx_u = batches

    def logits():
        for ids in zip(idx_l, idx_u):
            data, data_u = batcher.batch(*ids)
            batcher.join(data, data_u)
            yield model(data)[0], data["y"]
    was = model.training
    model.eval()
    try:
        with torch.no_grad():
            cm = ntm.cal_mean_feature(logits(), inner.cfg["num_classes"] if num_classes is None else num_classes)
            if cm is not None:
                inner.cm.copy_(cm)
    finally:
        model.train(was)
    return inner.cm


class _Numbers:
    """An optimizer as ckpt_util.save_checkpoint takes it, its device-tensor lr written as a number."""

    def __init__(self, optimizer):
        self.optimizer = optimizer

    def state_dict(self):
        return checkpoint.numbers_only(self.optimizer.state_dict())


def _protected(dev, draws, fn):
    """fn() with the training run's random streams put back behind it: the host generators, the device's generator
    (checkpoint.rng_state) and the DeviceDraws counters."""
    rng, counters = checkpoint.rng_state(dev), [d.state() for d in draws]
    try:
        return fn()
    finally:
        checkpoint.set_rng_state(rng)
        for d, s in zip(draws, counters):
            d.set_state(s)


def _record(epoch, lr, stats, seconds, clouds):
    rec = {"epoch": epoch, "lr": lr, "seconds": seconds, "clouds_per_s": clouds / seconds if seconds > 0 else float("inf")}
    if stats is None:
        return rec
    named = stats[0]
    for key, name in LOG_NAMES.items():
        if key in named:
            rec[name] = named[key]
    for key, name in CLASS_LOG_NAMES.items():
        for j, v in enumerate(named.get(key, ())):
            rec[name + str(j)] = v
    if "last_loss" in named:
        rec["last_loss"] = named["last_loss"]
    return rec


VAL_WHOLE = ("interp", "covered", "decoded")


def _val_whole(cfg, num_votes, graph, lookahead):
    """cfg.val_whole, checked before the first epoch: how a whole scan gets its labels from the sampled points in fit()'s
    validation -- "interp" (default: validate_scans / validate_scans_voted, get_pred_whole's interpolation), "covered"
    (validate_scans_covered: ceil(M / num_points) forward passes whose samples partition the scan) or "decoded"
    (validate_scans_decoded: one forward pass, the last decoder stage at every vertex).  Votes belong to "interp"; "decoded"
    has neither graph nor lookahead."""
    mode = _cfg(cfg, "val_whole", "interp")
    mode = "interp" if mode is None else mode
    if mode not in VAL_WHOLE:
        raise ValueError("fit: cfg.val_whole must be one of %s, got %r" % (", ".join(VAL_WHOLE), mode))
    if mode != "interp" and num_votes > 0:
        raise ValueError("fit: cfg.val_whole=%r takes no votes (cfg.num_votes=%d): votes are summed interpolations" % (mode, num_votes))
    if mode == "decoded" and (graph is not False or lookahead):
        raise ValueError("fit: cfg.val_whole='decoded' has no graph / lookahead form")
    return mode


def _val_teeth3ds(cfg):
    """cfg.val_teeth3ds, checked before the first epoch: a bool (default False); anything else is a ValueError."""
    on = _cfg(cfg, "val_teeth3ds", False)
    if not isinstance(on, bool):
        raise ValueError("fit: cfg.val_teeth3ds must be a bool, got %r" % (on,))
    return on


def fit(step, batcher, cfg, val=None, test=None, ckpt_dir=None, resume=None, log=logging.info, draws=None, generator=None,
        prior=True, graph=False, lookahead=0, refine=0, parts=None, val_stream=None, islands=None):
    """Train `step` over `batcher` for the configured epochs -> {"epoch", "best", "best_epoch", "records", "schedule", "generator"}.

    step / batcher: as train_one_epoch takes them.  cfg (a dict or an object with attributes): epochs, start_epoch (1),
    val_freq (1), test_freq (1), batch_size_l / batch_size_u (default: the step's cfg) or batch_size for the supervised
    stage, the schedule's keys (schedule.LrSchedule), num_points / num_classes / batch_size_val (2) / num_votes (0) for the
    validation, run_name ("run"), seed (0: the sampler generator's when `generator` is None), supervised_epochs (must be 0).
    Epochs run over range(start_epoch, epochs + 1) (train.py:277).

    The schedule is installed first -- every optimizer group's lr becomes a device tensor, so a wrapper handed in captures
    tensor learning rates -- and stepped behind every epoch (train.py:333-338).
    prior: before the first epoch of a FixMatch run that is not a resume, compute_prior() over one epoch_batches plan fills
    step.cm in place; False keeps what the step holds.
    val: a DeviceScanSet (or a ValBatcher / VoteBatcher on one).  Every val_freq epochs and at the last one the STUDENT
    (step.model) runs validation.validate_scans -- validate_scans_voted when cfg.num_votes > 0 -- with graph / lookahead /
    refine / parts / val_stream / islands passed through (islands: validation.clean_scans behind the refinement -- None / False:
    off, True or a dict of its keyword arguments; anything else is a ValueError before the first epoch), and the training
    run's random streams are put back (_protected): a run with validation trains to the bits of a run without.  cfg.val_whole
    (_val_whole; ValueError before the first epoch for an unknown value): "interp" (default) is that, "covered" runs validate_scans_covered, "decoded" validate_scans_decoded.
    cfg.val_teeth3ds (a bool, default False; ValueError before the first epoch for anything else): the validation's final
    labels also go through a validation.ToothScores, the record gains val_tsa, val_tsa_instance, val_tla, val_tir and val_score
    (the 3DTeethSeg challenge's scores) and one more line is logged; "best" and the checkpoints are untouched.  "Best" is the
    highest validation mIoU so far.  test: scored the same way at every save, on the student as it stands, and reported as test_*.
    ckpt_dir: at test_freq epochs, at the last epoch and at every new best, checkpoint.save writes
    <ckpt_dir>/<run_name>_ckpt_latest.pt (the step's whole state, `draws`, the generators, epoch, best, best_epoch and the
    sampler generator's state) and ckpt_util.save_checkpoint the reference-layout <run_name>_ckpt_latest.pth, copied to
    <run_name>_ckpt_best.pth at a new best -- the file the second stage names as pretrained_path.
    resume: a ..._ckpt_latest.pt; loaded into step / draws / generator in place, then schedule.step(epoch), and the run
    continues with the next epoch: an interrupted and resumed run gives the bits of an uninterrupted one.
    draws: the DeviceDraws whose counters travel (one or a sequence; default: the batcher's own, if it has one).
    generator: the torch.Generator of the two samplers (default: a new one seeded with cfg.seed).
    log: called once per epoch with a dict: epoch, lr (the rate the epoch trained at), the meters under train.py:304-330's
    names, val_miou / val_dsc / val_acc and best_val_* when a validation has run, test_*, saved, seconds and clouds_per_s.

    NotImplementedError: cfg.supervised_epochs > 0 in a FixMatch run (the two stages are two fit calls), an initialised
    process group of more than one rank, and what LrSchedule refuses."""
    import torch.distributed as dist
    from .openpoints.utils import ckpt_util
    num_votes = int(_cfg(cfg, "num_votes", 0) or 0)
    val_whole = _val_whole(cfg, num_votes, graph, lookahead)       # an unknown value: ValueError before anything is touched
    val_teeth = _val_teeth3ds(cfg)
    from . import validation
    islands = validation._islands_kw(islands, "fit")              # a bad value: ValueError here, before the first epoch
    for held_out in (val, test):                                  # islands={"mesh": ...} on a set without faces: likewise
        if held_out is not None:
            validation._need_mesh(islands, held_out, "fit")
    inner = _inner(step)
    fixmatch = _is_fixmatch(step)
    if fixmatch and (_cfg(cfg, "supervised_epochs", 0) or 0) > 0:
        raise NotImplementedError("fit: supervised_epochs=%r inside a FixMatch run is not built -- run the supervised stage "
                                  "as a fit() of its own (SupervisedStep, SupervisedBatcher)" % (_cfg(cfg, "supervised_epochs"),))
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError("fit: a process group of %d ranks -- the samplers are not sharded" % dist.get_world_size())
    epochs, start = int(_cfg(cfg, "epochs")), int(_cfg(cfg, "start_epoch", 1) or 1)
    val_freq, test_freq = int(_cfg(cfg, "val_freq", 1) or 1), int(_cfg(cfg, "test_freq", 1) or 1)
    run_name = _cfg(cfg, "run_name", "run") or "run"
    if fixmatch:
        own = getattr(inner, "cfg", {})
        sizes = (batcher.n_l, batcher.n_u, int(_cfg(cfg, "batch_size_l", own.get("batch_size_l", 2))),
                 int(_cfg(cfg, "batch_size_u", own.get("batch_size_u", 2))))
    else:
        sizes = (len(batcher), None, int(_cfg(cfg, "batch_size")))
    clouds = sizes[2] + (sizes[3] if fixmatch else 0)
    if draws is None:
        draws = getattr(batcher, "draws", None)
    draws = () if draws is None else tuple(draws) if isinstance(draws, (list, tuple)) else (draws,)
    if generator is None:
        generator = torch.Generator()
        generator.manual_seed(int(_cfg(cfg, "seed", 0) or 0))
    optimizers = inner.optimizers()
    param = optimizers[0].param_groups[0]["params"][0]
    dev = param.device if param.is_cuda else None
    schedule = LrSchedule(optimizers, cfg)
    best = best_epoch = None
    best_all = {}
    if resume is not None:
        extra = checkpoint.load(resume, step, draws=draws)
        start = int(extra["epoch"]) + 1
        best, best_epoch, best_all = extra.get("best"), extra.get("best_epoch"), dict(extra.get("best_all") or {})
        if extra.get("sampler") is not None:
            generator.set_state(extra["sampler"].cpu())
        schedule.step(start - 1)
    elif fixmatch and prior:
        compute_prior(step, batcher, epoch_batches(*sizes, generator=generator))
    val_cfg = {k: _cfg(cfg, k) for k in ("num_points", "num_classes", "datatransforms") if _cfg(cfg, k) is not None}

    def score(scans, epoch, teeth=False):
        """-> validate()'s three-tuple; with teeth (macc, miou, mdsc, the dict of ToothScores.read())."""
        vcfg = dict(val_cfg, epoch=epoch, epochs=epochs, num_votes=num_votes)
        kw = dict(batch_size=int(_cfg(cfg, "batch_size_val", 2) or 2), stream=val_stream, refine=refine, parts=parts)
        if islands is not None:
            kw["islands"] = islands
        if teeth:
            kw["teeth"] = validation.ToothScores(val_cfg.get("num_classes", 17), scans.device)
        if val_whole == "interp":
            fn = validation.validate_scans_voted if num_votes > 0 else validation.validate_scans
            kw.update(graph=graph, lookahead=lookahead)
        elif val_whole == "covered":
            # a covering draw is a device draw: a batcher handed in brings its own, a bare scan set gets a fresh counter per
            # validation, so every validation of a run covers the scans in the same way
            from .openpoints.dataset.sample_draw import DeviceDraws
            fn = validation.validate_scans_covered
            kw.update(graph=graph, lookahead=lookahead,
                      draws=None if getattr(scans, "draws", None) is not None else DeviceDraws(int(_cfg(cfg, "seed", 0) or 0)))
        else:
            fn = validation.validate_scans_decoded

        def run():
            triple = fn(inner.model, scans, vcfg, **kw)
            if not teeth:
                return triple
            out = kw["teeth"].read()
            validation.report_tooth_scores(out, vcfg)
            return tuple(triple) + (out,)
        return _protected(dev, draws, run)
    records = []
    epoch = start - 1
    for epoch in range(start, epochs + 1):
        t0 = time.perf_counter()
        batches = epoch_batches(*sizes, generator=generator)
        stats = train_one_epoch(step, batcher, epoch, batches)
        if stats is None and dev is not None:
            torch.cuda.synchronize(dev)
        seconds = time.perf_counter() - t0
        n_iter = len(batches[0]) if fixmatch else len(batches)
        rec = _record(epoch, schedule.values(epoch - 1)[0], stats, seconds, clouds * n_iter)
        last = epoch == epochs
        is_best = False
        if val is not None and (epoch % val_freq == 0 or last):
            scored = score(val, epoch, val_teeth)
            macc, miou, mdsc = (float(v) for v in scored[:3])
            rec.update(val_miou=miou, val_dsc=mdsc, val_acc=macc)
            if val_teeth:
                rec.update(("val_" + k, scored[3][k]) for k in ("tsa", "tsa_instance", "tla", "tir", "score"))
            if best is None or miou > best:
                is_best, best, best_epoch = True, miou, epoch
                best_all = {"miou": miou, "dsc": mdsc, "acc": macc}
        if best is not None:
            rec.update(best_val_miou=best_all["miou"], best_val_dsc=best_all["dsc"], best_val_acc=best_all["acc"],
                       best_epoch=best_epoch)
        schedule.step(epoch)
        saved = ckpt_dir is not None and (epoch % test_freq == 0 or last or is_best)
        if saved:
            os.makedirs(ckpt_dir, exist_ok=True)
            checkpoint.save(os.path.join(ckpt_dir, "%s_ckpt_latest.pt" % run_name), step, draws=draws, rng_device=dev,
                            epoch=epoch, best=best, best_epoch=best_epoch, best_all=best_all, sampler=generator.get_state())
            ckpt_util.save_checkpoint({"run_name": run_name, "ckpt_dir": os.fspath(ckpt_dir), "save_freq": _cfg(cfg, "save_freq", 0)},
                                      inner.model, epoch, optimizer=_Numbers(optimizers[0]),
                                      additioanl_dict=dict(best_all, best_val=best) if best is not None else None, is_best=is_best)
        if test is not None and (epoch % test_freq == 0 or last):
            macc, miou, mdsc = (float(v) for v in score(test, epoch))
            rec.update(test_miou=miou, test_dsc=mdsc, test_acc=macc)
        rec["saved"] = saved
        records.append(rec)
        log(rec)
    return {"epoch": epoch, "best": best, "best_epoch": best_epoch, "records": records, "schedule": schedule,
            "generator": generator}


class _CallableModule(types.ModuleType):
    """`from geot_amd import fit` binds this module: calling it calls fit(), so that the function and the module that carries
    its name are one object to a caller."""

    def __call__(self, *args, **kwargs):
        return fit(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule
