"""geot_amd/meters.py (csrc/meters.hip): the FixMatch epoch statistics on the device equal the reference's per-iteration
statements and AverageMeters (examples/segmentation/train.py:599-644, 672-699), restated below on the same CUDA tensors --
every value `==` (NaN matching NaN), per iteration and as the epoch's averages; and a step that keeps them computes
exactly what a step without them computes, eagerly and replayed from hipGraphs, on both sides of switch_ep."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


class AverageMeter:
    """The reference's meter (openpoints/utils/metrics.py): Python arithmetic on whatever it is handed."""

    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


class ReferenceMeters:
    """train_one_epoch's meters, fed by a restatement of train.py:599-644 on the iteration's tensors."""

    def __init__(self, c, bl, bu, threshold):
        self.c, self.bl, self.bu, self.threshold = c, bl, bu, threshold
        self.scalar = {k: AverageMeter() for k in ("th", "pl", "t_acc", "s_acc", "wobg", "acc_wobg", "loss", "loss_l",
                                                   "loss_u", "feat", "ident", "3d")}
        self.cls = {k: [AverageMeter() for _ in range(c)] for k in ("acc", "num", "rec")}

    def iteration(self, label_u_aug, logits_u_aug, y_u, prob_s, loss, sup, unsup, threed):
        thresh_mask = logits_u_aug.ge(torch.tensor(self.threshold)).bool()
        over_th = torch.sum(thresh_mask) / (thresh_mask.shape[0] * thresh_mask.shape[1]) * 100
        teacher_acc = torch.sum(label_u_aug == y_u.squeeze(-1)) / (label_u_aug.shape[0] * label_u_aug.shape[1])
        _, label_u_strong = torch.max(prob_s, dim=1)
        student_acc = torch.sum(label_u_strong == y_u.squeeze(-1)) / (label_u_strong.shape[0] * label_u_strong.shape[1])
        pseudo_label, target_u = label_u_aug.clone().detach(), y_u.squeeze(-1)
        den = torch.sum(thresh_mask)
        pl_acc = 0 if den == 0 else torch.sum((pseudo_label == target_u) * thresh_mask) / den * 100
        acc, num, rec = [], [], []
        for ii in range(self.c):
            cur_pred, cur_gt = (pseudo_label == ii).float(), (target_u == ii).float()
            den = torch.sum(cur_pred * thresh_mask.float())
            acc.append(0 if den == 0 else (torch.sum((cur_pred * cur_gt) * thresh_mask.float()) / den).item() * 100)
            den = torch.sum(cur_pred)
            num.append(0 if den == 0 else (torch.sum(cur_pred * thresh_mask.float()) / den).item() * 100)
            den = torch.sum(cur_gt)
            rec.append(0 if den == 0 else (torch.sum((cur_pred * cur_gt) * thresh_mask.float()) / den).item() * 100)
        cur_pred = (pseudo_label > 0).float()
        over_th_wobg = torch.sum(thresh_mask * cur_pred) / (torch.sum(cur_pred)) * 100
        total_acc = torch.sum(((pseudo_label == target_u) * cur_pred) * (thresh_mask))
        den = torch.sum(cur_pred * thresh_mask.float())
        over_acc_wobg = 0 if den == 0 else ((total_acc) / den) * 100
        m, bl, bu = self.scalar, self.bl, self.bu
        m["loss"].update(loss.item(), n=bl + bu)
        m["loss_l"].update(sup.item(), n=bl)
        m["loss_u"].update(unsup.item(), n=bu)
        m["th"].update(over_th, n=bu)
        m["feat"].update(torch.tensor([0.]).item(), n=bu)
        m["ident"].update(torch.tensor([0.]).item(), n=bu)
        m["3d"].update(threed.item(), n=bu)
        m["t_acc"].update(teacher_acc, n=bu)
        m["s_acc"].update(student_acc, n=bu)
        m["wobg"].update(over_th_wobg, n=bu)
        m["acc_wobg"].update(over_acc_wobg, n=bu)
        m["pl"].update(pl_acc, n=bu)
        for jj in range(self.c):
            self.cls["acc"][jj].update(acc[jj], n=bu)
            self.cls["num"][jj].update(num[jj], n=bu)
            self.cls["rec"][jj].update(rec[jj], n=bu)

    def named(self, what):
        """{meters.py name: the meters' `what` ("val" / "avg")} as Python floats."""
        f = lambda v: float(v.item()) if torch.is_tensor(v) else float(v)     # noqa: E731
        m = self.scalar
        out = {"th_percentage": m["th"], "mean_pseudo_label_acc": m["pl"], "teacher_acc": m["t_acc"],
               "student_acc": m["s_acc"], "over_th_wobg": m["wobg"], "over_acc_wobg": m["acc_wobg"], "train_loss": m["loss"],
               "train_loss_l": m["loss_l"], "train_loss_u": m["loss_u"], "manifold_loss_feat": m["feat"],
               "insT_identity_loss": m["ident"], "insT_threed_loss": m["3d"]}
        out = {k: f(getattr(v, what)) for k, v in out.items()}
        for k, name in (("acc", "mean_pseudo_label_acc_classwise"), ("num", "mean_th_meter_u_classwise"),
                        ("rec", "mean_th_meter_u_classwise_recall")):
            out[name] = [f(getattr(v, what)) for v in self.cls[k]]
        return out


def _same_value(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _assert_equal(got, want, where):
    bad = []
    for k, w in want.items():
        g = got[k]
        if isinstance(w, list):
            bad += ["%s[%d]: %r != %r" % (k, i, x, y) for i, (x, y) in enumerate(zip(g, w)) if not _same_value(x, y)]
        elif not _same_value(g, w):
            bad.append("%s: %r != %r" % (k, g, w))
    assert not bad, (where, bad[:10])


def _case(name, seed, b=2, n=1500, c=17):
    """Tensors of one iteration: (label_u_aug, logits_u_aug, y_u, prob_s, (loss, sup, unsup, threed), ema_t_corr)."""
    g = torch.Generator().manual_seed(seed)
    prob = F.softmax(torch.randn(b, c, n, generator=g) * 3, dim=1)
    conf, t = torch.max(prob, dim=1)
    y = torch.where(torch.rand(b, n, generator=g) < 0.6, t, torch.randint(0, c, (b, n), generator=g))
    prob_s = F.softmax(torch.randn(b, c, n, generator=g) * 3, dim=1)
    if name == "none_confident":                  # threshold 0.9: not one confident point
        conf = conf * 0.5
    elif name == "no_foreground":                 # every pseudo label is background: over_th_wobg = 0 / 0
        t = torch.zeros_like(t)
    elif name == "absent_class":                  # one class neither predicted nor present
        a = min(5, c - 3)
        t = torch.where(t == a, torch.full_like(t, a + 1), t)
        y = torch.where(y == a, torch.full_like(y, a + 2), y)
    elif name == "ties_nan":                      # tied maxima, NaN rows / entries, NaN confidence
        prob_s[:, :, :40] = 0.25
        prob_s[0, 3, 10:20] = float("nan")
        prob_s[1, :, 30:35] = float("nan")
        prob_s[1, min(9, c - 2), 100:140] = 2.0
        prob_s[1, min(12, c - 1), 100:120] = 2.0
        conf[0, :25] = float("nan")
        y[:, :40] = 3
    elif name == "out_of_range":                  # ignore-style ground truth labels
        y[0, :7] = -1
        y[1, 7:9] = c
    elif name == "column_y":                      # data_u["y"] as (B_u, N, 1)
        y = y.unsqueeze(-1)
    losses = tuple(torch.rand((), generator=g) * s for s in (4.0, 2.0, 1.5, 0.3))
    ema_corr = torch.rand(c, c, generator=g)
    to = lambda x: x.to(DEV).contiguous()         # noqa: E731
    return to(t), to(conf), to(y), to(prob_s), tuple(to(x) for x in losses), to(ema_corr)


@pytest.mark.parametrize("threshold,cases", [
    (0.0, ["plain", "column_y", "absent_class", "no_foreground", "plain"]),
    (0.9, ["none_confident", "plain", "ties_nan"]),
    (0.3, ["ties_nan", "no_foreground", "plain"]),
    (0.0, ["plain"]),
])
@pytest.mark.parametrize("c", [17, 5])
def test_meters_equal_the_reference_statements(threshold, cases, c):
    from geot_amd.meters import FixMatchMeters
    ema_t = torch.rand(c, c, device=DEV)
    meters = FixMatchMeters(c, DEV, batch_size_l=2, batch_size_u=3, threshold=threshold, ema_t=ema_t)
    ref = ReferenceMeters(c, 2, 3, threshold)
    for it, name in enumerate(cases):
        t, conf, y, prob_s, losses, ema_corr = _case(name, 100 * it + c, c=c)
        meters.update(t, conf, y, prob_s, *losses, ema_t_corr=ema_corr)
        ref.iteration(t, conf, y, prob_s, *losses)
        got, values = meters.read()
        _assert_equal(got["val"], ref.named("val"), (name, it, "val"))
        _assert_equal(got, ref.named("avg"), (name, it, "avg"))
        assert got["iterations"] == it + 1 and got["labels_out_of_range"] == 0
        assert torch.equal(got["ema_t_corr"], ema_corr) and torch.equal(got["ema_t"], ema_t)
        assert len(values) == 17 and values[0] == got["train_loss"] and values[5] == got["mean_pseudo_label_acc_classwise"]
    if "no_foreground" in cases:
        assert math.isnan(got["over_th_wobg"])       # the reference's unguarded 0 / 0 poisons the epoch mean
    meters.reset()
    got, _ = meters.read()
    assert got["iterations"] == 0 and got["train_loss"] == 0.0 and got["th_percentage"] == 0.0
    t, conf, y, prob_s, losses, ema_corr = _case("plain", 7, c=c)
    meters.update(t, conf, y, prob_s, *losses, ema_t_corr=ema_corr)
    ref = ReferenceMeters(c, 2, 3, threshold)
    ref.iteration(t, conf, y, prob_s, *losses)
    _assert_equal(meters.read()[0], ref.named("avg"), "after reset")


def test_an_out_of_range_label_is_reported_at_read_out():
    from geot_amd.meters import FixMatchMeters
    meters = FixMatchMeters(17, DEV, threshold=0.0)
    ref = ReferenceMeters(17, 2, 2, 0.0)
    for it, name in enumerate(["plain", "out_of_range", "plain"]):
        t, conf, y, prob_s, losses, _ = _case(name, 40 + it)
        meters.update(t, conf, y, prob_s, *losses)
        ref.iteration(t, conf, y, prob_s, *losses)
    with pytest.warns(RuntimeWarning, match="9 pseudo / ground-truth labels outside"):
        got, _ = meters.read()                    # the values, as the reference computes them with those points left out
    assert got["labels_out_of_range"] == 9
    _assert_equal(got, ref.named("avg"), "out of range")
    with pytest.raises(RuntimeError, match="9 pseudo / ground-truth labels outside"):
        meters.read(strict=True)


def test_meters_refuse_tensors_off_their_gpu_before_any_launch():
    """A host tensor (data_u["y"] left on the CPU, most likely) is refused with a RuntimeError and nothing is launched:
    the counters and meters are untouched and the next iteration counts as the first."""
    from geot_amd.meters import FixMatchMeters
    with pytest.raises(RuntimeError, match="GPU"):
        FixMatchMeters(17, "cpu")
    meters = FixMatchMeters(17, DEV, threshold=0.0)
    t, conf, y, prob_s, losses, corr = _case("plain", 9)
    bad_inputs = [(t, conf, y.cpu(), prob_s, losses, corr), (t.cpu(), conf, y, prob_s, losses, corr),
                  (t, conf, y, prob_s.cpu(), losses, corr), (t, conf, y, prob_s, (losses[0].cpu(),) + losses[1:], corr),
                  (t, conf, y, prob_s, losses, corr.cpu())]
    for args in bad_inputs:
        with pytest.raises(RuntimeError, match="is on cpu"):
            meters.update(*args[:4], *args[4], ema_t_corr=args[5])
    torch.cuda.synchronize()
    for buf in (meters.counts, meters.f32, meters.f64, meters.i64):
        assert not buf.any()
    meters.update(t, conf, y, prob_s, *losses, ema_t_corr=corr)
    ref = ReferenceMeters(17, 2, 2, 0.0)
    ref.iteration(t, conf, y, prob_s, *losses)
    got, _ = meters.read()
    assert got["iterations"] == 1
    _assert_equal(got, ref.named("avg"), "after the refusals")


def test_meters_refuse_2_pow_24_points():
    from geot_amd.meters import FixMatchMeters
    meters = FixMatchMeters(3, DEV)
    t = torch.zeros(1, 1 << 24, dtype=torch.long, device=DEV)
    conf = torch.zeros(1, 1 << 24, device=DEV)
    s = torch.zeros((), device=DEV)
    with pytest.raises(RuntimeError, match="2\\^24"):
        meters.update(t, conf, t, torch.zeros(1, 3, 1 << 24, device=DEV), s, s, s, s)


# ---- the meters inside the training step ----------------------------------------------------------------------------------
SMALL = dict(trans_dim=384, depth=3, num_heads=4, group_size=32, num_group=128, encoder_dims=256, nclasses=17,
             drop_path_rate=0.1, downsample_targets=[2048, 1024, 512], extract_layers=[1, 2, 3])


def _batch(seed, n=4096):
    from geot_amd.synth import make_batch, region_labels
    xl, xu = make_batch(2, n, start_index=seed)[0], make_batch(2, n, start_index=seed + 50)[0]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    lab, unl, strong = T(xl), T(xu), T(xu * np.float32(1.04))
    z = torch.zeros(2, 1, dtype=torch.long, device=DEV)
    return ({"pos": lab, "x": lab.transpose(1, 2).contiguous(), "cls": z, "y": T(region_labels(xl))},
            {"pos_w": unl, "x_w": unl.transpose(1, 2).contiguous(), "cls_w": z, "pos_s": strong,
             "x_s": strong.transpose(1, 2).contiguous(), "cls_s": z, "raw_pos": unl, "y": T(region_labels(xu)).unsqueeze(-1)})


def _params(step):
    out = {"ema_t": step.ema_t.detach().clone()}
    for name, mod in (("model", step.model), ("T", step.T_predictor)):
        out.update({name + "." + k: v.detach().clone() for k, v in mod.state_dict().items()})
    return out


EPOCHS = [1, 2, 50, 50, 51, 51, 52, 52]     # four iterations before switch_ep (50), four after it: with warmup=2 the graphed
                                            # step captures and replays P / M before the switch and P@2 / M@2 after it


def test_a_step_with_meters_equals_one_without_and_its_meters_the_reference():
    from geot_amd import train_step as ts, graph_step as gs
    cfg = dict(ts.NTM_CFG, threed_k=8)
    batches = [_batch(3), _batch(400)]
    runs = {}
    for mode in ("plain", "meters", "graphed"):
        torch.manual_seed(5)
        step = ts.build_fixmatch(DEV, seg_cfg=SMALL, cfg=cfg, use_ddp=False, meters=mode != "plain")
        assert (step.meters is None) == (mode == "plain")
        call = gs.GraphedFixMatchStep(step, warmup=2) if mode == "graphed" else step
        seen = []
        if mode == "meters":
            update = step.meters.update

            def recording(*args, **kw):
                seen.append([a.detach().clone() for a in args[:8]])
                return update(*args, **kw)
            step.meters.update = recording
        torch.manual_seed(11)
        losses, reads = [], []
        for i, epoch in enumerate(EPOCHS):
            if mode == "graphed" and epoch == 51 and not call.step.self_labelling:
                assert {"P", "M"} <= set(call.graphs), sorted(call.graphs)      # the teacher's phase replays before the switch
            call.set_epoch(epoch)
            cur, nxt = batches[i % 2], batches[(i + 1) % 2]
            res = call(cur[0], cur[1], next_batches=nxt)
            losses.append({k: v.clone() for k, v in res.items()})
            if step.meters is not None:
                reads.append(step.meters.read())
        torch.cuda.synchronize()
        if mode == "graphed":
            assert {"P@2", "M@2"} <= set(call.graphs), sorted(call.graphs)     # captured: no host sync inside the step
        runs[mode] = (losses, _params(step), reads, seen)
    for mode in ("meters", "graphed"):
        for i, (a, b) in enumerate(zip(runs["plain"][0], runs[mode][0])):
            assert all(torch.equal(a[k], b[k]) for k in a), (mode, i)
        p0, p1 = runs["plain"][1], runs[mode][1]
        assert [k for k in p0 if not torch.equal(p0[k], p1[k])] == [], mode
    # the eager step's meters against the restatement fed with the very tensors the step handed them
    ref = ReferenceMeters(17, cfg["batch_size_l"], cfg["batch_size_u"], cfg["threshold"])
    assert len(runs["meters"][3]) == len(EPOCHS)
    for i, args in enumerate(runs["meters"][3]):
        ref.iteration(*args)
        got = runs["meters"][2][i][0]
        _assert_equal(got["val"], ref.named("val"), ("eager val", i))
        _assert_equal(got, ref.named("avg"), ("eager avg", i))
    # ... and the replayed step's meters against the eager step's, read for read
    for i, (a, b) in enumerate(zip(runs["meters"][2], runs["graphed"][2])):
        a, b = a[0], b[0]
        _assert_equal(b["val"], a["val"], ("graphed val", i))
        _assert_equal(b, {k: a[k] for k in a if k not in ("val", "ema_t", "ema_t_corr", "iterations", "labels_out_of_range")},
                      ("graphed avg", i))
        assert torch.equal(a["ema_t_corr"], b["ema_t_corr"]) and torch.equal(a["ema_t"], b["ema_t"]), i
        assert b["iterations"] == i + 1


@pytest.mark.parametrize("graphed", [False, True])
def test_a_host_ground_truth_is_refused_before_the_step_runs(graphed):
    """data_u["y"] on the CPU with the meters on: the step (eager or replayed) raises before it queues anything -- parameters,
    ema_t and meters untouched; a meters object built without ema_t reports the step's."""
    from geot_amd import train_step as ts, graph_step as gs
    from geot_amd.meters import FixMatchMeters
    cfg = dict(ts.NTM_CFG, threed_k=8)
    torch.manual_seed(5)
    step = ts.build_fixmatch(DEV, seg_cfg=SMALL, cfg=cfg, use_ddp=False, meters=FixMatchMeters(17, DEV))
    assert step.meters.ema_t is step.ema_t
    call = gs.GraphedFixMatchStep(step, warmup=2) if graphed else step
    d, u = _batch(3)
    before = _params(step)
    for bad in (dict(u, y=u["y"].cpu()), {k: v for k, v in u.items() if k != "y"}):
        with pytest.raises(RuntimeError, match="data_u\\['y'\\]"):
            call(d, bad)
    torch.cuda.synchronize()
    after = _params(step)
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert step.meters.read()[0]["iterations"] == 0 and not step.meters.counts.any()
    call(d, u)                                     # and the same step goes on with a proper batch
    assert step.meters.read()[0]["iterations"] == 1
