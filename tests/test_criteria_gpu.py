"""GPU suite of the loss switches of the FixMatch+NTM loop: the fused criteria (csrc/loss.hip geot_weighted_ce,
geot_poly1_focal_beta) against the reference-executed fixture and against fp64 composites at every shape at which the
kernels branch; their gradient details and reproducibility; FixMatchNTMStep / SupervisedStep under every switch against
the reference's statements spelled out on the same modules, bit for bit; the hipGraph replay of two non-default
configurations (own process, fast launch mode); the two switched losses in the epoch meters.

Tolerance: the project's `close` / `referee` (tests/test_ref_fixtures_gpu.py): 1e-5 of the element's row scale."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import make_criteria_golden as maker  # noqa: E402
from test_fixmatch_phase2_gpu import SMALL, _batch, _same, _state  # noqa: E402
from test_ref_fixtures_gpu import REL, T, _row_scale, close, host, referee  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TH = 0.95


def crit(name, **kw):
    from geot_amd.openpoints.loss import build_criterion_from_cfg
    return build_criterion_from_cfg({"NAME": name, **kw})


def run(fn, *xs):
    """fn(*leaves) -> loss; -> [loss, gradient of every leaf] as numpy."""
    leaves = [x.detach().clone().requires_grad_(True) for x in xs]
    loss = fn(*leaves)
    loss.backward()
    return [host(loss)] + [host(x.grad) for x in leaves]


def judge(got, ref32, ref64, what):
    """`close` to the reference's fp32 and fp64 runs; where its own fp32 run is farther than that from its fp64 run,
    `referee`."""
    ref32, ref64 = np.asarray(ref32, np.float64), np.asarray(ref64, np.float64)
    own = float((np.abs(ref32 - ref64) / _row_scale(ref64)).max())
    print("%-12s reference fp32 vs fp64 %.3g  ours vs fp64 %.3g" % (what, own, float(
        (np.abs(np.asarray(got, np.float64) - ref64) / _row_scale(ref64)).max())))
    if own > REL:
        referee(got, ref32, ref64, what=what)
    else:
        close(got, ref32, ref64, what=what)


# ---- fixtures ----------------------------------------------------------------------------------------------------------------
def test_fused_criteria_equal_the_reference_classes(golden):
    ref, z = golden("criteria_ref.npz"), maker.draw_inputs()
    x, t, lab, lab_u = T(z["logits"]), T(z["t"]), T(z["labels"], torch.int64), T(z["labels_u"], torch.int64)
    cf, cf_nan = T(z["conf"]), T(z["conf_nan"])
    cases = {}
    for bw in (2, 3):
        cases["wce_bw%d" % bw] = run(lambda a, bw=bw: crit("Weight_CELoss")(a, lab, T(z["cw%d" % bw])), x)
    keep_lab = lab_u.clone()
    cases["wceu_t095"] = run(lambda a: crit("Weight_CELoss_U")(a, lab_u, T(z["cw2"]), cf_nan, thresh=TH), x)
    assert torch.equal(lab_u, keep_lab)                                   # the caller's gt is not written
    cases["pu_t095"] = run(lambda a: crit("Poly1FocalLoss_U")(a, lab, cf_nan, thresh=TH), x)
    cases["put_t095"] = run(lambda a, b: crit("Poly1FocalLoss_U_T")(a, lab, cf, None, b, thresh=TH), x, t)
    for name, got in cases.items():
        for k, g in zip(("loss", "grad", "gradt"), got):
            judge(g, ref["%s_%s_f32" % (name, k)], ref["%s_%s_f64" % (name, k)], name + "." + k)


# ---- branch shapes -----------------------------------------------------------------------------------------------------------
def draw(b, c, n, bw, seed=0, p_conf=0.6):
    g = torch.Generator().manual_seed(1000 * seed + 31 * n + 7 * c + b)
    x = (torch.randn(b, c, n, generator=g) * 3).to(DEV)
    t = ((torch.rand(b, c, n, generator=g) * 3.75 + 0.25) * (torch.randint(0, 2, (b, c, n), generator=g) * 2 - 1)).to(DEV)
    lab = torch.randint(0, c, (b, n), generator=g).to(DEV)
    conf = torch.where(torch.rand(b, n, generator=g) < p_conf, 0.97, 0.5).to(DEV) * (1 - 0.02 * torch.rand(b, n, generator=g).to(DEV))
    cw = (torch.rand(bw, c, generator=g) * 0.1 + 0.01).to(DEV)
    return x, t, lab, conf, cw


def four(x, t, lab, conf, cw, thresh=TH, dt=None):
    """The four criteria on one input set -> {name: [loss, grads...]}; dt=torch.float64: their fp64 composites."""
    c = (lambda a: a.to(dt)) if dt is not None else (lambda a: a)
    return {"wce": run(lambda a: crit("Weight_CELoss")(a, lab, c(cw)), c(x)),
            "wceu": run(lambda a: crit("Weight_CELoss_U")(a, lab, c(cw), c(conf), thresh=thresh), c(x)),
            "pu": run(lambda a: crit("Poly1FocalLoss_U")(a, lab, c(conf), thresh=thresh), c(x)),
            "put": run(lambda a, b: crit("Poly1FocalLoss_U_T")(a, lab, c(conf), None, b, thresh=thresh), c(x), c(t))}


def fused_calls(monkeypatch):
    """Count the launches of the new entry points: the fused path really ran (or, for C = 33, really did not)."""
    from geot_amd.ext import _common
    seen, real = [], _common.call
    monkeypatch.setattr(_common, "call", lambda name, *a: (seen.append(name), real(name, *a))[1])
    return seen


SHAPES = [(3, 17, n, 2) for n in (1, 63, 257, 1025, 33000)] + \
         [(1, 1, 257, 1), (3, 5, 63, 3), (1, 32, 257, 3), (3, 32, 1025, 1), (1, 5, 1025, 2), (1, 17, 257, 1)]


@pytest.mark.parametrize("b,c,n,bw", SHAPES)
def test_fused_path_equals_the_fp64_composite_at_every_branch(b, c, n, bw, monkeypatch):
    seen = fused_calls(monkeypatch)
    ins = draw(b, c, n, bw)
    got = four(*ins)
    assert seen.count("geot_weighted_ce") == 2 and seen.count("geot_weighted_ce_grad") == 2, seen
    assert seen.count("geot_poly1_focal_beta") == 1 and seen.count("geot_poly1_focal_beta_grad") == 1, seen
    del seen[:]
    want = four(*ins, dt=torch.float64)
    assert not [s for s in seen if "weighted_ce" in s or "poly1" in s], seen            # fp64: the composite
    for name in got:
        for k, (g, w) in enumerate(zip(got[name], want[name])):
            assert np.isfinite(w).all()
            close(g, w, what="%s[%d] b%d c%d n%d bw%d" % (name, k, b, c, n, bw))


def test_more_than_32_classes_take_the_composite(monkeypatch):
    seen = fused_calls(monkeypatch)
    ins = draw(2, 33, 257, 2)
    got, want = four(*ins), four(*ins, dt=torch.float64)
    assert not [s for s in seen if "weighted_ce" in s or "poly1_focal_beta" in s], seen
    for name in got:
        for g, w in zip(got[name], want[name]):
            close(g, w, what=name)


def test_all_ignored_none_ignored_and_a_nan_confidence():
    x, t, lab, conf, cw = draw(2, 17, 1025, 2)
    # every point ignored: loss 0, gradient exactly 0, no NaN
    for name, res in four(x, t, lab, conf * 0.5, cw).items():
        if name != "wce":
            assert res[0] == 0.0 and all((g == 0).all() for g in res[1:]), name
    # no point ignored (confident everywhere, no background label)
    sure, fg = torch.full_like(conf, 0.99), lab.clamp(min=1)
    got, want = four(x, t, fg, sure, cw), four(x, t, fg, sure, cw, dt=torch.float64)
    for name in got:
        for g, w in zip(got[name], want[name]):
            close(g, w, what="none ignored " + name)
        assert (got[name][1] != 0).all(), name
    # thresh = 0.0 and one NaN confidence: that point alone is dropped (put divides the confidence: left out here)
    cf = conf.clone()
    cf[1, 7] = float("nan")
    got, want = four(x, t, fg, cf, cw, thresh=0.0), four(x, t, fg, cf, cw, thresh=0.0, dt=torch.float64)
    for name in ("wceu", "pu"):
        assert np.isfinite(got[name][0]) and np.isfinite(got[name][1]).all()
        for g, w in zip(got[name], want[name]):
            close(g, w, what="nan confidence " + name)
        zero = got[name][1] == 0
        assert zero[1, :, 7].all() and zero.sum() == 17, name


# ---- gradient details --------------------------------------------------------------------------------------------------------
def test_gradient_details(monkeypatch):
    x, t, lab, conf, cw = draw(2, 17, 257, 3)
    lab[0, :5] = 0
    lab[1, 3] = 255
    conf[1, 3] = 0.99
    got = four(x, t, lab.clamp(max=16), conf, cw)
    wceu = run(lambda a: crit("Weight_CELoss_U")(a, lab, cw, conf, thresh=TH), x)
    dead = ~(conf.ge(TH) & (lab != 0) & (lab != 255))
    assert dead[1, 3] and dead[0, :5].all() and np.isfinite(wceu[0])
    g = torch.from_numpy(wceu[1]).permute(0, 2, 1)
    assert (g[dead.cpu()] == 0).all() and (g[~dead.cpu()] != 0).all()
    for name in ("pu", "put"):
        g = torch.from_numpy(got[name][1]).permute(0, 2, 1)
        assert (g[~conf.ge(TH).cpu()] == 0).all() and (g[conf.ge(TH).cpu()] != 0).all(), name
    gt = torch.from_numpy(got["put"][2])
    on = F.one_hot(lab.clamp(max=16).cpu(), 17).permute(0, 2, 1).bool()
    assert (gt[~on] == 0).all() and (gt[on & conf.ge(TH).cpu()[:, None, :]] != 0).all()      # d/dt: the label channel only
    # a label of C poisons the loss (the reference raises there); GEOT_CHECK_LABELS=1 gives the synchronous raise
    bad = lab.clamp(max=16).clone()
    bad[0, 9] = 17
    sure = torch.full_like(conf, 0.99)
    calls = {"wce": lambda: crit("Weight_CELoss")(x, bad, cw), "wceu": lambda: crit("Weight_CELoss_U")(x, bad, cw, sure, thresh=TH),
             "put": lambda: crit("Poly1FocalLoss_U_T")(x, bad, sure, None, t, thresh=TH),
             "pu": lambda: crit("Poly1FocalLoss_U")(x, bad, sure, thresh=TH)}
    for name, fn in calls.items():
        assert torch.isnan(fn()), name
    monkeypatch.setenv("GEOT_CHECK_LABELS", "1")
    for name, fn in calls.items():
        with pytest.raises(RuntimeError):
            fn()
    assert torch.isfinite(crit("Weight_CELoss_U")(x, lab, cw, conf, thresh=TH))        # 255 is the ignore index, not an error


def test_two_calls_give_the_same_bits():
    ins = draw(3, 17, 33000, 3)
    a, b = four(*ins), four(*ins)
    for name in a:
        for g, w in zip(a[name], b[name]):
            assert np.array_equal(g, w), name


# ---- composition: the steps against the reference's statements on the same modules -----------------------------------------
def _batches():
    out = []
    for seed in (3, 400):
        d, u = _batch(seed)
        d["class_weights"] = (torch.rand(2, 17, generator=torch.Generator().manual_seed(seed)) * 0.1 + 0.01).to(DEV)
        u["y"] = d["y"].flip(0).contiguous()
        out.append((d, u))
    return out


def _new_step(cfg, meters=None):
    from geot_amd import train_step as ts
    torch.manual_seed(5)
    return ts.build_fixmatch(DEV, seg_cfg=SMALL, cfg=cfg, use_ddp=False, meters=meters)


def _composed(step, data, data_u):
    """examples/segmentation/train.py:460-666 for one iteration, statement by statement, on the step's own modules."""
    from geot_amd import ntm
    cfg = step.cfg
    bl, bu, n = data["pos"].shape[0], data_u["pos_w"].shape[0], data["pos"].shape[1]
    p_threshold = cfg["threshold"]
    if not step.self_labelling:                                                  # :469-475
        with torch.no_grad():
            step.model_t.eval()
            pred_u = F.softmax(step.model_t(data_u, if_teacher=True)[0], dim=1)
            logits_u_aug, label_u_aug = torch.max(pred_u, dim=1)
    step.model.train()
    step.T_predictor.train()
    data_u = dict(data_u, T=step.ema_t)
    pred_all, delta_T, sigma = step.model(data, u0=data_u, fixmatch=True)        # :490
    pred_l, pred_u_strong, pred_u_w = torch.split(pred_all, [bl, bu, pred_all.shape[0] - bl - bu])
    if step.self_labelling:                                                      # :494-497
        pred_u = F.softmax(pred_u_w, dim=1)
        logits_u_aug, label_u_aug = torch.max(pred_u.detach(), dim=1)
    ema_t_corr, ema_next, _, _ = ntm.class_transition(pred_u.clone().detach(), sigma, step.ema_t, cfg["geo_lambma"],
                                                      cfg["ema_t_decay"], filter_outlier=cfg["filter_outlier"])   # :505-545
    pred_u_strong_softmax = F.softmax(pred_u_strong, dim=1)                      # :547-552
    insT = step.T_predictor(pred_u_strong_softmax.detach(), step.cm)
    pred_u_strong_corr = ntm.correct_logits(pred_u_strong, insT, ema_t_corr, cfg["lambma"])
    with torch.no_grad():                                                        # :556-557
        step.ema_t.copy_(ema_next)
    if cfg["use_feat_loss"]:                                                     # :560-573
        manifold_loss_feat = ntm.feature_space_loss(cfg["feat_k"], cfg["feat_sigma"], 17)(
            pred_u_strong_softmax, label_u_aug, insT) * cfg["feat_loss_weight"]
    if cfg["use_identity_loss"]:
        insT_identity_loss = ntm.Idenyity_loss()(insT, torch.eye(17, device=DEV)) * cfg["identity_loss_weight"]
    if cfg["use_3d_loss"]:
        raw = data_u["raw_pos"].contiguous()
        manifold_loss_3d = step.threed_loss(raw, label_u_aug, insT, nbr=step.threed_loss.neighbours(raw),
                                            order=ntm.spatial_order(raw)) * cfg["threed_loss_weight"]
    target = data["y"]
    criterion, criterion_u = crit(cfg["criterion"]), crit(cfg["criterion_u"])
    if cfg["criterion"] == "Weight_CELoss":                                      # :576-581
        sup_loss = criterion(pred_l, target, data["class_weights"])
    else:
        sup_loss = criterion(pred_l, target)
    if cfg["criterion_u"] == "Weight_CELoss_U":                                  # :584-596
        unsup_loss = criterion_u(pred_u_strong, label_u_aug.clone().detach(), data["class_weights"],
                                 logits_u_aug.clone().detach(), thresh=p_threshold)
    elif cfg["criterion_u"] == "Poly1FocalLoss_U":
        unsup_loss = criterion_u(pred_u_strong, label_u_aug.detach(), logits_u_aug.detach(), thresh=p_threshold, mask=None)
    elif cfg["criterion_u"] == "Poly1FocalLoss_U_corr":
        unsup_loss = criterion_u(pred_u_strong_corr, label_u_aug.detach(), logits_u_aug.detach(), thresh=p_threshold, mask=None)
    elif cfg["criterion_u"] == "Poly1FocalLoss_U_T":
        unsup_loss = criterion_u(pred_u_strong, label_u_aug.detach(), logits_u_aug.detach(), step.ema_t, pred_u_strong_corr,
                                 thresh=p_threshold, mask=None)
    thresh_mask = logits_u_aug.ge(torch.tensor(p_threshold))                     # :599-602
    scale_factor = (bu * n) / thresh_mask.sum()
    unsup_loss = unsup_loss * (cfg["unsupervised_loss_weight"] * scale_factor)
    loss = sup_loss + unsup_loss                                                 # :646-657
    out = {"sup": sup_loss.detach(), "unsup": unsup_loss.detach()}
    if cfg["use_feat_loss"]:
        loss = loss + manifold_loss_feat
        out["feat"] = manifold_loss_feat.detach()
    if cfg["use_identity_loss"]:
        loss = loss + insT_identity_loss
        out["identity"] = insT_identity_loss.detach()
    if cfg["use_3d_loss"]:
        loss = loss + manifold_loss_3d
    out["threed"] = manifold_loss_3d.detach() if cfg["use_3d_loss"] else torch.zeros((), device=DEV)
    loss.backward()
    step.optimizer.step()                                                        # :659-666
    step.optimizer.zero_grad(set_to_none=True)
    step.T_optimizer.step()
    step.T_optimizer.zero_grad(set_to_none=True)
    return dict(out, loss=loss.detach())


ALL_ON = dict(use_feat_loss=True, use_identity_loss=True, use_3d_loss=False)
SWITCHES = {"u": dict(criterion_u="Poly1FocalLoss_U"), "u_corr": dict(criterion_u="Poly1FocalLoss_U_corr"),
            "u_t": dict(criterion_u="Poly1FocalLoss_U_T"), "wce_u": dict(criterion_u="Weight_CELoss_U"),
            "wce": dict(criterion="Weight_CELoss"), "feat": dict(use_feat_loss=True), "identity": dict(use_identity_loss=True),
            "no3d": dict(use_3d_loss=False), "together": dict(ALL_ON, criterion="Weight_CELoss", criterion_u="Poly1FocalLoss_U_T")}


def _three(cfg, epoch, mode, batches):
    step = _new_step(cfg)
    step.set_epoch(epoch)
    torch.manual_seed(11)
    out = []
    for i in range(3):
        d, u = batches[i % 2]
        res = step(d, u) if mode == "step" else _composed(step, d, u)
        out.append({k: v.clone() for k, v in res.items()})
    torch.cuda.synchronize()
    return out, _state(step)


@pytest.fixture(scope="module")
def batches():
    return _batches()


@pytest.mark.parametrize("phase", ["teacher", "self"])
@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_three_iterations_equal_the_reference_statements(switch, phase, batches):
    from geot_amd import train_step as ts
    cfg = dict(ts.NTM_CFG, threed_k=8, feat_k=8, **SWITCHES[switch])
    epoch = cfg["switch_ep"] + (1 if phase == "self" else 0)
    a, sa = _three(cfg, epoch, "step", batches)
    b, sb = _three(cfg, epoch, "composed", batches)
    for i, (x, y) in enumerate(zip(a, b)):
        assert set(x) == set(y), (set(x), set(y))
        assert ("feat" in x) == cfg["use_feat_loss"] and ("identity" in x) == cfg["use_identity_loss"]
        for k in x:
            assert torch.isfinite(x[k]) and torch.equal(x[k], y[k]), (i, k, float(x[k]), float(y[k]))
    _same(sa, sb, "parameters / moments / ema_t")


def test_defaults_are_todays_step(batches):
    """Every new key at its default: the bits of a step built from the keys NTM_CFG had before the switches."""
    from geot_amd import train_step as ts
    new = ("criterion", "criterion_u", "use_3d_loss", "use_feat_loss", "feat_loss_weight", "feat_k", "feat_sigma",
           "use_identity_loss", "identity_loss_weight")
    old = {k: v for k, v in dict(ts.NTM_CFG, threed_k=8).items() if k not in new}
    for epoch in (50, 51):
        a, sa = _three(old, epoch, "step", batches)
        b, sb = _three(dict(ts.NTM_CFG, threed_k=8), epoch, "composed", batches)
        for x, y in zip(a, b):
            assert set(x) == {"loss", "sup", "unsup", "threed"} and all(torch.equal(x[k], y[k]) for k in x)
        _same(sa, sb, "defaults")


def test_supervised_step_with_weight_celoss(batches):
    from geot_amd import train_step as ts
    from geot_amd.openpoints.models.backbone.transformer import PointTransformer_seg_T
    torch.manual_seed(0)
    init = PointTransformer_seg_T(**SMALL).state_dict()
    runs = {}
    for mode in ("step", "composed"):
        m = PointTransformer_seg_T(**SMALL).to(DEV)
        m.load_state_dict(init)
        step = ts.SupervisedStep(m, criterion="Weight_CELoss")
        torch.manual_seed(11)
        losses = []
        for i in range(3):
            d = batches[i % 2][0]
            if mode == "step":
                losses.append(step(d["pos"], d["cls"], d["y"], class_weights=d["class_weights"]).clone())
            else:                                                                # train.py:441-452, 646-666
                m.train()
                logits = m(d["pos"], d["pos"].transpose(1, 2).contiguous(), d["cls"])[0]
                loss = crit("Weight_CELoss")(logits, d["y"], d["class_weights"])
                loss.backward()
                step.optimizer.step()
                step.optimizer.zero_grad(set_to_none=True)
                losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        runs[mode] = (losses, {k: v.clone() for k, v in m.state_dict().items()})
    assert all(torch.isfinite(a) and torch.equal(a, b) for a, b in zip(runs["step"][0], runs["composed"][0]))
    _same(runs["step"][1], runs["composed"][1], "supervised")
    with pytest.raises(RuntimeError, match="class_weights"):
        step(d["pos"], d["cls"], d["y"])


# ---- replay ------------------------------------------------------------------------------------------------------------------
def test_replay_of_two_switched_configurations_in_fast_launch_mode():
    """tests/_criteria_fast_check.py in its own process (the launch mode is read when HIP initialises): graphed == eager
    across switch_ep for _U_T + all three extra losses and for Weight_CELoss + Weight_CELoss_U without the 3-D loss, the
    supervised Weight_CELoss step too; every captured graph's node census is {"kernel"}."""
    env = {k: v for k, v in os.environ.items() if k != "DEBUG_CLR_GRAPH_PACKET_CAPTURE"}
    env["GEOT_GRAPH_LAUNCH"] = "fast"
    r = subprocess.run([sys.executable, os.path.join(HERE, "_criteria_fast_check.py")], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "criteria fast ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ---- meters ------------------------------------------------------------------------------------------------------------------
class AverageMeter:                       # openpoints/utils: val / sum / count / avg in Python floats
    def __init__(self):
        self.sum, self.count, self.avg = 0.0, 0, 0.0

    def update(self, val, n):
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


@pytest.mark.parametrize("on", [True, False])
def test_meters_carry_the_switched_losses(on, batches):
    from geot_amd import train_step as ts
    cfg = dict(ts.NTM_CFG, threed_k=8, feat_k=8, use_feat_loss=on, use_identity_loss=on)
    step = _new_step(cfg, meters=True)
    torch.manual_seed(11)
    want = {k: AverageMeter() for k in ("feat", "identity", "threed", "loss")}
    for i in range(3):
        d, u = batches[i % 2]
        res = step(d, u)
        for k, m in want.items():
            if k in res:
                m.update(res[k].item(), n=cfg["batch_size_u"] + (cfg["batch_size_l"] if k == "loss" else 0))
    stats = step.meters.read()[0]
    assert stats["iterations"] == 3 and stats["insT_threed_loss"] == want["threed"].avg and stats["train_loss"] == want["loss"].avg
    if on:
        assert want["feat"].avg != 0.0 and want["identity"].avg != 0.0
        assert stats["manifold_loss_feat"] == want["feat"].avg and stats["insT_identity_loss"] == want["identity"].avg
        assert stats["val"]["manifold_loss_feat"] == res["feat"].item() and stats["val"]["insT_identity_loss"] == res["identity"].item()
    else:
        assert stats["manifold_loss_feat"] == 0.0 and stats["insT_identity_loss"] == 0.0
