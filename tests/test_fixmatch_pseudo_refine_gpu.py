"""cfg pseudo_refine in the FixMatch+NTM step: an iteration with the refined mask equals the reference's statements composed
by hand on the step's own modules, with the mask built by the COMPOSITE pseudo_label_refine / _margin (train.py:500: the
`mask` the loop passes to its unsupervised criteria and never fills), bit for bit -- before and after switch_ep; the hipGraph
replay equals the eager step and holds kernel nodes only; "kept" is the mask's sum; the refusals.

The small model of tests/test_fixmatch_phase2_gpu.py, its classifier's last layer scaled so that a freshly initialised model
is confident at some points and not at others: with cfg threshold 0.9 both mask values occur, refined and unrefined (checked:
an empty threshold mask would make scale_factor infinite)."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_fixmatch_phase2_gpu import SMALL, _batch, _same, _state  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TH = 0.9
# measured on the freshly initialised small model: the eval-mode teacher (running statistics) puts 7 367 of 8 192 points at
# or above 0.9 at x 8 (none at x 3, all at x 24), the train-mode student 7 451 at x 24
HEAD_SCALE = {"teacher": 8.0, "student": 24.0}


def _cfg(**kw):
    from geot_amd import train_step as ts
    return dict(ts.NTM_CFG, threed_k=8, threshold=TH, **kw)


def _new_step(cfg):
    from geot_amd import train_step as ts
    torch.manual_seed(5)
    step = ts.build_fixmatch(DEV, seg_cfg=SMALL, cfg=cfg, use_ddp=False)
    with torch.no_grad():
        step.model.segmentor.seg_head[3].weight.mul_(HEAD_SCALE["student"])
        step.model_t.segmentor.seg_head[3].weight.mul_(HEAD_SCALE["teacher"])
    return step


@functools.lru_cache(maxsize=None)
def _batches():
    return [_batch(3), _batch(400)]


def _composed(step, data, data_u, seen):
    """examples/segmentation/train.py:460-666 for one iteration, statement by statement, on the step's own modules, with
    `mask` (:500) filled by the composite refinement of utils/pseudo_mask.py.  seen: gets the mask and the unrefined one."""
    from geot_amd import ntm
    from geot_amd.utils import pseudo_mask as pm
    cfg = step.cfg
    bl, bu, n = data["pos"].shape[0], data_u["pos_w"].shape[0], data["pos"].shape[1]
    p_threshold = cfg["threshold"]
    if not step.self_labelling:
        with torch.no_grad():
            step.model_t.eval()
            pred_u = F.softmax(step.model_t(data_u, if_teacher=True)[0], dim=1)
            logits_u_aug, label_u_aug = torch.max(pred_u, dim=1)
    step.model.train()
    step.T_predictor.train()
    data_u = dict(data_u, T=step.ema_t)
    pred_all, delta_T, sigma = step.model(data, u0=data_u, fixmatch=True)
    pred_l, pred_u_strong, pred_u_w = torch.split(pred_all, [bl, bu, pred_all.shape[0] - bl - bu])
    if step.self_labelling:
        pred_u = F.softmax(pred_u_w, dim=1)
        logits_u_aug, label_u_aug = torch.max(pred_u.detach(), dim=1)
    size, k = cfg["pseudo_refine_size"], cfg["pseudo_refine_neighbors"]
    if cfg["pseudo_refine"] in (True, "max"):
        mask = pm.pseudo_label_refine(pred_u.clone().detach(), p_threshold, data_u["pos_w"], size, k)
    else:
        mask = pm.pseudo_label_refine_margin(pred_u.clone().detach(), p_threshold, data_u["pos_w"], size, k)[0]
    ema_t_corr, ema_next, _, _ = ntm.class_transition(pred_u.clone().detach(), sigma, step.ema_t, cfg["geo_lambma"],
                                                      cfg["ema_t_decay"], filter_outlier=cfg["filter_outlier"])
    pred_u_strong_softmax = F.softmax(pred_u_strong, dim=1)
    insT = step.T_predictor(pred_u_strong_softmax.detach(), step.cm)
    pred_u_strong_corr = ntm.correct_logits(pred_u_strong, insT, ema_t_corr, cfg["lambma"])
    with torch.no_grad():
        step.ema_t.copy_(ema_next)
    raw = data_u["raw_pos"].contiguous()
    manifold_loss_3d = step.threed_loss(raw, label_u_aug, insT, nbr=step.threed_loss.neighbours(raw),
                                        order=ntm.spatial_order(raw)) * cfg["threed_loss_weight"]
    sup_loss = step.criterion(pred_l, data["y"])
    if cfg["criterion_u"] == "Poly1FocalLoss_U":
        unsup_loss = step.criterion_u(pred_u_strong, label_u_aug.detach(), logits_u_aug.detach(), thresh=p_threshold, mask=mask)
    elif cfg["criterion_u"] == "Poly1FocalLoss_U_corr":
        unsup_loss = step.criterion_u(pred_u_strong_corr, label_u_aug.detach(), logits_u_aug.detach(), thresh=p_threshold,
                                      mask=mask)
    else:
        unsup_loss = step.criterion_u(pred_u_strong, label_u_aug.detach(), logits_u_aug.detach(), step.ema_t,
                                      pred_u_strong_corr, thresh=p_threshold, mask=mask)
    thresh_mask = logits_u_aug.ge(torch.tensor(p_threshold))                     # :599-602: the UNrefined mask
    scale_factor = (bu * n) / thresh_mask.sum()
    unsup_loss = unsup_loss * (cfg["unsupervised_loss_weight"] * scale_factor)
    loss = sup_loss + unsup_loss + manifold_loss_3d
    loss.backward()
    step.optimizer.step()
    step.optimizer.zero_grad(set_to_none=True)
    step.T_optimizer.step()
    step.T_optimizer.zero_grad(set_to_none=True)
    seen.append((mask.clone(), thresh_mask.clone()))
    return {"loss": loss.detach(), "sup": sup_loss.detach(), "unsup": unsup_loss.detach(), "threed": manifold_loss_3d.detach(),
            "kept": mask.sum()}


@functools.lru_cache(maxsize=None)
def _one(refine, criterion_u, epoch, how):
    """One iteration of a fresh step -> (losses, state, [(mask, unrefined mask)] of the composition)."""
    step = _new_step(_cfg(pseudo_refine=refine, criterion_u=criterion_u))
    step.set_epoch(epoch)
    torch.manual_seed(11)
    d, u = _batches()[0]
    seen = []
    res = step(d, u) if how == "step" else _composed(step, d, u, seen)
    out = {k: v.clone() for k, v in res.items()}
    torch.cuda.synchronize()
    return out, _state(step), seen


CASES = [("max", "Poly1FocalLoss_U_corr", 50), ("margin", "Poly1FocalLoss_U_corr", 50), ("max", "Poly1FocalLoss_U_corr", 51),
         ("max", "Poly1FocalLoss_U", 50), ("margin", "Poly1FocalLoss_U_T", 51)]


@pytest.mark.parametrize("refine,criterion_u,epoch", CASES)
def test_an_iteration_equals_the_composition_with_the_composite_mask(refine, criterion_u, epoch):
    a, sa, _ = _one(refine, criterion_u, epoch, "step")
    b, sb, seen = _one(refine, criterion_u, epoch, "composed")
    mask, plain = seen[0]
    print("%s epoch %d: %d of %d kept, %d above the threshold unrefined, %d differ" % (
        refine, epoch, int(mask.sum()), mask.numel(), int(plain.sum()), int((mask != plain).sum())))
    assert 0 < int(mask.sum()) < mask.numel() and 0 < int(plain.sum()) and (mask != plain).any()
    assert set(a) == set(b) == {"loss", "sup", "unsup", "threed", "kept"}
    for k in a:
        assert torch.isfinite(a[k].float()) and torch.equal(a[k], b[k]), (k, float(a[k]), float(b[k]))
    _same(sa, sb, "parameters / moments / ema_t")


def test_kept_is_the_masks_sum_on_the_device():
    a, _, _ = _one("max", "Poly1FocalLoss_U_corr", 50, "step")
    _, _, seen = _one("max", "Poly1FocalLoss_U_corr", 50, "composed")
    assert a["kept"].is_cuda and a["kept"].dim() == 0 and int(a["kept"]) == int(seen[0][0].sum())


def test_refinement_changes_the_loss_and_off_returns_no_kept():
    on, _, _ = _one("max", "Poly1FocalLoss_U_corr", 50, "step")
    off, _, _ = _one(False, "Poly1FocalLoss_U_corr", 50, "step")
    assert "kept" not in off and set(off) == {"loss", "sup", "unsup", "threed"}
    assert torch.equal(on["sup"], off["sup"]) and not torch.equal(on["unsup"], off["unsup"])


def test_off_adds_no_launch(monkeypatch):
    from geot_amd.utils import pseudo_mask as pm
    calls = []
    monkeypatch.setattr(pm, "neighbours", lambda *a, **k: calls.append("neighbours"))
    monkeypatch.setattr(pm, "pseudo_refine_mask", lambda *a, **k: calls.append("pseudo_refine_mask"))
    step = _new_step(_cfg())
    assert step.refine_mode is None
    d, u = _batches()[0]
    out = step(d, u)
    pre = step.lookahead_work(d, u)
    torch.cuda.synchronize()
    assert not calls and "kept" not in out and pre.refine_nbr is None


def test_graphed_step_equals_eager_and_holds_kernel_nodes_only():
    from geot_amd import graph_step as gs
    cfg = _cfg(pseudo_refine="max")
    runs = {}
    for mode in ("eager", "graph"):
        step = _new_step(cfg)
        call = gs.GraphedFixMatchStep(step, warmup=1) if mode == "graph" else step
        call.set_epoch(1)
        torch.manual_seed(11)
        out = []
        for i in range(3):
            cur, nxt = _batches()[i % 2], _batches()[(i + 1) % 2]
            out.append({k: v.clone() for k, v in call(cur[0], cur[1], next_batches=nxt).items()})
        torch.cuda.synchronize()
        if mode == "graph":
            assert {"P", "M"} <= set(call.graphs) and call.captured, sorted(call.graphs)
            assert all(set(call.node_types[k]) == {"kernel"} for k in call.graphs), call.node_types
            assert call.pre.refine_nbr is not None and call.pre.refine_nbr.dtype == torch.int32
        runs[mode] = (out, _state(step))
    for i, (a, b) in enumerate(zip(runs["eager"][0], runs["graph"][0])):
        assert "kept" in a and set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (i, k, float(a[k]), float(b[k]))
    _same(runs["eager"][1], runs["graph"][1], "graph against eager")


def test_refusals():
    from geot_amd import train_step as ts
    with pytest.raises(ValueError, match="Weight_CELoss_U"):
        ts.build_fixmatch(DEV, seg_cfg=SMALL, cfg=_cfg(pseudo_refine="max", criterion_u="Weight_CELoss_U"), use_ddp=False)
    with pytest.raises(ValueError, match="pseudo_refine"):
        ts.build_fixmatch(DEV, seg_cfg=SMALL, cfg=_cfg(pseudo_refine="median"), use_ddp=False)
    step = _new_step(_cfg(pseudo_refine="max", pseudo_refine_size=32, pseudo_refine_neighbors=2))
    d, u = _batches()[0]
    small_u = {k: (v[:, :32].contiguous() if v.dim() == 3 and v.shape[1] == 4096 else v) for k, v in u.items()}
    with pytest.raises(RuntimeError, match="no 32 nearest other points"):            # N >= size + 1, at the first batch
        step._refine_neighbours(small_u)
