"""cfg use_contrastive in the FixMatch+NTM step: with the switch off the step is the one without the keys, bit for bit; with
it on, "contrast" is nativeContrastLoss_t called by hand on the tapped head features with the same seed and counter, the
total is the sum in the stated order and the head receives another gradient -- before and after switch_ep; the hipGraph
replay equals the eager step (state, bank, pointer, counter) and holds kernel nodes only; the refusals.

The small model of tests/test_fixmatch_phase2_gpu.py with its classifier's last layer scaled as in
tests/test_fixmatch_pseudo_refine_gpu.py, here so that at cur_threshold 0.9 SOME points of each cloud pass and fewer than
contrast_samples in at least one cloud: 0 < anchors < B_u * S is asserted wherever a loss is read."""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_fixmatch_phase2_gpu import SMALL, _batch, _same, _state  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TH = 0.9
S = 512
WEIGHT = 0.5
# measured on the freshly initialised small model, points of a 4 096-point cloud at or above 0.9: the eval-mode teacher at
# x 4 puts 271 / 611 (first batch) and 455 / 385 (second) there, 1 277 / 1 704 at x 5; the train-mode student at x 1.5
# between 309 and 397 over three iterations, 846 / 759 at x 2
HEAD_SCALE = {"teacher": 4.0, "student": 1.5}


def _cfg(**kw):
    from geot_amd import train_step as ts
    return dict(ts.NTM_CFG, threed_k=8, threshold=TH, **kw)


def _on(**kw):
    return _cfg(use_contrastive=True, contrast_samples=S, contrastive_loss_weight=WEIGHT, contrast_seed=7, **kw)


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


def _counter(step):
    return int(step.contrast.draw_counter.item()) & 0xFFFFFFFFFFFFFFFF


def _contrast_state(step):
    c = step.contrast
    return {"bank": c.point_queue.clone(), "ptr": c.point_queue_ptr.clone(), "counter": c.draw_counter.clone()}


def test_switch_off_is_the_step_without_the_keys():
    from geot_amd import train_step as ts
    keys = ("use_contrastive", "contrastive_loss_weight", "cur_threshold", "contrast_samples", "contrast_seed")
    runs = []
    for cfg in (_cfg(), {k: v for k, v in _cfg().items() if k not in keys}):
        step = _new_step(cfg)
        assert step.contrast is None and not step.model.segmentor.keep_head_feature and step.model.segmentor.head_feature is None
        torch.manual_seed(11)
        out = [{k: v.clone() for k, v in step(*_batches()[i]).items()} for i in range(2)]
        torch.cuda.synchronize()
        assert step.model.segmentor.head_feature is None and step.model_t.segmentor.head_feature is None
        runs.append((out, _state(step)))
    assert ts.NTM_CFG["use_contrastive"] is False
    for a, b in zip(runs[0][0], runs[1][0]):
        assert set(a) == set(b) == {"loss", "sup", "unsup", "threed"}
        assert all(torch.equal(a[k], b[k]) for k in a)
    _same(runs[0][1], runs[1][1], "switch off against no keys")


def _run(cfg, epoch, record=None):
    """Two iterations of a fresh step -> (losses per iteration, state, seg_head[0] weight gradients per iteration)."""
    step = _new_step(cfg)
    step.set_epoch(epoch)
    grads = []
    step.model.segmentor.seg_head[0].weight.register_hook(lambda g: grads.append(g.clone()))
    if record is not None and step.contrast is not None:
        inner = step.contrast.forward

        def forward(feat_s, score, feat_t, **kw):
            record.append({"feat_s": feat_s, "score": score.clone(), "feat_t": feat_t.clone(), "kw": kw,
                           "before": _contrast_state(step), "counter": _counter(step)})
            return inner(feat_s, score, feat_t, **kw)
        step.contrast.forward = forward
    torch.manual_seed(11)
    out = [{k: v.clone() for k, v in step(*_batches()[i]).items()} for i in range(2)]
    torch.cuda.synchronize()
    return out, _state(step), grads, step


@pytest.mark.parametrize("epoch", [50, 51])
def test_switch_on_adds_the_modules_loss_last(epoch):
    from geot_amd.utils.cluster_contrastloss import nativeContrastLoss_t
    from geot_amd.openpoints.dataset.sample_draw import DeviceDraws
    seen = []
    on, _, grads_on, step = _run(_on(), epoch, seen)
    off, _, grads_off, _ = _run(_cfg(), epoch)
    bl = bu = 2
    assert len(seen) == 2 and seen[0]["counter"] == 0 and seen[1]["counter"] == bu + 1 == _counter(step) - (bu + 1)
    for i, (a, rec) in enumerate(zip(on, seen)):
        assert set(a) == {"loss", "sup", "unsup", "threed", "contrast", "anchors"}
        n_anchors = int(a["anchors"])
        print("epoch %d iteration %d: %d anchors, per cloud at or above %.1f: %s" % (
            epoch, i, n_anchors, TH, (rec["score"] >= TH).sum(1).tolist()))
        assert a["anchors"].is_cuda and 0 < n_anchors < bu * S
        assert n_anchors == int((rec["score"] >= TH).sum(1).clamp(max=S).sum())
        # what the loss read: the student's strong-view slice of the tapped feature, in place and channel-first ...
        feat_all = rec["feat_s"]._base
        assert rec["kw"] == {"channels_first": True} and tuple(feat_all.shape) == (bl + 2 * bu, 128, 4096)
        assert rec["feat_s"].data_ptr() == feat_all[bl].data_ptr() and rec["feat_s"].requires_grad
        assert not rec["feat_t"].requires_grad and tuple(rec["feat_t"].shape) == (bu, 128, 4096)
        if epoch > 50:          # ... against the student's own weak-view slice, detached
            assert torch.equal(rec["feat_t"], feat_all[bl + bu:].detach())
        elif i == 0:            # ... against the frozen teacher's feature of its weak-view forward
            with torch.no_grad():
                step.model_t.eval()
                step.model_t(_batches()[0][1], if_teacher=True)
            assert torch.equal(rec["feat_t"], step.model_t.segmentor.head_feature)
            step.model_t.segmentor.head_feature = None
        # the module by hand: the same seed, counter, bank and pointer
        hand = nativeContrastLoss_t(S, 128, TH, DEV, DeviceDraws(7, rec["counter"]), bank=rec["before"]["bank"].cpu())
        hand.point_queue_ptr.copy_(rec["before"]["ptr"])
        loss = hand(rec["feat_s"].detach().contiguous(), rec["score"], rec["feat_t"], channels_first=True)[0]
        assert torch.equal(loss, a["contrast"]) and float(loss) > 0 and int(hand.anchors) == n_anchors
        # the total: the stated order, the contrastive term last
        assert torch.equal(a["loss"], a["sup"] + a["unsup"] + a["threed"] + WEIGHT * a["contrast"])
    assert all(torch.equal(on[0][k], off[0][k]) for k in ("sup", "unsup", "threed"))          # the same first forward
    assert not torch.equal(on[0]["loss"], off[0]["loss"])
    assert len(grads_on) == len(grads_off) == 2 and not torch.equal(grads_on[0], grads_off[0])


@pytest.mark.parametrize("epoch", [1, 51])
def test_graphed_step_equals_eager_and_holds_kernel_nodes_only(epoch):
    from geot_amd import graph_step as gs
    runs = {}
    for mode in ("eager", "graph"):
        step = _new_step(_on())
        call = gs.GraphedFixMatchStep(step, warmup=1) if mode == "graph" else step
        call.set_epoch(epoch)
        torch.manual_seed(11)
        out = []
        for i in range(3):
            cur, nxt = _batches()[i % 2], _batches()[(i + 1) % 2]
            out.append({k: v.clone() for k, v in call(cur[0], cur[1], next_batches=nxt).items()})
        torch.cuda.synchronize()
        if mode == "graph":
            assert call.captured and all(set(call.node_types[k]) == {"kernel"} for k in call.graphs), call.node_types
            assert (call.pre.feat_t is not None) == (epoch <= 50)
        runs[mode] = (out, dict(_state(step), **_contrast_state(step)))
    for i, (a, b) in enumerate(zip(runs["eager"][0], runs["graph"][0])):
        assert "contrast" in a and set(a) == set(b) and 0 < int(a["anchors"]) < 2 * S
        for k in a:
            assert torch.equal(a[k], b[k]), (i, k, float(a[k]), float(b[k]))
    assert int(runs["eager"][1]["counter"]) == 9
    _same(runs["eager"][1], runs["graph"][1], "graph against eager")


def test_refusals():
    from geot_amd import train_step as ts
    for bad in (dict(use_contrastive=1), dict(use_contrastive=True, contrast_samples=2048),
                dict(use_contrastive=True, cur_threshold=0.0), dict(use_contrastive=True, contrastive_loss_weight=-1.0)):
        with pytest.raises((TypeError, ValueError), match="contrast|cur_threshold"):
            ts.build_fixmatch(DEV, seg_cfg=SMALL, cfg=_cfg(**bad), use_ddp=False)
    step = _new_step(_on())
    d, u = _batches()[0]
    pre = step.lookahead_work(d, u)
    assert tuple(pre.feat_t.shape) == (2, 128, 4096) and not pre.feat_t.requires_grad
    pre.feat_t = pre.feat_t.clone().requires_grad_(True)
    with pytest.raises(ValueError, match="feat_t"):
        step.student_iteration(d, u, pre)
