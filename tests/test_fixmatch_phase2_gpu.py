"""FixMatchNTMStep after switch_ep (examples/segmentation/train.py:469-475, 494-498): the pseudo labels come from the
soft-max of the student's own weak-view slice and the frozen teacher no longer runs.  An eager phase-2 iteration equals the
reference's statements composed with the step's stages, bit for bit; a step whose epoch is never set, or set at or below
switch_ep, is the teacher's step it always was; and the hipGraph replay (GraphedFixMatchStep) equals the eager step across
the switch, with and without the look-ahead, its phase-2 graphs kernel-only in fast launch mode."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

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
             "x_s": strong.transpose(1, 2).contiguous(), "cls_s": z, "raw_pos": unl})


def _state(step):
    out = {"ema_t": step.ema_t.detach().clone()}
    for name, mod in (("model", step.model), ("T", step.T_predictor)):
        out.update({name + "." + k: v.detach().clone() for k, v in mod.state_dict().items()})
    for i, opt in enumerate(step.optimizers()):
        for j, p in enumerate(pp for g in opt.param_groups for pp in g["params"]):
            for k, v in opt.state.get(p, {}).items():
                if torch.is_tensor(v):
                    out["opt%d.%d.%s" % (i, j, k)] = v.detach().clone()
    return out


def _same(a, b, what):
    assert set(a) == set(b), what
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, (what, len(bad), bad[:8])


def _new_step(cfg):
    from geot_amd import train_step as ts
    torch.manual_seed(5)
    return ts.build_fixmatch(DEV, seg_cfg=SMALL, cfg=cfg, use_ddp=False)


def _composed_phase2(step, data, data_u):
    """One iteration for epoch > switch_ep spelled out: train.py:486-500 for the student's forward and its own pseudo labels,
    then the step's stages 3-5 (class transition, T_predictor, corrected logits, losses, backward, both optimisers)."""
    from geot_amd import ntm
    cfg = step.cfg
    bl, bu, n = data["pos"].shape[0], data_u["pos_w"].shape[0], data["pos"].shape[1]
    step.model.train()
    step.T_predictor.train()
    data_u = dict(data_u, T=step.ema_t)
    pred_all, delta_T, sigma = step.model(data, u0=data_u, fixmatch=True)
    pred_l, pred_u_strong, pred_u = torch.split(pred_all, [bl, bu, pred_all.shape[0] - bl - bu])
    pred_u = F.softmax(pred_u, dim=1)
    logits_u_aug, label_u_aug = torch.max(pred_u.detach(), dim=1)
    ema_t_corr, ema_next, _, _ = ntm.class_transition(pred_u.clone().detach(), sigma, step.ema_t, cfg["geo_lambma"],
                                                      cfg["ema_t_decay"], filter_outlier=cfg["filter_outlier"])
    ins_t = step.T_predictor(F.softmax(pred_u_strong, dim=1).detach(), step.cm)
    corr = ntm.correct_logits(pred_u_strong, ins_t, ema_t_corr, cfg["lambma"])
    with torch.no_grad():
        step.ema_t.copy_(ema_next)
    raw = data_u["raw_pos"].contiguous()
    loss_3d = step.threed_loss(raw, label_u_aug, ins_t, nbr=step.threed_loss.neighbours(raw),
                               order=ntm.spatial_order(raw)) * cfg["threed_loss_weight"]
    sup = step.criterion(pred_l, data["y"])
    unsup = step.criterion_u(corr, label_u_aug.detach(), logits_u_aug.detach(), thresh=cfg["threshold"])
    mask = logits_u_aug.ge(cfg["threshold"])
    unsup = unsup * (cfg["unsupervised_loss_weight"] * (bu * n) / mask.sum())
    loss = sup + unsup + loss_3d
    loss.backward()
    step.optimizer.step()
    step.optimizer.zero_grad(set_to_none=True)
    step.T_optimizer.step()
    step.T_optimizer.zero_grad(set_to_none=True)
    return {"loss": loss.detach(), "sup": sup.detach(), "unsup": unsup.detach(), "threed": loss_3d.detach()}


def _count_teacher(step):
    calls = [0]
    step.model_t.register_forward_hook(lambda *a: calls.__setitem__(0, calls[0] + 1))
    return calls


def test_a_phase2_iteration_equals_the_reference_composition():
    from geot_amd import train_step as ts
    cfg = dict(ts.NTM_CFG, threed_k=8)
    batches = [_batch(3), _batch(400)]
    runs = {}
    for mode in ("step", "composed"):
        step = _new_step(cfg)
        teacher = _count_teacher(step)
        step.set_epoch(cfg["switch_ep"] + 1)
        assert step.self_labelling
        torch.manual_seed(11)
        out = []
        for i in range(3):
            d, u = batches[i % 2]
            res = step(d, u) if mode == "step" else _composed_phase2(step, d, u)
            out.append({k: v.clone() for k, v in res.items()})
        torch.cuda.synchronize()
        assert teacher[0] == 0, "the teacher ran after switch_ep"
        runs[mode] = (out, _state(step))
    for i, (a, b) in enumerate(zip(runs["step"][0], runs["composed"][0])):
        for k in a:
            assert torch.equal(a[k], b[k]), (i, k, float(a[k]), float(b[k]))
    _same(runs["step"][1], runs["composed"][1], "parameters / moments / ema_t")


def test_at_or_before_switch_ep_the_step_is_the_teachers():
    """Never set, set to switch_ep or to an early epoch: the same bits, and the teacher runs every iteration."""
    from geot_amd import train_step as ts
    cfg = dict(ts.NTM_CFG, threed_k=8)
    batches = [_batch(3), _batch(400)]
    runs = {}
    for epoch in (None, cfg["switch_ep"], 1):
        step = _new_step(cfg)
        teacher = _count_teacher(step)
        if epoch is not None:
            step.set_epoch(epoch)
        assert not step.self_labelling
        torch.manual_seed(11)
        out = []
        for i in range(3):
            cur, nxt = batches[i % 2], batches[(i + 1) % 2]
            out.append({k: v.clone() for k, v in step(cur[0], cur[1], next_batches=nxt).items()})
        torch.cuda.synchronize()
        assert teacher[0] == 3
        runs[epoch] = (out, _state(step))
    for epoch in (cfg["switch_ep"], 1):
        for i, (a, b) in enumerate(zip(runs[None][0], runs[epoch][0])):
            assert all(torch.equal(a[k], b[k]) for k in a), (epoch, i)
        _same(runs[None][1], runs[epoch][1], epoch)


EPOCHS = [50, 50, 50, 50, 51, 51, 51, 51]    # four iterations with the teacher, four without: with warmup=2 the graphed step
                                              # captures and replays P / M before the switch and P@2 / M@2 after it


@pytest.mark.parametrize("look", [True, False])
def test_graphed_equals_eager_across_the_switch(look):
    from geot_amd import train_step as ts, graph_step as gs
    cfg = dict(ts.NTM_CFG, threed_k=8)
    batches = [_batch(3), _batch(400)]
    runs = {}
    for mode in ("eager", "graph"):
        step = _new_step(cfg)
        teacher = _count_teacher(step)
        call = gs.GraphedFixMatchStep(step, warmup=2) if mode == "graph" else step
        torch.manual_seed(11)
        out, seen = [], []
        for i, epoch in enumerate(EPOCHS):
            if mode == "graph" and epoch > cfg["switch_ep"] and not step.self_labelling:
                assert {"P", "M"} <= set(call.graphs) and call.captured, sorted(call.graphs)   # replayed before the switch
            call.set_epoch(epoch)
            cur, nxt = batches[i % 2], batches[(i + 1) % 2]
            res = call(cur[0], cur[1], next_batches=nxt if look else None)
            out.append({k: v.clone() for k, v in res.items()})
            seen.append(teacher[0])
        torch.cuda.synchronize()
        assert seen[4:] == [seen[3]] * 4, seen          # no teacher forward after the switch (nor a replayed one: no P)
        if mode == "graph":
            assert {"P@2", "M@2"} <= set(call.graphs), sorted(call.graphs)
            assert all(set(call.node_types[k]) == {"kernel"} for k in ("P@2", "M@2")), call.node_types
        runs[mode] = (out, _state(step))
    for i, (a, b) in enumerate(zip(runs["eager"][0], runs["graph"][0])):
        for k in a:
            assert torch.equal(a[k], b[k]), (i, k, float(a[k]), float(b[k]))
    _same(runs["eager"][1], runs["graph"][1], "graph against eager")


def test_phase2_graphs_are_kernel_only_in_fast_launch_mode():
    """GEOT_GRAPH_LAUNCH=fast (packet capture on): the wrapper refuses any graph that is not kernel nodes alone, so the
    phase-2 graphs capturing there -- and replaying to the eager step's bits -- is the check (tests/_phase2_fast_check.py,
    its own process: the switch is read when HIP initialises)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "DEBUG_CLR_GRAPH_PACKET_CAPTURE"}
    env["GEOT_GRAPH_LAUNCH"] = "fast"
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_phase2_fast_check.py")], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "phase2 fast ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
