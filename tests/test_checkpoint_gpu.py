"""Save and resume, bit for bit (geot_amd/checkpoint.py): k calls, save, load, k more calls give the bits of 2k calls -- for
the eager steps into fresh objects, and for the replayed steps into the very wrapper whose graphs are captured.  The small
segmentor of tests/test_fixmatch_phase2_gpu.py, 2 + 2 clouds of 4096 points; every comparison is bitwise."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

SMALL = dict(trans_dim=384, depth=3, num_heads=4, group_size=32, num_group=128, encoder_dims=256, nclasses=17,
             drop_path_rate=0.1, downsample_targets=[2048, 1024, 512], extract_layers=[1, 2, 3])
WIDE = dict(threed_k=8, use_contrastive=True, contrast_samples=256, cur_threshold=0.05, ema_teacher=True, grad_norm_clip=1.0,
            step_per_update=2, filter_outlier=True)          # (cur_threshold: a random teacher is never 0.9 sure: anchors exist)


def _batch(seed, n=4096):
    from geot_amd.synth import make_batch, region_labels
    xl, xu = make_batch(2, n, start_index=seed)[0], make_batch(2, n, start_index=seed + 50)[0]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    lab, unl, strong = T(xl), T(xu), T(xu * np.float32(1.04))
    z = torch.zeros(2, 1, dtype=torch.long, device=DEV)
    return ({"pos": lab, "x": lab.transpose(1, 2).contiguous(), "cls": z, "y": T(region_labels(xl))},
            {"pos_w": unl, "x_w": unl.transpose(1, 2).contiguous(), "cls_w": z, "pos_s": strong,
             "x_s": strong.transpose(1, 2).contiguous(), "cls_s": z, "raw_pos": unl, "y": T(region_labels(xu))})


@pytest.fixture(scope="module")
def batches():
    return [_batch(3), _batch(400), _batch(90)]


@pytest.fixture(scope="module")
def sup_batches():
    from geot_amd.synth import make_batch, region_labels
    out = []
    for start in (0, 40, 90):
        xyz = make_batch(2, 4096, start_index=start)[0]
        out.append((torch.from_numpy(xyz).to(DEV), torch.zeros(2, 1, dtype=torch.long, device=DEV),
                    torch.from_numpy(region_labels(xyz)).to(DEV)))
    return out


def _new_step(cfg, seed, meters=None, tensor_lr=False):
    from geot_amd import train_step as ts
    torch.manual_seed(seed)
    step = ts.build_fixmatch(DEV, seg_cfg=SMALL, cfg=dict(ts.NTM_CFG, **cfg), use_ddp=False, meters=meters)
    if tensor_lr:
        _tensor_lr(step)
    return step


def _tensor_lr(step, value=1e-3):
    for opt in step.optimizers():
        for group in opt.param_groups:
            group["lr"] = torch.tensor(value, dtype=torch.float32, device=DEV)


def _lrs(step):
    return [group["lr"] for opt in step.optimizers() for group in opt.param_groups]


def flat(obj, prefix=""):
    """{path: leaf} of a tree of dicts and lists."""
    if isinstance(obj, dict):
        return {k2: v2 for k, v in obj.items() for k2, v2 in flat(v, "%s.%s" % (prefix, k)).items()}
    if isinstance(obj, (list, tuple)):
        return {k2: v2 for i, v in enumerate(obj) for k2, v2 in flat(v, "%s[%d]" % (prefix, i)).items()}
    return {prefix: obj}


def snap(obj):
    """A deep copy of such a tree (tensors cloned)."""
    if isinstance(obj, dict):
        return {k: snap(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [snap(v) for v in obj]
    return obj.detach().clone() if torch.is_tensor(obj) else obj


def _bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


HOST_VIEW = (".tail._calls", ".tail._pending")
# The tail's host-side view of its window is advanced by calls that run in python, not by replays (geot_amd/optim_tail.py:
# the device counter `window` and the accumulator are the state; a load takes the host's count from `window`).  Behind
# replays two runs therefore agree in every tensor and need not agree in that view: the replay tests leave it out.


def same(a, b, what, ignore=()):
    """Two trees hold the same leaves: tensors bit for bit (shape and dtype too), everything else equal (nan = nan)."""
    a, b = ({k: v for k, v in flat(t).items() if not k.startswith(tuple(ignore))} if ignore else flat(t) for t in (a, b))
    assert set(a) == set(b), (what, sorted(set(a) ^ set(b))[:8])
    bad = []
    for k, x in a.items():
        y = b[k]
        if torch.is_tensor(x) or torch.is_tensor(y):
            ok = torch.is_tensor(x) and torch.is_tensor(y) and x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x), _bits(y))
        else:
            ok = x == y or (isinstance(x, float) and isinstance(y, float) and x != x and y != y)
        if not ok:
            bad.append(k)
    assert not bad, (what, len(bad), bad[:8])


def _fix_calls(call, batches, first, count, look=False):
    out = []
    for i in range(first, first + count):
        cur, nxt = batches[i % 3], batches[(i + 1) % 3]
        res = call(cur[0], cur[1], next_batches=nxt) if look else call(cur[0], cur[1])
        out.append({k: v.clone() for k, v in res.items()})
    return out


# ---- 1, 2: eager, fresh objects, the widest cfg -- fused tail and torch form ---------------------------------------------------
@pytest.fixture(scope="module", params=[True, False], ids=["fused", "torch"])
def eager_run(request, batches, tmp_path_factory):
    """5 calls (the save falls inside an open window of 2), save, 4 more: the uninterrupted run."""
    from geot_amd import checkpoint as ck
    cfg = dict(WIDE, fused_tail=request.param)
    step = _new_step(cfg, 5, meters=True)
    torch.manual_seed(11)
    _fix_calls(step, batches, 0, 5)
    path = tmp_path_factory.mktemp("ckpt") / "eager.pt"
    ck.save(path, step, rng_device=DEV, epoch=0)
    at_save = snap(step.state_dict())
    losses = _fix_calls(step, batches, 5, 4)
    return {"cfg": cfg, "fused": request.param, "path": path, "step": step, "at_save": at_save, "losses": losses,
            "final": snap(step.state_dict()), "meters": snap(step.meters.read())}


def test_eager_resume_into_fresh_objects(eager_run, batches):
    from geot_amd import checkpoint as ck
    run = eager_run
    saved = run["at_save"]
    if run["fused"]:
        assert int(saved["tail"]["window"]) == 1 and saved["tail"]["_calls"] == 1 and saved["grads"] is None      # an open window
        assert bool(saved["tail"]["accumulator"].any())
    else:
        assert saved["window_calls"] == 1 and saved["tail"] is not None          # (the composite tail runs the teacher's EMA)
        # .grad carries the window: one for every parameter the optimizers hold state for
        assert len(saved["grads"]["model"]) == len(saved["optimizer"]["state"]) > 0
        assert len(saved["grads"]["T_predictor"]) == len(saved["T_optimizer"]["state"]) > 0
    assert bool((saved["contrast"]["point_queue_ptr"] > 0).all()) and int(saved["meters"]["i64"][4]) == 5
    step = _new_step(run["cfg"], 77, meters=True)          # other weights, another bank, no optimizer state yet
    torch.manual_seed(123)
    assert ck.load(run["path"], step) == {"epoch": 0}
    same(step.state_dict(), saved, "right after the load")
    losses = _fix_calls(step, batches, 5, 4)
    same(losses, run["losses"], "losses")
    same(step.state_dict(), run["final"], "the state 4 calls later")
    same(step.meters.read(), run["meters"], "meters.read()")
    # the teacher moved, and the run did not stand still
    moved = [k for k, v in saved["model_t"].items() if not torch.equal(v, run["final"]["model_t"][k])]
    assert len(moved) > len(saved["model_t"]) // 2, len(moved)


def test_a_saved_file_loads_with_weights_only(eager_run):
    state = torch.load(eager_run["path"], map_location="cpu", weights_only=True)
    assert set(state) == {"format", "step", "draws", "rng", "extra"} and state["extra"] == {"epoch": 0}
    kinds = (int, float, str, bool, type(None), torch.Tensor)
    odd = [k for k, v in flat(state).items() if not isinstance(v, kinds)]
    assert not odd, odd[:8]
    for name in ("optimizer", "T_optimizer"):
        assert all(isinstance(g["lr"], float) for g in state["step"][name]["param_groups"])
    assert state["rng"]["cuda"]["device"] == str(DEV)
    # torch's own optimizer still loads the entry (geot_amd/optim_tail.py's promise)
    step = eager_run["step"]
    plain = torch.optim.AdamW([{"params": list(g["params"])} for g in step.optimizer.param_groups])
    plain.load_state_dict(state["step"]["optimizer"])


def test_state_dict_returns_copies(eager_run, batches):
    step = eager_run["step"]
    state = step.state_dict()
    kept = snap(state)
    live = {t.data_ptr() for m in (step.model, step.model_t, step.T_predictor) for t in m.state_dict().values()}
    live |= {v.data_ptr() for opt in step.optimizers() for st in opt.state.values() for v in st.values() if torch.is_tensor(v)}
    live |= {step.ema_t.data_ptr(), step.cm.data_ptr(), step.contrast.point_queue.data_ptr(), step.meters.f64.data_ptr()}
    shared = [k for k, v in flat(state).items() if torch.is_tensor(v) and v.numel() and v.data_ptr() in live]
    assert not shared, shared[:8]
    _fix_calls(step, batches, 9, 2)          # an update call among them
    same(state, kept, "a state taken before two further calls")
    assert not torch.equal(_bits(step.ema_t), _bits(kept["ema_t"]))


def test_refusals_name_the_key_and_write_nothing(eager_run, monkeypatch):
    step = eager_run["step"]
    good = torch.load(eager_run["path"], map_location="cpu", weights_only=True)["step"]
    before = snap(step.state_dict())

    def bad(edit):
        state = snap(good)
        edit(state)
        return state
    cases = [
        (bad(lambda s: s["layout"].__setitem__("num_classes", 5)), "num_classes"),
        (bad(lambda s: (s["layout"].__setitem__("use_contrastive", False), s.__setitem__("contrast", None))), "use_contrastive"),
        (bad(lambda s: s.__setitem__("contrast", None)), "contrast"),
        (bad(lambda s: s.pop("T_optimizer")), "T_optimizer"),
        (bad(lambda s: s["optimizer"]["state"].pop(sorted(s["optimizer"]["state"])[-1])), r"optimizer\.state"),
        (bad(lambda s: s.__setitem__("ema_t", torch.zeros(3, 3))), "ema_t"),
        (bad(lambda s: s["meters"].__setitem__("f64", torch.zeros(7, dtype=torch.float64))), r"meters\.f64"),          # the last part checked
        (bad(lambda s: s["model"].__setitem__("surplus.weight", torch.zeros(1))), r"surplus\.weight"),
        (bad(lambda s: s["contrast"].__setitem__("point_queue_ptr", torch.zeros(1, dtype=torch.int32))), "point_queue_ptr"),
        (bad(lambda s: s.__setitem__("format", 0)), "format"),
    ]
    for state, name in cases:
        with pytest.raises(ValueError, match=name):
            step.load_state_dict(state)
    same(step.state_dict(), before, "after ten refused loads")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)          # (as tests/test_accumulate_gpu.py does)
    for part in (step, step.tail, step.meters, step.contrast):
        with pytest.raises(RuntimeError, match="stream capture"):
            part.state_dict()
    monkeypatch.undo()
    same(step.state_dict(), before, "after a refused state_dict()")


# ---- 3, 4: replayed -- into the same wrapper, and into fresh objects -----------------------------------------------------------
GRAPH_CFG = dict(threed_k=8, fused_tail=True, step_per_update=2, use_contrastive=True, contrast_samples=256, cur_threshold=0.05)


@pytest.fixture(scope="module")
def replayed_run(batches, tmp_path_factory):
    """4 calls with look-ahead (two warm-up calls, the capture, a replay), state_dict() and a file, 3 replays."""
    from geot_amd import checkpoint as ck, graph_step as gs
    step = _new_step(GRAPH_CFG, 5, tensor_lr=True)
    call = gs.GraphedFixMatchStep(step, warmup=2)
    torch.manual_seed(11)
    _fix_calls(call, batches, 0, 4, look=True)
    assert call.captured and {"P", "M"} <= set(call.graphs)
    state, rng = call.state_dict(), ck.rng_state(DEV)
    path = tmp_path_factory.mktemp("ckpt") / "replayed.pt"
    ck.save(path, call, rng_device=DEV)
    losses = _fix_calls(call, batches, 4, 3, look=True)
    return {"call": call, "state": state, "rng": rng, "path": path, "losses": losses, "final": snap(call.state_dict())}


def test_replayed_resume_into_the_same_wrapper(replayed_run, batches):
    from geot_amd import checkpoint as ck
    run = replayed_run
    call, step = run["call"], run["call"].step
    graphs = {k: v[0] for k, v in call.graphs.items()}
    eager_runs = dict(call._eager_runs)
    lrs = _lrs(step)
    assert int(run["state"]["tail"]["window"]) == 0 and call._pending          # (4 calls: two windows; a look-ahead is in flight)
    for lr in lrs:
        lr.fill_(0.25)          # the load puts the saved 1e-3 back, into these very tensors
    call.load_state_dict(run["state"])
    ck.set_rng_state(run["rng"])
    assert call._pre_next is None and call._announced is None and not call._pending          # the look-ahead in flight: dropped
    assert step.tail._calls == int(step.tail.window) == 0          # the host's count: taken from the device counter
    assert all(a is b for a, b in zip(lrs, _lrs(step)))
    same(call.state_dict(), run["state"], "right after the load", ignore=HOST_VIEW)
    losses = _fix_calls(call, batches, 4, 3, look=True)
    same(losses, run["losses"], "losses")
    same(call.state_dict(), run["final"], "the state 3 replays later", ignore=HOST_VIEW)
    assert call.captured and set(call.graphs) == set(graphs) and all(call.graphs[k][0] is g for k, g in graphs.items())
    assert call._eager_runs == eager_runs          # nothing ran eagerly, nothing was captured anew
    # the captured update reads the restored lr tensors: at lr 0 an update moves no weight (and the step counters go on)
    for lr in lrs:
        lr.fill_(0.0)
    weights = snap(dict(step.model.state_dict(keep_vars=False)))
    params = {k: v for k, v in weights.items() if k in dict(step.model.named_parameters())}
    steps = step.tail.steps.clone()
    _fix_calls(call, batches, 7, 2, look=True)          # calls 8 and 9 of the run: call 8 closes a window
    same({k: v for k, v in step.model.state_dict().items() if k in params}, params, "weights under lr = 0")
    assert float((step.tail.steps - steps).max()) == 1.0


def test_replayed_resume_into_fresh_objects(replayed_run, batches):
    """The new wrapper's warm-up calls are real calls: call for call the bits of the uninterrupted replays."""
    from geot_amd import checkpoint as ck, graph_step as gs
    run = replayed_run
    step = _new_step(GRAPH_CFG, 77, tensor_lr=True)
    torch.manual_seed(123)
    ck.load(run["path"], step)
    call = gs.GraphedFixMatchStep(step, warmup=2)          # (it marks the optimizers' groups capturable, as the saved ones are)
    same(call.state_dict(), run["state"], "right after the load", ignore=HOST_VIEW)
    losses = _fix_calls(call, batches, 4, 3, look=True)
    assert call.captured
    same(losses, run["losses"], "losses")
    same(call.state_dict(), run["final"], "the state 3 calls later", ignore=HOST_VIEW)


# ---- 5: across switch_ep ---------------------------------------------------------------------------------------------------------
def test_resume_across_switch_ep(batches, tmp_path):
    """Saved at switch_ep inside an open window, resumed into the epoch after it: the epoch comes back without
    restart_window(), and set_epoch() then restarts the count and keeps the sum as in the uninterrupted run."""
    from geot_amd import checkpoint as ck
    cfg = dict(threed_k=8, fused_tail=True, step_per_update=2, switch_ep=3)
    step = _new_step(cfg, 5)
    step.set_epoch(3)
    torch.manual_seed(11)
    _fix_calls(step, batches, 0, 3)
    ck.save(tmp_path / "switch.pt", step, rng_device=DEV)
    step.set_epoch(4)
    assert step.self_labelling
    want = _fix_calls(step, batches, 3, 2)
    final = snap(step.state_dict())
    fresh = _new_step(cfg, 77)
    ck.load(tmp_path / "switch.pt", fresh)
    assert fresh.epoch == 3 and not fresh.self_labelling and int(fresh.tail.window) == 1 and fresh.tail._calls == 1
    fresh.set_epoch(4)
    assert int(fresh.tail.window) == 0
    same(_fix_calls(fresh, batches, 3, 2), want, "losses")
    same(fresh.state_dict(), final, "the state two calls behind the switch")


# ---- 6: the supervised step --------------------------------------------------------------------------------------------------------
def _sup_step(seed, tensor_lr=False):
    from geot_amd.openpoints.models.backbone.transformer import PointTransformer_seg_T
    from geot_amd import train_step as ts
    torch.manual_seed(seed)
    step = ts.SupervisedStep(PointTransformer_seg_T(**SMALL).to(DEV), grad_norm_clip=1.0, fused_tail=True, step_per_update=2)
    if tensor_lr:
        _tensor_lr(step)
    return step


def _sup_calls(call, batches, first, count):
    out = []
    for i in range(first, first + count):
        cur, nxt = batches[i % 3], batches[(i + 1) % 3]
        out.append(call(cur[0], cur[1], cur[2], next_pos=nxt[0]).clone())
    return out


def test_supervised_eager_resume_into_fresh_objects(sup_batches, tmp_path):
    from geot_amd import checkpoint as ck
    step = _sup_step(5)
    torch.manual_seed(11)
    _sup_calls(step, sup_batches, 0, 3)
    ck.save(tmp_path / "sup.pt", step, rng_device=DEV)
    saved = snap(step.state_dict())
    assert int(saved["tail"]["window"]) == 1 and bool(saved["tail"]["accumulator"].any())
    want = _sup_calls(step, sup_batches, 3, 3)
    final = snap(step.state_dict())
    fresh = _sup_step(77)
    torch.manual_seed(123)
    ck.load(tmp_path / "sup.pt", fresh)
    same(fresh.state_dict(), saved, "right after the load")
    same(_sup_calls(fresh, sup_batches, 3, 3), want, "losses")
    same(fresh.state_dict(), final, "the state 3 calls later")
    with pytest.raises(ValueError, match="kind"):
        fresh.load_state_dict(dict(saved, kind="FixMatchNTMStep"))
    with pytest.raises(ValueError, match="step_per_update"):
        fresh.load_state_dict(dict(saved, layout=dict(saved["layout"], step_per_update=3)))
    same(fresh.state_dict(), final, "after two refused loads")
    # the reference's file layout carries the same state: save_checkpoint(step=) / resume_checkpoint(step=)
    from types import SimpleNamespace
    from geot_amd.openpoints.utils import ckpt_util as cu
    cfg = SimpleNamespace(run_name="sup", ckpt_dir=str(tmp_path), save_freq=0)
    path = cu.save_checkpoint(cfg, step.model, 6, optimizer=step.optimizer, step=step)
    assert list(torch.load(path, weights_only=True)) == ["model", "optimizer", "scheduler", "epoch", "geot_amd_step"]
    _sup_calls(fresh, sup_batches, 6, 1)          # (away from the saved state)
    assert cu.resume_checkpoint(cfg, None, pretrained_path=path, step=fresh, printer=lambda s: None) == (7, None)
    same(fresh.state_dict(), final, "after resume_checkpoint(step=)")
    plain = SimpleNamespace(module=_sup_step(3).model)          # ... and the same file as pretrained weights
    assert cu.load_checkpoint(plain, path) == (6, {})
    same(dict(plain.module.state_dict()), final["model"], "load_checkpoint")


def test_supervised_replayed_resume_into_the_same_wrapper(sup_batches):
    from geot_amd import checkpoint as ck, graph_step as gs
    step = _sup_step(5, tensor_lr=True)
    call = gs.GraphedSupervisedStep(step, warmup=2)
    torch.manual_seed(11)
    _sup_calls(call, sup_batches, 0, 5)
    assert call.captured
    state, rng = call.state_dict(), ck.rng_state(DEV)
    assert int(state["tail"]["window"]) == 1
    want = _sup_calls(call, sup_batches, 5, 3)
    final = snap(call.state_dict())
    graphs = {k: v[0] for k, v in call.graphs.items()}
    call.load_state_dict(state)
    ck.set_rng_state(rng)
    same(_sup_calls(call, sup_batches, 5, 3), want, "losses")
    same(call.state_dict(), final, "the state 3 replays later", ignore=HOST_VIEW)
    assert set(call.graphs) == set(graphs) and all(call.graphs[k][0] is g for k, g in graphs.items())
