"""The training driver on the GPU (geot_amd/fit.py, geot_amd/schedule.py): fit() against the loop written out by hand, across a
decay epoch and the switch_ep phase change, with and without validation, stopped and resumed, eager and replayed, and the
supervised stage.  Every comparison is bitwise.

The set-up: the small segmentor and the wide cfg of tests/test_checkpoint_gpu.py (fused tail, clipping, step_per_update 2, a
moving teacher, DropPath live); 6 labelled, 6 unlabelled and 2 validation scans of 3 500 to 9 000 vertices sampled at 4096
points -- with replacement for the scan below 4096 --, batches of 2 + 2: three iterations per epoch; epochs = 3,
decay_epochs = [2], switch_ep = 2, so the second epoch trains at the decayed rate and the third in the self-labelling phase."""
import bisect
import copy
import os
import random
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

SMALL = dict(trans_dim=384, depth=3, num_heads=4, group_size=32, num_group=128, encoder_dims=256, nclasses=17,
             drop_path_rate=0.1, downsample_targets=[2048, 1024, 512], extract_layers=[1, 2, 3])
STEP_CFG = dict(threed_k=8, fused_tail=True, grad_norm_clip=1.0, step_per_update=2, ema_teacher=True, switch_ep=2)
N = 4096
SIZES_L, SIZES_U, SIZES_V = [5003, 9000, 3500, 6111, 8192, 7000], [6001, 5500, 8999, 7321, 5000, 6789], [5200, 8100]
CFG = dict(lr=1e-3, sched="multistep", decay_epochs=[2], decay_rate=0.1, warmup_epochs=0, sched_on_epoch=True, epochs=3,
           val_freq=1, test_freq=2, batch_size_l=2, batch_size_u=2, batch_size=2, batch_size_val=2, num_points=N, num_classes=17,
           num_votes=0, run_name="small", supervised_epochs=0)
SAMPLER_SEED = 7
TIMING = ("seconds", "clouds_per_s")
VAL_KEYS = ("val_miou", "val_dsc", "val_acc", "best_val_miou", "best_val_dsc", "best_val_acc", "best_epoch", "saved")
HOST_VIEW = (".tail._calls", ".tail._pending")      # the tail's host-side view of its window: advanced by python calls, not by replays
_made = {}


# ---- the comparison helpers of tests/test_checkpoint_gpu.py, restated -----------------------------------------------------------
def flat(obj, prefix=""):
    if isinstance(obj, dict):
        return {k2: v2 for k, v in obj.items() for k2, v2 in flat(v, "%s.%s" % (prefix, k)).items()}
    if isinstance(obj, (list, tuple)):
        return {k2: v2 for i, v in enumerate(obj) for k2, v2 in flat(v, "%s[%d]" % (prefix, i)).items()}
    return {prefix: obj}


def snap(obj):
    if isinstance(obj, dict):
        return {k: snap(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [snap(v) for v in obj]
    return obj.detach().clone() if torch.is_tensor(obj) else obj


def _bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


def same(a, b, what, ignore=()):
    """Two trees hold the same leaves: tensors bit for bit (shape and dtype too), everything else equal (nan = nan)."""
    ignore = tuple(ignore)          # (a prefix or a suffix of the leaf's path)
    a, b = ({k: v for k, v in flat(t).items() if not (k.startswith(ignore) or k.endswith(ignore))} if ignore else flat(t) for t in (a, b))
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


def differ(a, b):
    a, b = flat(a), flat(b)
    return [k for k, x in a.items() if torch.is_tensor(x) and not torch.equal(_bits(x), _bits(b[k]))]


# ---- the set-up -----------------------------------------------------------------------------------------------------------------
def _scan_set(sizes, first):
    from geot_amd.openpoints.dataset import DeviceScanSet
    from geot_amd.synth import make_cloud, region_labels
    units = [make_cloud(m, first + i)[0] for i, m in enumerate(sizes)]
    scale, center = np.float32(31.5), np.array([14.0, -37.0, 61.0], np.float32)
    return DeviceScanSet([(u * scale + center).astype(np.float32) for u in units], [(region_labels(u) % 17).astype(np.int32) for u in units],
                         cls=[i % 2 for i in range(len(sizes))], device=DEV)


def _sets():
    if "sets" not in _made:
        _made["sets"] = (_scan_set(SIZES_L, 800), _scan_set(SIZES_U, 830), _scan_set(SIZES_V, 860))
    return _made["sets"]


def _new(seed=5, draws=None):
    from geot_amd import train_step as ts
    from geot_amd.openpoints.dataset import FixMatchBatcher
    torch.manual_seed(seed)
    step = ts.build_fixmatch(DEV, seg_cfg=SMALL, cfg=dict(ts.NTM_CFG, **STEP_CFG), use_ddp=False, meters=True)
    lab, unl, _ = _sets()
    return step, FixMatchBatcher(lab, unl, N, stream=torch.cuda.Stream(DEV), draws=draws)


def _seed(seed=11):
    """Every generator a run reads: numpy's and python's (the batchers' host draws), torch's CPU and device ones (DropPath)."""
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)


def _lrs(step):
    return [group["lr"] for opt in step.optimizers() for group in opt.param_groups]


def _lr_at(epoch, decay=(2,)):
    """The rate `epoch` trains at, by hand: MultiStepLRScheduler's value of the epoch before."""
    return 1e-3 * 0.1 ** bisect.bisect_right(list(decay), epoch)


def _clean(rec, drop=TIMING):
    return {k: v for k, v in rec.items() if k not in drop}


def _fit(cfg=CFG, val=False, draws=None, graphed=False, ckpt_dir=None, resume=None, seed=5, run_seed=11, spy=None):
    from geot_amd import graph_step as gs
    from geot_amd.fit import fit
    step, batcher = _new(seed, draws)
    call = gs.GraphedFixMatchStep(step, warmup=2) if graphed else step
    _seed(run_seed)
    seen = []

    def log(rec):
        seen.append({"rec": rec, "lrs": [float(t) for t in _lrs(step)], "lr_objects": _lrs(step)})
        if spy is not None:
            spy(rec, step, call)
    out = fit(call, batcher, cfg, val=_sets()[2] if val else None, ckpt_dir=ckpt_dir, resume=resume, log=log,
              generator=torch.Generator().manual_seed(SAMPLER_SEED))
    return {"step": step, "call": call, "out": out, "seen": seen, "final": snap(step.state_dict())}


def _prior_by_hand(step, batcher, generator):
    from geot_amd.fit import epoch_batches
    from geot_amd.ntm import cal_mean_feature
    lab, unl = epoch_batches(len(SIZES_L), len(SIZES_U), 2, 2, generator=generator)

    def logits():
        for idx_l, idx_u in zip(lab, unl):
            data, data_u = batcher.batch(idx_l, idx_u)
            batcher.join(data, data_u)
            yield step.model(data)[0], data["y"]
    step.model.eval()
    with torch.no_grad():
        cm = cal_mean_feature(logits(), 17)
    step.model.train()
    return cm


@pytest.fixture(scope="module")
def plain_run():
    """fit(), eager, host draws, no validation, no files."""
    return _fit()


@pytest.fixture(scope="module")
def val_run(tmp_path_factory):
    """The same run with a validation behind every epoch and files at epochs 2 and 3 (and at every new best); the file of
    epoch 2 is kept aside, and so are the model and the generators as the validation of epoch 2 found them."""
    folder = tmp_path_factory.mktemp("fit")
    kept = {}

    def spy(rec, step, call):
        from geot_amd import checkpoint as ck
        if rec["epoch"] == 2:
            assert rec["saved"]
            shutil.copyfile(folder / "small_ckpt_latest.pt", folder / "epoch2.pt")
            kept["model"] = copy.deepcopy(step.model.state_dict())
            kept["rng"] = ck.rng_state(DEV)          # put back behind the validation: what it started from
    run = _fit(val=True, ckpt_dir=folder, spy=spy)
    run.update(folder=folder, kept=kept)
    return run


# ---- 1. fit == the loop by hand -------------------------------------------------------------------------------------------------
def test_fit_equals_the_loop_written_out_by_hand(plain_run):
    from geot_amd.fit import LOG_NAMES, epoch_batches
    step, batcher = _new()
    _seed()
    g = torch.Generator().manual_seed(SAMPLER_SEED)
    lrs = []
    for opt in step.optimizers():
        for group in opt.param_groups:
            group["lr"] = torch.tensor(1e-3, dtype=torch.float32, device=DEV)
            group["initial_lr"] = 1e-3          # (what a scheduler records in the group: checkpoint.py carries the key)
            lrs.append(group["lr"])
    step.cm.copy_(_prior_by_hand(step, batcher, g))
    for epoch in (1, 2, 3):
        lab, unl = epoch_batches(len(SIZES_L), len(SIZES_U), 2, 2, generator=g)
        assert len(lab) == len(unl) == 3
        step.set_epoch(epoch)
        step.meters.reset()
        cur = batcher.batch(lab[0], unl[0])
        batcher.join(*cur)
        for it in range(3):
            nxt = None
            if it + 1 < 3:
                nxt = batcher.batch(lab[it + 1], unl[it + 1])
                batcher.join(*nxt)
            step(cur[0], cur[1], next_batches=nxt) if nxt is not None else step(cur[0], cur[1])
            cur = nxt
        stats = step.meters.read()[0]
        for t in lrs:
            t.fill_(_lr_at(epoch + 1))
        got = plain_run["seen"][epoch - 1]
        assert stats["iterations"] == 3
        same({name: stats[key] for key, name in LOG_NAMES.items()}, {name: got["rec"][name] for name in LOG_NAMES.values()},
             "the meters of epoch %d" % epoch)
        assert [got["rec"]["train_over_th_acc_class_%d" % j] for j in range(17)] == stats["mean_pseudo_label_acc_classwise"]
        assert got["lrs"] == [float(t) for t in lrs] and got["rec"]["lr"] == _lr_at(epoch)
    same(step.state_dict(), plain_run["final"], "the final state")
    assert step.self_labelling and plain_run["step"].self_labelling and plain_run["out"]["epoch"] == 3


# ---- 2. the decay takes effect --------------------------------------------------------------------------------------------------
def test_the_decay_takes_effect(plain_run):
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lr_schedule_ref.npz"))
    flat_run = _fit(cfg=dict(CFG, decay_epochs=[99]))
    f32 = lambda v: float(np.float32(v))          # noqa: E731
    assert [s["rec"]["lr"] for s in plain_run["seen"]] == [1e-3, 1e-3 * 0.1 ** 1, 1e-3 * 0.1 ** 1]
    assert [s["lrs"] for s in plain_run["seen"]] == [[f32(1e-3 * 0.1 ** 1)] * len(plain_run["seen"][0]["lrs"])] * 3
    assert all(s["lrs"] == [f32(1e-3)] * len(s["lrs"]) and s["rec"]["lr"] == 1e-3 for s in flat_run["seen"])
    # (the golden schedule's shape: the value behind the epoch before a decay epoch is the decayed one)
    assert want["multistep_220"][218] == 1e-3 and want["multistep_220"][219] == 1e-3 * 0.1 ** 1
    # the tensors were filled, never rebound
    objects = [s["lr_objects"] for s in plain_run["seen"]]
    assert all(a is b for later in objects[1:] for a, b in zip(objects[0], later))
    # epoch 1 trains at 1e-3 in both runs; from epoch 2 on the parameters part
    assert _clean(flat_run["seen"][0]["rec"]) == _clean(plain_run["seen"][0]["rec"])
    assert _clean(flat_run["seen"][1]["rec"]) != _clean(plain_run["seen"][1]["rec"])
    moved = differ(flat_run["final"]["model"], plain_run["final"]["model"])
    assert len(moved) > len(plain_run["final"]["model"]) // 2, len(moved)


# ---- 3. stop behind epoch 2, resume into fresh objects --------------------------------------------------------------------------
def test_resume_into_fresh_objects_equals_the_uninterrupted_run(val_run, tmp_path):
    first = _fit(cfg=dict(CFG, epochs=2), val=True, ckpt_dir=tmp_path)          # the run that stops behind epoch 2
    assert [s["rec"]["epoch"] for s in first["seen"]] == [1, 2] and first["seen"][1]["rec"]["saved"]
    for a, b in zip(first["seen"], val_run["seen"]):
        same(_clean(a["rec"]), _clean(b["rec"]), "the record of epoch %d" % a["rec"]["epoch"])
    # ... leaves the file the uninterrupted run wrote behind its epoch 2
    files = [torch.load(path, map_location="cpu", weights_only=True) for path in (tmp_path / "small_ckpt_latest.pt", val_run["folder"] / "epoch2.pt")]
    same(files[0], files[1], "the file behind epoch 2")
    assert files[0]["extra"]["epoch"] == 2 and set(files[0]["extra"]) == {"epoch", "best", "best_epoch", "best_all", "sampler"}
    resumed = _fit(val=True, ckpt_dir=tmp_path, resume=tmp_path / "small_ckpt_latest.pt", seed=77, run_seed=123)      # other weights, other streams
    assert [s["rec"]["epoch"] for s in resumed["seen"]] == [3]
    same(resumed["final"], val_run["final"], "the final state")
    same(_clean(resumed["seen"][0]["rec"]), _clean(val_run["seen"][2]["rec"]), "the record of epoch 3")
    assert resumed["seen"][0]["lrs"] == val_run["seen"][2]["lrs"]
    assert resumed["out"]["best"] == val_run["out"]["best"] is not None and resumed["out"]["best_epoch"] == val_run["out"]["best_epoch"]
    a, b = resumed["out"]["generator"], val_run["out"]["generator"]
    assert torch.equal(a.get_state(), b.get_state())
    perm = lambda g: torch.randperm(6, generator=torch.Generator().set_state(g.get_state()))      # noqa: E731
    assert torch.equal(perm(a), perm(b))          # the sampler's next permutation


# ---- 4. replayed == eager -------------------------------------------------------------------------------------------------------
def test_fit_replayed_equals_fit_eager(tmp_path):
    from geot_amd.openpoints.dataset import DeviceDraws
    eager = _fit(draws=DeviceDraws(3, views=True))
    graphs = {}

    def spy(rec, step, call):
        graphs[rec["epoch"]] = ({k: v[0] for k, v in call.graphs.items()}, dict(call._eager_runs))
        if rec["epoch"] == 2:
            shutil.copyfile(tmp_path / "small_ckpt_latest.pt", tmp_path / "epoch2.pt")
    replayed = _fit(draws=DeviceDraws(3, views=True), graphed=True, ckpt_dir=tmp_path, spy=spy)
    for a, b in zip(eager["seen"], replayed["seen"]):
        same(_clean(a["rec"], TIMING + ("saved",)), _clean(b["rec"], TIMING + ("saved",)), "the record of epoch %d" % a["rec"]["epoch"])
        assert a["lrs"] == b["lrs"]
    # (the wrapper marks the optimizers' groups capturable: how the target executes, which a load never restores either)
    same(replayed["final"], eager["final"], "the final state", ignore=HOST_VIEW + (".capturable",))
    # every phase's graphs are captured on its first use; the decay behind epoch 1 captured nothing anew and raised nothing
    assert set(graphs[1][0]) == {"P@e", "M@e"} and set(graphs[2][0]) == {"P@e", "M@e"}
    assert set(graphs[3][0]) == {"P@e", "M@e", "P@2", "M@2"}
    assert all(graphs[e][0][k] is graphs[1][0][k] for e in (2, 3) for k in ("P@e", "M@e"))
    assert graphs[2][1] == graphs[1][1] and all(graphs[3][1][k] == graphs[1][1][k] for k in ("P@e", "M@e"))
    assert all(set(kinds) == {"kernel"} for kinds in replayed["call"].node_types.values())
    assert float(replayed["step"].tail.steps.max()) > 0
    # the replayed run, stopped behind epoch 2 and resumed into a fresh wrapper (its warm-up calls are real calls), draw
    # counters included
    resumed = _fit(draws=DeviceDraws(99, views=True), graphed=True, resume=tmp_path / "epoch2.pt", seed=77, run_seed=123)
    assert [s["rec"]["epoch"] for s in resumed["seen"]] == [3]
    same(_clean(resumed["seen"][0]["rec"], TIMING + ("saved",)), _clean(replayed["seen"][2]["rec"], TIMING + ("saved",)), "the record of epoch 3")
    same(resumed["final"], replayed["final"], "the final state of the resumed replay", ignore=HOST_VIEW)


# ---- 5. a run with validation == a run without ----------------------------------------------------------------------------------
def test_validation_leaves_the_training_run_alone(plain_run, val_run):
    from geot_amd import checkpoint as ck
    from geot_amd.openpoints.models.segmentation import WholePartSeg
    from geot_amd.validation import validate_scans
    same(val_run["final"], plain_run["final"], "the final state")
    for a, b in zip(val_run["seen"], plain_run["seen"]):
        same(_clean(a["rec"], TIMING + VAL_KEYS), _clean(b["rec"], TIMING + VAL_KEYS), "the record of epoch %d" % a["rec"]["epoch"])
        assert {"val_miou", "val_dsc", "val_acc", "best_val_miou"} <= set(a["rec"]) and "val_miou" not in b["rec"]
    # the metrics of epoch 2 are those of validate_scans on the model as it stood, from the generators as they stood
    model = WholePartSeg(segmentor_args=dict(NAME="PointTransformer_seg_T", **SMALL)).to(DEV)
    model.load_state_dict(val_run["kept"]["model"])
    ck.set_rng_state(val_run["kept"]["rng"])
    macc, miou, mdsc = validate_scans(model, _sets()[2], dict(num_points=N, num_classes=17, epoch=2, epochs=3), batch_size=2)
    rec = val_run["seen"][1]["rec"]
    assert (rec["val_acc"], rec["val_miou"], rec["val_dsc"]) == (float(macc), float(miou), float(mdsc))
    best = max(s["rec"]["val_miou"] for s in val_run["seen"])
    assert val_run["out"]["best"] == best and val_run["seen"][2]["rec"]["best_val_miou"] == best
    assert [s["rec"]["saved"] for s in val_run["seen"]][1:] == [True, True]


# ---- 6. the prior ---------------------------------------------------------------------------------------------------------------
def test_the_prior_is_computed_into_the_steps_own_tensor():
    from geot_amd.fit import fit
    step, batcher = _new()
    held, before = step.cm, step.cm.clone()
    _seed()
    out = fit(step, batcher, dict(CFG, epochs=0), generator=torch.Generator().manual_seed(SAMPLER_SEED))
    assert out["records"] == [] and step.cm is held and not torch.equal(step.cm, before)
    assert step.model.training
    other, other_batcher = _new()
    _seed()
    want = _prior_by_hand(other, other_batcher, torch.Generator().manual_seed(SAMPLER_SEED))
    assert torch.equal(_bits(step.cm), _bits(want))
    fit(step, batcher, dict(CFG, epochs=0), prior=False)
    assert torch.equal(_bits(step.cm), _bits(want))          # prior=False keeps what the step holds


# ---- 7. the supervised stage ----------------------------------------------------------------------------------------------------
def _sup():
    from geot_amd import train_step as ts
    from geot_amd.openpoints.dataset import SupervisedBatcher
    from geot_amd.openpoints.models.segmentation import WholePartSeg
    torch.manual_seed(5)
    model = WholePartSeg(segmentor_args=dict(NAME="PointTransformer_seg_T", **SMALL)).to(DEV)
    step = ts.SupervisedStep(model, grad_norm_clip=1.0, fused_tail=True, step_per_update=2)
    return step, SupervisedBatcher(_sets()[0], N, stream=torch.cuda.Stream(DEV))


def test_the_supervised_stage(tmp_path):
    from geot_amd.fit import epoch_batches, fit
    from geot_amd.openpoints.models.segmentation import WholePartSeg
    from geot_amd.openpoints.utils import ckpt_util as cu
    cfg = dict(CFG, epochs=2, run_name="stage1")
    step, batcher = _sup()
    _seed()
    weights = {}
    out = fit(step, batcher, cfg, val=_sets()[2], ckpt_dir=tmp_path, generator=torch.Generator().manual_seed(SAMPLER_SEED),
              log=lambda rec: weights.__setitem__(rec["epoch"], copy.deepcopy(step.model.state_dict())))
    assert [r["epoch"] for r in out["records"]] == [1, 2] and all("last_loss" in r and "val_miou" in r for r in out["records"])
    # by hand
    hand, hand_batcher = _sup()
    _seed()
    g = torch.Generator().manual_seed(SAMPLER_SEED)
    lr = hand.optimizer.param_groups
    for group in lr:
        group["lr"], group["initial_lr"] = torch.tensor(1e-3, dtype=torch.float32, device=DEV), 1e-3
    for epoch in (1, 2):
        plan = epoch_batches(len(SIZES_L), None, 2, generator=g)
        hand.new_epoch()
        cur = hand_batcher.batch(plan[0])
        hand_batcher.join(cur)
        for it in range(3):
            nxt = None
            if it + 1 < 3:
                nxt = hand_batcher.batch(plan[it + 1])
                hand_batcher.join(nxt)
            loss = hand(cur["pos"], cur["cls"], cur["y"], next_pos=None if nxt is None else nxt["pos"])
            cur = nxt
        assert float(loss) == out["records"][epoch - 1]["last_loss"]
        for group in lr:
            group["lr"].fill_(_lr_at(epoch + 1))
    same(hand.state_dict(), step.state_dict(), "the final state")
    # the best file is what the second stage names as pretrained_path: it loads into a fresh student and teacher
    assert out["best_epoch"] in (1, 2)
    for _ in ("student", "teacher"):
        fresh = WholePartSeg(segmentor_args=dict(NAME="PointTransformer_seg_T", **SMALL)).to(DEV)
        epoch, metrics = cu.load_checkpoint(fresh, str(tmp_path / "stage1_ckpt_best.pth"))
        assert epoch == out["best_epoch"] and metrics["miou"] == out["best"]
        same(dict(fresh.state_dict()), weights[out["best_epoch"]], "the weights of the best epoch")
