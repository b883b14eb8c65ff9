"""The training driver without a GPU (geot_amd/schedule.py, geot_amd/fit.py): the schedule against the values the reference's
MultiStepLRScheduler returned (tests/golden/lr_schedule_ref.npz, made by tests/golden/make_lr_golden.py), the batch plans
against torch's samplers run by hand, and fit()'s control flow over a duck-typed step and batcher on CPU tensors that record
every call."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch.utils.data import BatchSampler, RandomSampler

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lr_schedule_ref.npz")
CASES = {"multistep_210_270": dict(lr=1e-3, sched="multistep", decay_epochs=[210, 270], decay_rate=0.1, warmup_epochs=0,
                                   min_lr=None, sched_on_epoch=True),
         "multistep_220": dict(lr=1e-3, sched="multistep", decay_epochs=[220], decay_rate=0.1, warmup_epochs=0, min_lr=None),
         "warmup_3": dict(lr=1e-3, sched="multistep", decay_epochs=[5, 8], decay_rate=0.1, warmup_epochs=3, warmup_lr=1e-6)}


def _optimizers(lr=1e-3):
    a, b = torch.nn.Linear(3, 2), torch.nn.Linear(2, 2)
    return [torch.optim.AdamW([{"params": [a.weight]}, {"params": [a.bias], "weight_decay": 0.0}], lr=lr),
            torch.optim.AdamW(b.parameters(), lr=lr)]


# ---- the schedule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_schedule_equals_the_reference_values(name):
    from geot_amd.schedule import LrSchedule
    want = np.load(GOLDEN)[name]
    assert want.dtype == np.float64 and want.shape == (301,)
    opts = _optimizers()
    sched = LrSchedule(opts, SimpleNamespace(**CASES[name]))
    groups = [g for o in opts for g in o.param_groups]
    tensors = [g["lr"] for g in groups]
    assert all(torch.is_tensor(t) and t.dtype == torch.float32 and t.numel() == 1 for t in tensors)
    assert all(g["initial_lr"] == 1e-3 for g in groups)
    assert all(t.item() == np.float32(want[0]) for t in tensors)          # construction: the epoch-0 value
    for e in range(301):
        got = sched.values(e)
        assert len(got) == 3 and all(type(v) is float for v in got)
        assert all(v == want[e] for v in got), (e, got, want[e])          # float64 ==
    for e in (0, 1, 2, 3, 4, 5, 7, 8, 209, 210, 219, 220, 269, 270, 300):
        sched.step(e)
        assert all(a is g["lr"] for a, g in zip(tensors, groups))          # filled, never rebound
        assert all(t.item() == np.float32(want[e]) for t in tensors), e
    # a dict cfg reads the same
    assert LrSchedule(_optimizers(), dict(CASES[name])).values(250) == [want[250]] * 3


def test_schedule_keeps_a_tensor_lr_and_its_base():
    from geot_amd.schedule import LrSchedule
    opts = _optimizers()
    held = torch.tensor(1e-3, dtype=torch.float32)
    opts[1].param_groups[0]["lr"] = held
    opts[0].param_groups[0]["lr"] = 5e-4          # a group of its own base
    sched = LrSchedule(opts, CASES["multistep_220"])
    assert opts[1].param_groups[0]["lr"] is held
    # the tensor holds float32(1e-3): the base is the configured double, not the float32's double
    assert sched.base_values == [5e-4, 1e-3, 1e-3] and opts[1].param_groups[0]["initial_lr"] == 1e-3
    sched.step(219)
    assert held.item() == np.float32(1e-3 * 0.1 ** 1) and opts[0].param_groups[0]["lr"].item() == np.float32(5e-4 * 0.1 ** 1)
    # a second schedule on the same groups (a resumed process builds one) starts from initial_lr, not from the decayed tensors
    again = LrSchedule(opts, CASES["multistep_220"])
    assert again.base_values == [5e-4, 1e-3, 1e-3] and held.item() == np.float32(1e-3)


@pytest.mark.parametrize("bad, name", [(dict(sched="cosine"), "cosine"), (dict(sched="step"), "step"), (dict(sched=None), "None"),
                                       (dict(lr_noise=[0.5, 0.9]), "lr_noise"), (dict(sched_on_epoch=False), "sched_on_epoch")])
def test_schedule_refuses_by_name(bad, name):
    from geot_amd.schedule import LrSchedule
    opts = _optimizers()
    with pytest.raises(NotImplementedError, match=name):
        LrSchedule(opts, dict(CASES["multistep_220"], **bad))
    assert all(isinstance(g["lr"], float) and "initial_lr" not in g for o in opts for g in o.param_groups)      # untouched


# ---- the batch plans ------------------------------------------------------------------------------------------------------------
def _by_hand(n, b, g, take=None):
    """take: that many next() calls on the loader's iterator, as train.py:462 consumes the unlabelled one (an iterator that
    is not run to its end leaves the sampler's closing draw unmade); None: the whole list, as `for data in loader` does."""
    batches = iter(BatchSampler(RandomSampler(range(n), generator=g), b, drop_last=True))
    return list(batches) if take is None else [next(batches) for _ in range(take)]


def test_epoch_batches_are_torchs_samplers():
    from geot_amd.fit import epoch_batches
    g, h = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    for _ in range(3):          # three epochs from one generator
        lab, unl = epoch_batches(7, 9, 2, 2, generator=g)
        want_l = _by_hand(7, 2, h)
        want_u = _by_hand(9, 2, h, take=len(want_l))
        assert len(want_l) == 3 == len(want_u) < 9 // 2          # drop_last on both, the unlabelled list longer
        assert lab == want_l and unl == want_u
        assert torch.equal(g.get_state(), h.get_state())
    assert epoch_batches(7, None, 3, generator=g) == _by_hand(7, 3, h)          # the supervised form: one list
    assert epoch_batches(8, None, 4, None, g) == _by_hand(8, 4, h)
    before = g.get_state()
    with pytest.raises(ValueError, match="runs out"):
        epoch_batches(6, 3, 2, 2, generator=g)
    assert torch.equal(g.get_state(), before)          # refused when the plan is made, before a draw


# ---- fit()'s control flow -------------------------------------------------------------------------------------------------------
class FakeMeters:
    def __init__(self, events):
        self.events, self.sum, self.n = events, 0.0, 0

    def reset(self):
        self.events.append(("reset",))
        self.sum, self.n = 0.0, 0

    def read(self):
        self.events.append(("read",))
        avg = self.sum / max(self.n, 1)
        out = {"train_loss": avg, "train_loss_l": avg, "train_loss_u": 0.0, "th_percentage": 1.0, "mean_pseudo_label_acc": 0.5,
               "teacher_acc": 0.25, "student_acc": 0.75, "over_th_wobg": 0.0, "over_acc_wobg": 0.0, "manifold_loss_feat": 0.0,
               "insT_identity_loss": 0.0, "insT_threed_loss": 0.0, "mean_pseudo_label_acc_classwise": [0.0, 1.0],
               "mean_th_meter_u_classwise": [2.0, 3.0], "mean_th_meter_u_classwise_recall": [4.0, 5.0]}
        return out, tuple(out.values())


class FakeStep:
    """What fit() touches of a FixMatchNTMStep, on the CPU: one weight, trained by hand at the group's tensor lr."""

    def __init__(self, events):
        self.events = events
        self.model = torch.nn.Linear(2, 1, bias=False)
        with torch.no_grad():
            self.model.weight.fill_(1.0)
        self.optimizer = torch.optim.SGD(self.model.parameters(), lr=1e-3)
        self.cfg = {"batch_size_l": 2, "batch_size_u": 2, "num_classes": 2}
        self.cm = torch.zeros(2, 2)
        self.meters = FakeMeters(events)
        self.epoch = self.announced = None

    def optimizers(self):
        return [self.optimizer]

    def set_epoch(self, epoch):
        self.events.append(("set_epoch", epoch))
        self.epoch = epoch

    def __call__(self, data, data_u, next_batches=None):
        lr = self.optimizer.param_groups[0]["lr"]
        assert torch.is_tensor(lr), "the schedule is installed before the first call"
        self.events.append(("call", self.epoch, data["ids"], data_u["ids"], next_batches is not None, lr.item()))
        if self.announced is not None:
            assert self.announced[0] is data and self.announced[1] is data_u          # the very dicts the last call announced
        self.announced = next_batches
        with torch.no_grad():
            self.model.weight.mul_(1.0 - lr.item()).add_(data["noise"])
        self.meters.sum += float(self.model.weight.detach().sum())
        self.meters.n += 1
        return {"loss": self.model.weight.sum().detach()}

    def state_dict(self):
        return {"w": self.model.weight.detach().clone(), "epoch": self.epoch}

    def load_state_dict(self, state):
        with torch.no_grad():
            self.model.weight.copy_(state["w"])
        self.epoch = state["epoch"]


class FakeBatcher:
    """6 labelled and 8 unlabelled scans; a batch draws from numpy's global stream, as the host draws of the real one."""
    n_l, n_u, draws = 6, 8, None

    def __init__(self, events):
        self.events = events

    def batch(self, idx_l, idx_u):
        noise = float(np.random.rand())
        self.events.append(("batch", tuple(idx_l), tuple(idx_u), noise))
        return {"ids": tuple(idx_l), "noise": noise}, {"ids": tuple(idx_u)}

    def join(self, data, data_u):
        self.events.append(("join", data["ids"]))


CFG = dict(CASES["warmup_3"], epochs=7, val_freq=3, test_freq=4, run_name="fake", seed=11, batch_size_val=2, num_points=16,
           num_classes=2, supervised_epochs=0)
MIOU = {3: 0.5, 6: 0.4, 7: 0.6}          # scripted validation results by epoch


def _run(monkeypatch, tmp_path, cfg=CFG, val=True, resume=None, ckpt=True, events=None, test=None):
    from geot_amd import fit as F, validation
    events = [] if events is None else events

    def validate_scans(model, scans, vcfg, **kw):
        events.append(("validate", vcfg["epoch"], scans, sorted(kw)))
        np.random.rand(3), torch.rand(3)          # a validation reads the host generators
        import random
        random.random()
        miou = MIOU.get(vcfg["epoch"], 0.1)
        return np.float64(miou + 0.1), np.float64(miou), np.float64(miou + 0.2)
    monkeypatch.setattr(validation, "validate_scans", validate_scans)
    saves = []
    real_save = F.checkpoint.save
    monkeypatch.setattr(F.checkpoint, "save", lambda path, step, **kw: (saves.append((kw["epoch"], os.path.basename(path))),
                                                                        events.append(("save", kw["epoch"])),
                                                                        real_save(path, step, **kw))[-1])
    np.random.seed(3)
    torch.manual_seed(3)
    step, records = FakeStep(events), []
    out = F.fit(step, FakeBatcher(events), cfg, val="VAL" if val else None, test=test, ckpt_dir=str(tmp_path) if ckpt else None,
                resume=resume, log=lambda rec: (records.append(rec), events.append(("log", rec["epoch"]))), prior=False)
    return SimpleNamespace(step=step, events=events, records=records, out=out, saves=saves)


def test_fit_control_flow(monkeypatch, tmp_path):
    want = np.load(GOLDEN)["warmup_3"]
    run = _run(monkeypatch, tmp_path)
    ev = run.events
    calls = [e for e in ev if e[0] == "call"]
    assert [e[1] for e in ev if e[0] == "set_epoch"] == list(range(1, 8))          # epochs start_epoch .. epochs inclusive
    assert len(calls) == 7 * 3 and [c[1] for c in calls] == [e for e in range(1, 8) for _ in range(3)]
    for epoch in range(1, 8):
        at = [i for i, e in enumerate(ev) if e[:2] in (("set_epoch", epoch), ("log", epoch)) or (e[0] == "call" and e[1] == epoch)]
        assert ev[at[0]][0] == "set_epoch" and ev[at[-1]][0] == "log"          # set_epoch before the epoch's first call
        assert ev[at[0] + 1] == ("reset",)                                           # ... and the meters' reset with it
        mine = [ev[i] for i in at[1:-1]]
        # the schedule is stepped AFTER the epoch: epoch e trains at values(e - 1), the tensor read inside the call
        assert all(c[5] == np.float32(want[epoch - 1]) for c in mine), (epoch, mine)
        # the pipeline: every call but the epoch's last announces the next batch; the last one -- before a save or not --
        # carries no look-ahead
        assert [c[4] for c in mine] == [True, True, False]
        assert sum(1 for e in ev[at[0]:at[-1]] if e == ("read",)) == 1          # one read per epoch
    # every batch is built once, joined, in plan order, and the plan is torch's samplers' from the seeded generator
    g = torch.Generator().manual_seed(CFG["seed"])
    plan = []
    for _ in range(7):
        lab, unl = _by_hand(6, 2, g), _by_hand(8, 2, g, take=3)
        plan += list(zip(map(tuple, lab), map(tuple, unl)))
    assert [(e[1], e[2]) for e in ev if e[0] == "batch"] == plan == [(c[2], c[3]) for c in calls]
    assert torch.equal(run.out["generator"].get_state(), g.get_state())
    # validation exactly at val_freq multiples and the last epoch; saves at test_freq, the last epoch and new bests
    assert [e[1] for e in ev if e[0] == "validate"] == [3, 6, 7]
    assert all(e[2] == "VAL" and {"graph", "lookahead", "refine", "parts", "batch_size"} <= set(e[3]) for e in ev if e[0] == "validate")
    assert [s[0] for s in run.saves] == [3, 4, 7] and {s[1] for s in run.saves} == {"fake_ckpt_latest.pt"}
    assert sorted(os.listdir(tmp_path)) == ["fake_ckpt_best.pth", "fake_ckpt_latest.pt", "fake_ckpt_latest.pth"]
    best = torch.load(tmp_path / "fake_ckpt_best.pth", weights_only=True)
    assert best["epoch"] == 7 and best["miou"] == 0.6 and best["best_val"] == 0.6 and isinstance(best["optimizer"]["param_groups"][0]["lr"], float)
    assert torch.equal(best["model"]["weight"], run.step.model.weight)
    assert run.out["best"] == 0.6 and run.out["best_epoch"] == 7 and run.out["epoch"] == 7
    # one record per epoch, with the reference's names
    assert [r["epoch"] for r in run.records] == list(range(1, 8)) and run.records == run.out["records"]
    names = {"epoch", "lr", "train_loss", "train_loss_l", "train_loss_u", "th_percentage", "train_over_th_acc", "teacher_acc",
             "student_acc", "over_th_wobg", "over_acc_wobg", "manifold_loss_feat", "insT_identity_loss", "insT_threed_loss",
             "train_over_th_acc_class_0", "train_over_th_acc_class_1", "train_over_th_num_class_0", "train_over_th_num_class_1",
             "train_over_th_recall_class_0", "train_over_th_recall_class_1", "seconds", "clouds_per_s", "saved"}
    for r in run.records:
        assert names <= set(r), sorted(names - set(r))
        assert r["lr"] == want[r["epoch"] - 1] and r["seconds"] > 0 and r["clouds_per_s"] == 12 / r["seconds"]
    assert ["val_miou" in r for r in run.records] == [False, False, True, False, False, True, True]
    assert ["best_val_miou" in r for r in run.records] == [False, False] + [True] * 5
    assert [r.get("best_val_miou") for r in run.records[2:]] == [0.5, 0.5, 0.5, 0.5, 0.6]
    assert run.records[5]["val_miou"] == 0.4 and run.records[5]["val_acc"] == 0.5 and run.records[5]["val_dsc"] == pytest.approx(0.6)
    assert [r["saved"] for r in run.records] == [False, False, True, True, False, False, True]
    # a run with validation draws the batches of a run without, and trains to the same weights
    plain = _run(monkeypatch, tmp_path / "plain", val=False, ckpt=False)
    assert [e for e in plain.events if e[0] == "batch"] == [e for e in ev if e[0] == "batch"]
    assert torch.equal(plain.step.model.weight, run.step.model.weight)
    assert not any("val_miou" in r or "best_val_miou" in r for r in plain.records) and plain.out["best"] is None


def test_fit_resume_skips_finished_epochs_and_restores_best(monkeypatch, tmp_path):
    whole = _run(monkeypatch, tmp_path / "whole")
    first = _run(monkeypatch, tmp_path / "cut", cfg=dict(CFG, epochs=4))          # stops behind epoch 4, which saves
    assert [s[0] for s in first.saves] == [3, 4] and first.out["best"] == 0.5
    state = torch.load(tmp_path / "cut" / "fake_ckpt_latest.pt", weights_only=True)
    assert state["extra"]["epoch"] == 4 and state["extra"]["best"] == 0.5 and state["extra"]["best_epoch"] == 3
    rest = _run(monkeypatch, tmp_path / "rest", resume=tmp_path / "cut" / "fake_ckpt_latest.pt")
    assert [e[1] for e in rest.events if e[0] == "set_epoch"] == [5, 6, 7]
    assert [r["epoch"] for r in rest.records] == [5, 6, 7]
    assert rest.records[0]["best_val_miou"] == 0.5 and rest.records[0]["best_epoch"] == 3          # best came back
    assert [s[0] for s in rest.saves] == [7]          # 6 is no new best (0.4 < 0.5), 7 is (0.6) and the last
    # the plans continue the saved sampler state, the schedule is restored by step(epoch) alone
    batches = lambda run, first: [e[1:3] for e in run.events if e[0] == "batch"][first:]      # noqa: E731
    assert batches(rest, 0) == batches(whole, 12)
    want = np.load(GOLDEN)["warmup_3"]
    assert [c[5] for c in rest.events if c[0] == "call"][:3] == [np.float32(want[4])] * 3
    assert torch.equal(rest.out["generator"].get_state(), whole.out["generator"].get_state())
    assert rest.out["best"] == whole.out["best"] == 0.6 and rest.out["best_epoch"] == 7


def test_fit_scores_the_test_set_at_every_save_epoch(monkeypatch, tmp_path):
    run = _run(monkeypatch, tmp_path, test="TEST")
    assert [(e[1], e[2]) for e in run.events if e[0] == "validate"] == [(3, "VAL"), (4, "TEST"), (6, "VAL"), (7, "VAL"), (7, "TEST")]
    assert ["test_miou" in r for r in run.records] == [False, False, False, True, False, False, True]
    assert run.records[6]["test_miou"] == run.records[6]["val_miou"] == 0.6
    plain = _run(monkeypatch, tmp_path / "plain", val=False, ckpt=False)
    assert torch.equal(plain.step.model.weight, run.step.model.weight)


def test_fit_refuses_by_name(monkeypatch, tmp_path):
    from geot_amd import fit as F
    events = []
    with pytest.raises(NotImplementedError, match="supervised_epochs"):
        F.fit(FakeStep(events), FakeBatcher(events), dict(CFG, supervised_epochs=5), prior=False)
    with pytest.raises(NotImplementedError, match="cosine"):
        F.fit(FakeStep(events), FakeBatcher(events), dict(CFG, sched="cosine"), prior=False)
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    with pytest.raises(NotImplementedError, match="2 ranks"):
        F.fit(FakeStep(events), FakeBatcher(events), CFG, prior=False)
    assert not events


def test_names_are_exported():
    from geot_amd import LrSchedule, epoch_batches, fit, train_one_epoch
    from geot_amd import fit as module, schedule
    assert LrSchedule is schedule.LrSchedule and epoch_batches is module.epoch_batches and train_one_epoch is module.train_one_epoch
    assert callable(fit) and callable(module.fit)          # geot_amd.fit(...) is geot_amd.fit.fit(...)
