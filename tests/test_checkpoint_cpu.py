"""Checkpoints without a GPU: the reference's file format (geot_amd/openpoints/utils/ckpt_util.py against the fixture
tests/golden/make_ckpt_golden.py made by executing the reference's own functions), the host generators, the atomic save
and the in-place optimizer restore of geot_amd/checkpoint.py."""
import json
import os
import random
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def tiny(fill=None):
    """The tiny module of the fixture (tests/golden/make_ckpt_golden.py builds the same)."""
    m = nn.Sequential(OrderedDict(encoder=nn.Linear(4, 3), norm=nn.BatchNorm1d(3), head=nn.Linear(3, 2)))
    if fill is not None:
        with torch.no_grad():
            for t in m.state_dict().values():
                t.fill_(fill)
    return m


def trained(seed, steps=3):
    torch.manual_seed(seed)
    m = tiny()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2, 5], gamma=0.1)
    for _ in range(steps):
        m(torch.randn(5, 4)).square().sum().backward()
        opt.step()
        opt.zero_grad()
        sched.step()
    return m, opt, sched


def same_tensors(a, b):
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "ckpt_ref.json")) as fh:
        meta = json.load(fh)
    with np.load(os.path.join(GOLDEN, "ckpt_ref.npz")) as z:
        arrays = {k: torch.from_numpy(z[k].copy()) for k in z.files}
    return meta, arrays


def part(arrays, prefix):
    return OrderedDict((k[len(prefix):], v) for k, v in arrays.items() if k.startswith(prefix))


def test_save_load_resume_round_trip(tmp_path):
    from geot_amd.openpoints.utils import ckpt_util as cu
    m, opt, sched = trained(0)
    cfg = SimpleNamespace(run_name="run", ckpt_dir=str(tmp_path), save_freq=0)
    path = cu.save_checkpoint(cfg, m, 4, optimizer=opt, scheduler=sched, additioanl_dict={"best_val": 0.75})
    assert path == str(tmp_path / "run_ckpt_latest.pth") and sorted(os.listdir(tmp_path)) == ["run_ckpt_latest.pth"]
    # pretrained weights alone
    target = tiny(fill=0.5)
    epoch, metrics = cu.load_checkpoint(target, path)
    assert epoch == 4 and metrics == {"best_val": 0.75}
    same_tensors(dict(target.state_dict()), dict(m.state_dict()))
    # the whole run
    target = tiny(fill=0.5)
    opt2 = torch.optim.AdamW(target.parameters(), lr=1e-2, weight_decay=1e-4)
    sched2 = torch.optim.lr_scheduler.MultiStepLR(opt2, milestones=[2, 5], gamma=0.1)
    config = SimpleNamespace(pretrained_path=path)
    assert cu.resume_checkpoint(config, target, opt2, sched2, printer=lambda s: None) == (5, 0.75)
    assert config.start_epoch == 5 and config.epoch == 5
    same_tensors(dict(target.state_dict()), dict(m.state_dict()))
    assert sched2.state_dict() == sched.state_dict()
    for p, q in zip(m.parameters(), target.parameters()):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[p][k], opt2.state[q][k]), k
    # ... and the two runs continue alike
    for model, o in ((m, opt), (target, opt2)):
        torch.manual_seed(9)
        model(torch.randn(5, 4)).square().sum().backward()
        o.step()
    same_tensors(dict(target.state_dict()), dict(m.state_dict()))


def test_written_layout_is_the_references(tmp_path, golden):
    from geot_amd.openpoints.utils import ckpt_util as cu
    want = golden[0]["written"]
    m, opt, sched = trained(0)
    cfg = SimpleNamespace(run_name="golden", ckpt_dir=str(tmp_path), save_freq=2)
    cu.save_checkpoint(cfg, m, 4, optimizer=opt, scheduler=sched, additioanl_dict={"best_val": 0.75}, is_best=True)
    assert sorted(os.listdir(tmp_path)) == want["files"]
    for name in want["files"]:
        wrote = torch.load(tmp_path / name, map_location="cpu", weights_only=True)
        assert list(wrote) == want["keys"]
        assert wrote["epoch"] == want["epoch"] and wrote["best_val"] == want["best_val"]
        assert {k: list(v.shape) for k, v in wrote["model"].items()} == want["model"]
        assert list(wrote["optimizer"]) == want["optimizer"]["keys"]
        assert {str(i): sorted(st) for i, st in wrote["optimizer"]["state"].items()} == want["optimizer"]["state"]
        assert {"params", "lr", "betas", "eps", "weight_decay"} <= set(wrote["optimizer"]["param_groups"][0])
        assert {"milestones", "gamma", "last_epoch"} <= set(wrote["scheduler"]) and {"milestones", "gamma", "last_epoch"} <= set(want["scheduler"])


def test_load_checkpoint_reads_what_the_reference_read(tmp_path, golden):
    from geot_amd.openpoints.utils import ckpt_util as cu
    meta, arrays = golden
    path = str(tmp_path / "pretrained.pth")
    torch.save({"model": part(arrays, "in_load."), "epoch": 7, "best_val": 0.5, "val_miou": 0.25, "test_accs": [0.5, 0.25],
                "note": "x"}, path)
    target = tiny(fill=0.5)
    epoch, metrics = cu.load_checkpoint(target, path)
    assert epoch == meta["load"]["epoch"] and metrics == meta["load"]["metrics"]
    same_tensors(dict(target.state_dict()), dict(part(arrays, "load.")))
    assert torch.equal(target.head.bias, torch.full((2,), 0.5))          # (the entry the file lacks: left alone)
    assert list(cu.load_checkpoint(target, path, return_pretrained_keys=True)) == list(part(arrays, "in_load."))


def test_resume_checkpoint_reads_what_the_reference_read(tmp_path, golden):
    from geot_amd.openpoints.utils import ckpt_util as cu
    meta, arrays = golden
    _, opt, sched = trained(1)          # (the script's second run: its optimizer and scheduler states)
    exp_avg = part(arrays, "in_resume_exp_avg.")
    for i, st in opt.state_dict()["state"].items():
        assert torch.equal(st["exp_avg"], exp_avg[str(i)]), "the fixture's run is not reproduced: %d" % i
    path = str(tmp_path / "resume.pth")
    torch.save({"model": part(arrays, "in_resume."), "optimizer": opt.state_dict(), "scheduler": sched.state_dict(), "epoch": 7,
                "best_val": 0.5}, path)
    target = tiny(fill=0.5)
    opt2 = torch.optim.AdamW(target.parameters(), lr=1e-2, weight_decay=1e-4)
    sched2 = torch.optim.lr_scheduler.MultiStepLR(opt2, milestones=[2, 5], gamma=0.1)
    config = SimpleNamespace(pretrained_path=path)
    start, best = cu.resume_checkpoint(config, target, opt2, sched2, printer=lambda s: None)
    want = meta["resume"]
    assert (start, best, config.start_epoch, config.epoch) == (want["start_epoch"], want["best_val"], want["config_start_epoch"],
                                                               want["config_epoch"])
    assert sched2.last_epoch == want["last_epoch"] and opt2.param_groups[0]["lr"] == want["lr"]
    assert [float(opt2.state[p]["step"]) for p in target.parameters()] == want["steps"]
    same_tensors(dict(target.state_dict()), dict(part(arrays, "resume.")))
    for i, p in enumerate(target.parameters()):
        assert torch.equal(opt2.state[p]["exp_avg"], arrays["resume_exp_avg.%d" % i]), i


@pytest.mark.parametrize("wrapper", [None, "model", "net", "network", "state_dict", "base_model"])
@pytest.mark.parametrize("prefixed", [False, True])
def test_bare_and_wrapped_and_prefixed_files_load(tmp_path, wrapper, prefixed):
    from geot_amd.openpoints.utils import ckpt_util as cu
    torch.manual_seed(3)
    src = tiny()
    weights = OrderedDict((("module." + k) if prefixed else k, v) for k, v in src.state_dict().items())
    path = str(tmp_path / "w.pth")
    torch.save(weights if wrapper is None else {wrapper: weights, "epoch": 2}, path)
    for target in (tiny(fill=0.5), SimpleNamespace(module=tiny(fill=0.5))):          # bare, and inside a DDP-like wrapper
        epoch, metrics = cu.load_checkpoint(target, path)
        assert epoch == (-1 if wrapper is None else 2) and metrics == {}
        same_tensors(dict(getattr(target, "module", target).state_dict()), dict(src.state_dict()))


def test_a_wrapped_model_is_saved_without_the_prefix(tmp_path):
    from geot_amd.openpoints.utils import ckpt_util as cu
    m, opt, sched = trained(0)
    cfg = {"run_name": "run", "ckpt_dir": str(tmp_path), "save_freq": 0}
    path = cu.save_checkpoint(cfg, SimpleNamespace(module=m), 1, optimizer=opt, scheduler=sched)
    assert list(torch.load(path, weights_only=True)["model"]) == list(m.state_dict())
    with pytest.raises(NotImplementedError):
        cu.load_checkpoint(m, str(tmp_path / "nothing.pth"))


def test_rng_state_restores_the_host_generators():
    from geot_amd import checkpoint as ck
    torch.manual_seed(4), np.random.seed(5), random.seed(6)
    np.random.standard_normal(3), random.gauss(0, 1)        # (an odd number of gaussians: both keep a cached one)
    state = ck.rng_state()
    assert state["cuda"] is None

    def draws():
        return (torch.rand(4), torch.randperm(9), np.random.rand(4), np.random.standard_normal(3), np.random.permutation(7),
                random.random(), random.gauss(0, 1), random.sample(range(100), 5))
    first = draws()
    again = draws()
    assert not torch.equal(first[0], again[0]) and first[5] != again[5] and not np.array_equal(first[2], again[2])
    ck.set_rng_state(state)
    for a, b in zip(first, draws()):
        assert torch.equal(a, b) if torch.is_tensor(a) else np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b


def test_rng_state_survives_a_weights_only_file(tmp_path):
    from geot_amd import checkpoint as ck
    torch.manual_seed(4), np.random.seed(5), random.seed(6)
    torch.save(ck.rng_state(), tmp_path / "rng.pt")
    want = (torch.rand(3), np.random.rand(3), random.random())
    ck.set_rng_state(torch.load(tmp_path / "rng.pt", weights_only=True))
    got = (torch.rand(3), np.random.rand(3), random.random())
    assert torch.equal(want[0], got[0]) and np.array_equal(want[1], got[1]) and want[2] == got[2]
    with pytest.raises(ValueError, match="numpy"):
        ck.set_rng_state({k: v for k, v in ck.rng_state().items() if k != "numpy"})


class _Step:
    def __init__(self, state):
        self.state, self.loaded = state, None

    def state_dict(self):
        return self.state

    def load_state_dict(self, state):
        self.loaded = state


def test_save_is_atomic_and_load_returns_extra(tmp_path):
    from geot_amd import checkpoint as ck
    from geot_amd.openpoints.dataset.sample_draw import DeviceDraws
    path = tmp_path / "ckpt.pt"
    draws = DeviceDraws(7, counter=(1 << 64) - 3, views=True)
    ck.save(path, _Step({"w": torch.arange(3.0)}), draws=(draws,), epoch=3, best={"miou": 0.5})
    before = path.read_bytes()
    assert os.listdir(tmp_path) == ["ckpt.pt"]
    with pytest.raises(Exception):
        ck.save(path, _Step({"w": lambda: None}), epoch=4)          # (serialisation raises half-way through the file)
    assert os.listdir(tmp_path) == ["ckpt.pt"] and path.read_bytes() == before          # no partial file; the old one stands
    with pytest.raises(Exception):
        ck.save(tmp_path / "other.pt", _Step({"w": lambda: None}))
    assert os.listdir(tmp_path) == ["ckpt.pt"]
    step, fresh = _Step(None), DeviceDraws(0)
    assert ck.load(path, step, draws=(fresh,)) == {"epoch": 3, "best": {"miou": 0.5}}
    assert torch.equal(step.loaded["w"], torch.arange(3.0)) and fresh.state() == draws.state()
    with pytest.raises(ValueError, match="draws"):
        ck.load(path, _Step(None))
    assert set(torch.load(path, weights_only=True)) == {"format", "step", "draws", "rng", "extra"}


def test_optimizer_restore_is_in_place_and_torch_loads_the_entry():
    from geot_amd import checkpoint as ck
    m, opt, _ = trained(0)
    opt.param_groups[0]["lr"] = torch.tensor(0.02)          # a tensor lr, as a replayed step keeps it
    entry = ck.optimizer_state(opt)
    assert torch.is_tensor(entry["param_groups"][0]["lr"])          # (copied, not read: state_dict() does not synchronise)
    stored = ck.numbers_only({"optimizer": entry})["optimizer"]
    assert stored["param_groups"][0]["lr"] == pytest.approx(0.02) and isinstance(stored["param_groups"][0]["lr"], float)
    # copies: a further step leaves the entry alone
    kept = {i: {k: v.clone() for k, v in st.items()} for i, st in entry["state"].items()}
    m(torch.ones(5, 4)).sum().backward()
    opt.step()
    for i, st in entry["state"].items():
        for k, v in st.items():
            assert torch.equal(v, kept[i][k]), (i, k)
    # in place: the state tensors and the lr tensor keep their memory
    ptrs = [opt.state[p][k].data_ptr() for p in m.parameters() for k in ("step", "exp_avg", "exp_avg_sq")]
    lr = opt.param_groups[0]["lr"]
    lr.fill_(0.5)
    r = ck.Restore()
    r.optimizer("optimizer", opt, stored)
    r.commit()
    assert ptrs == [opt.state[p][k].data_ptr() for p in m.parameters() for k in ("step", "exp_avg", "exp_avg_sq")]
    assert opt.param_groups[0]["lr"] is lr and float(lr) == pytest.approx(0.02)
    for i, p in enumerate(m.parameters()):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[p][k], kept[i][k]), (i, k)
    # a fresh optimizer: the state is created, then filled; and torch's own loader takes the stored entry
    m2 = tiny()
    fresh = torch.optim.AdamW(m2.parameters(), lr=1e-2, weight_decay=1e-4)
    r = ck.Restore()
    r.optimizer("optimizer", fresh, stored)
    r.commit()
    plain = torch.optim.AdamW(tiny().parameters(), lr=1e-2, weight_decay=1e-4)
    plain.load_state_dict(stored)
    for i, (p, q) in enumerate(zip(m2.parameters(), plain.param_groups[0]["params"])):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(fresh.state[p][k], plain.state[q][k]) and torch.equal(fresh.state[p][k], kept[i][k]), (i, k)
    assert fresh.param_groups[0]["lr"] == pytest.approx(0.02) and plain.param_groups[0]["lr"] == pytest.approx(0.02)


def test_optimizer_restore_refuses_before_it_writes():
    from geot_amd import checkpoint as ck
    m, opt, _ = trained(0)
    entry = ck.optimizer_state(opt)
    before = {(i, k): v.clone() for i, p in enumerate(m.parameters()) for k, v in opt.state[p].items()}
    missing = dict(entry, state={i: st for i, st in entry["state"].items() if i != 2})
    shaped = dict(entry, state={i: dict(st, exp_avg=torch.zeros(5)) if i == 3 else st for i, st in entry["state"].items()})
    groups = dict(entry, param_groups=[{k: v for k, v in entry["param_groups"][0].items() if k != "betas"}])
    for bad, name in ((missing, r"optimizer\.state.*2"), (shaped, r"optimizer\.state\[3\]\.exp_avg"), (groups, "betas"),
                      ({"state": entry["state"]}, "param_groups")):
        r = ck.Restore()
        with pytest.raises(ValueError, match=name):
            r.optimizer("optimizer", opt, bad)
    for (i, k), v in before.items():
        assert torch.equal(opt.state[list(m.parameters())[i]][k], v)
