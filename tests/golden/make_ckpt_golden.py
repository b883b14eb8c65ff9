"""Regenerate the REFERENCE-EXECUTED fixture of the checkpoint format (BUILD container only: /root/reference does not
exist on the GPU box).

    python tests/golden/make_ckpt_golden.py

What runs is the reference's own ``save_checkpoint`` / ``resume_checkpoint`` / ``load_checkpoint``
(openpoints/utils/ckpt_util.py:69-222), on a tiny nn.Module, AdamW and MultiStepLR, on the CPU.  The module itself does not
import here (``termcolor`` is not installed), so the three functions and the helpers they call are taken out of the file
with ``ast``, as make_ntm_golden.py does, compiled with the reference file as their filename and executed; the names its
import lines would have bound are supplied.  No reference source text is written anywhere, and no pickle:

    ckpt_ref.json   the key layout save_checkpoint wrote (file names, top-level keys, model keys and shapes, the optimizer's
                    and the scheduler's keys); what load_checkpoint / resume_checkpoint returned for the dicts built below
                    (epoch, metric dict, start_epoch, best_val, the optimizer's step, the scheduler's last_epoch)
    ckpt_ref.npz    in_load.* / in_resume.*: the model tensors of the two dicts this script builds (with a ``module.``
                    prefix, one entry the model lacks, one entry of the model left out -- the non-strict case); load.* /
                    resume.*: the tiny model's tensors after the reference loaded them; resume_exp_avg.*: the optimizer's
"""
import ast
import json
import logging
import os
import shutil
import tempfile
from collections import OrderedDict, defaultdict
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
CKPT = "openpoints/utils/ckpt_util.py"
NAMES = ("save_checkpoint", "resume_checkpoint", "load_checkpoint", "get_missing_parameters_message",
         "get_unexpected_parameters_message", "_group_checkpoint_keys", "_group_to_str", "bert2vit_ckpt_rename")


def ref_functions():
    import typing
    path = os.path.join(REF, CKPT)
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    picked = [n for n in tree.body if getattr(n, "name", None) in NAMES]
    assert {n.name for n in picked} == set(NAMES), sorted(set(NAMES) - {n.name for n in picked})
    ns = {"logging": logging, "os": os, "shutil": shutil, "torch": torch, "nn": nn, "OrderedDict": OrderedDict,
          "defaultdict": defaultdict, "colored": lambda text, *a, **k: text}
    ns.update({k: getattr(typing, k) for k in ("Any", "Optional", "List", "Dict", "NamedTuple", "Tuple", "Iterable")})
    exec(compile(ast.Module(body=picked, type_ignores=[]), path, "exec"), ns)
    provenance = {n.name: "%d-%d" % (n.lineno, n.end_lineno) for n in picked if n.name in NAMES[:3]}
    return ns, provenance


def tiny(fill=None):
    """The tiny module of the fixture (tests/test_checkpoint_cpu.py builds the same): fill: every tensor set to it."""
    m = nn.Sequential(OrderedDict(encoder=nn.Linear(4, 3), norm=nn.BatchNorm1d(3), head=nn.Linear(3, 2)))
    if fill is not None:
        with torch.no_grad():
            for t in m.state_dict().values():
                t.fill_(fill)
    return m


def trained(seed):
    torch.manual_seed(seed)
    m = tiny()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2, 5], gamma=0.1)
    for _ in range(3):
        m(torch.randn(5, 4)).square().sum().backward()
        opt.step()
        opt.zero_grad()
        sched.step()
    return m, opt, sched


def npy(sd):
    return {k: v.detach().cpu().numpy() for k, v in sd.items()}


def main():
    ns, provenance = ref_functions()
    out, arrays = {"reference": provenance, "torch": torch.__version__}, {}
    work = tempfile.mkdtemp()
    try:
        # 1. what save_checkpoint writes
        m, opt, sched = trained(0)
        cfg = SimpleNamespace(run_name="golden", ckpt_dir=work, save_freq=2)
        ns["save_checkpoint"](cfg, m, 4, optimizer=opt, scheduler=sched, additioanl_dict={"best_val": 0.75}, is_best=True)
        files = sorted(os.listdir(work))
        wrote = torch.load(os.path.join(work, "golden_ckpt_latest.pth"), map_location="cpu", weights_only=True)
        out["written"] = {
            "files": files, "keys": list(wrote), "epoch": wrote["epoch"], "best_val": wrote["best_val"],
            "model": {k: list(v.shape) for k, v in wrote["model"].items()},
            "optimizer": {"keys": list(wrote["optimizer"]), "state": {str(i): sorted(st) for i, st in wrote["optimizer"]["state"].items()},
                          "param_group_keys": sorted(wrote["optimizer"]["param_groups"][0])},
            "scheduler": sorted(wrote["scheduler"])}
        # 2. what load_checkpoint reads: module.-prefixed keys under "model", one entry too many, one missing
        m, opt, sched = trained(1)
        weights = OrderedDict(("module." + k, v.clone()) for k, v in m.state_dict().items() if k != "head.bias")
        weights["module.extra.weight"] = torch.ones(2, 2)
        path = os.path.join(work, "pretrained.pth")
        torch.save({"model": weights, "epoch": 7, "best_val": 0.5, "val_miou": 0.25, "test_accs": [0.5, 0.25], "note": "x"}, path)
        target = tiny(fill=0.5)
        epoch, metrics = ns["load_checkpoint"](target, path)
        out["load"] = {"epoch": epoch, "metrics": metrics}
        arrays.update({"in_load." + k: v for k, v in npy(weights).items()})
        arrays.update({"load." + k: v for k, v in npy(target.state_dict()).items()})
        # 3. what resume_checkpoint reads: the complete layout, module.-prefixed model keys into a bare model
        full = OrderedDict(("module." + k, v.clone()) for k, v in m.state_dict().items())
        path = os.path.join(work, "resume.pth")
        torch.save({"model": full, "optimizer": opt.state_dict(), "scheduler": sched.state_dict(), "epoch": 7, "best_val": 0.5}, path)
        target = tiny(fill=0.5)
        opt2 = torch.optim.AdamW(target.parameters(), lr=1e-2, weight_decay=1e-4)
        sched2 = torch.optim.lr_scheduler.MultiStepLR(opt2, milestones=[2, 5], gamma=0.1)
        config = SimpleNamespace(pretrained_path=path)
        start, best = ns["resume_checkpoint"](config, target, opt2, sched2)
        out["resume"] = {"start_epoch": start, "best_val": best, "config_start_epoch": config.start_epoch, "config_epoch": config.epoch,
                         "last_epoch": sched2.last_epoch, "lr": opt2.param_groups[0]["lr"],
                         "steps": [float(opt2.state[p]["step"]) for p in target.parameters()]}
        arrays.update({"in_resume." + k: v for k, v in npy(full).items()})
        arrays.update({"resume." + k: v for k, v in npy(target.state_dict()).items()})
        arrays.update({"in_resume_exp_avg.%d" % i: st["exp_avg"].numpy() for i, st in opt.state_dict()["state"].items()})
        arrays.update({"resume_exp_avg.%d" % i: opt2.state[p]["exp_avg"].numpy() for i, p in enumerate(target.parameters())})
    finally:
        shutil.rmtree(work)
    np.savez(os.path.join(HERE, "ckpt_ref.npz"), **arrays)
    with open(os.path.join(HERE, "ckpt_ref.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote ckpt_ref.npz (%d arrays), ckpt_ref.json" % len(arrays))


if __name__ == "__main__":
    main()
