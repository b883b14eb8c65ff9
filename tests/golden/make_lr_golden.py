"""Regenerate the REFERENCE-EXECUTED fixture of the learning-rate schedule (where the reference tree is present).

    python tests/golden/make_lr_golden.py

What runs is the reference's own MultiStepLRScheduler (openpoints/scheduler/multistep_lr.py on its base class,
openpoints/scheduler/scheduler.py), built with the arguments build_scheduler_from_cfg (scheduler_factory.py:78-86) hands it,
on a one-group torch.optim.SGD on the CPU.  The two files are loaded by path under the module names their own import line
uses (the package's __init__ pulls in every model and is not imported).  Stored are get_epoch_values(t)[0] for t = 0..300 as
float64 and a provenance string -- no reference text:

    multistep_210_270   cfgs/tooth_semi/default.yaml: lr 1e-3, decay_epochs [210, 270], decay_rate 0.1, no warm-up
    multistep_220       cfgs/tooth_semi/transformer_finetune_fixmatch_ntm.yaml: decay_epochs [220]
    warmup_3            warmup_epochs 3, warmup_lr 1e-6, decay_epochs [5, 8]
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_ckpt_golden import REF      # noqa: E402  (where the sibling scripts look for the reference tree)
CASES = {"multistep_210_270": dict(lr=1e-3, decay_epochs=[210, 270], decay_rate=0.1, warmup_epochs=0, warmup_lr=1.0e-6),
         "multistep_220": dict(lr=1e-3, decay_epochs=[220], decay_rate=0.1, warmup_epochs=0, warmup_lr=1.0e-6),
         "warmup_3": dict(lr=1e-3, decay_epochs=[5, 8], decay_rate=0.1, warmup_epochs=3, warmup_lr=1.0e-6)}
EPOCHS = 301


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    module = importlib.util.module_from_spec(spec)
    sys.modules[name] = module
    spec.loader.exec_module(module)
    return module


def ref_class():
    for pkg in ("openpoints", "openpoints.scheduler"):
        sys.modules.setdefault(pkg, types.ModuleType(pkg))
    _load("openpoints.scheduler.scheduler", "openpoints/scheduler/scheduler.py")
    return _load("openpoints.scheduler.multistep_lr", "openpoints/scheduler/multistep_lr.py").MultiStepLRScheduler


def main():
    cls = ref_class()
    arrays = {}
    for name, c in CASES.items():
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=c["lr"])
        sched = cls(opt, decay_t=c["decay_epochs"], decay_rate=c["decay_rate"], warmup_lr_init=c["warmup_lr"],
                    warmup_t=c["warmup_epochs"], noise_range_t=None, noise_pct=0.67, noise_std=1.0, noise_seed=42)
        arrays[name] = np.array([sched.get_epoch_values(t)[0] for t in range(EPOCHS)], dtype=np.float64)
    arrays["provenance"] = np.array("MultiStepLRScheduler.get_epoch_values (openpoints/scheduler/multistep_lr.py:55-59) on a "
                                    "one-group SGD, epochs 0..300, torch %s" % torch.__version__)
    np.savez(os.path.join(HERE, "lr_schedule_ref.npz"), **arrays)
    print("wrote lr_schedule_ref.npz (%s)" % ", ".join(CASES))


if __name__ == "__main__":
    main()
