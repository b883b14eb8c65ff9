"""fit()'s cfg.val_whole on the GPU (geot_amd/fit.py _val_whole): "covered" and "decoded" report what validate_scans_covered /
validate_scans_decoded give for the student as it stands after the epoch, and neither changes a bit of the training run (the
set-up and the comparison helpers are tests/test_fit_gpu.py's, at one epoch)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_fit_gpu as tf  # noqa: E402
from _seg_metrics_ref import quiet  # noqa: E402

pytestmark = pytest.mark.gpu
ONE = dict(tf.CFG, epochs=1, decay_epochs=[99])
VAL_SEED = 5
_runs = {}


def _val_batcher():
    """The validation scans behind a ValBatcher with device draws from a fixed counter: two such objects yield the same batches."""
    from geot_amd.openpoints.dataset import ValBatcher
    from geot_amd.openpoints.dataset.sample_draw import DeviceDraws
    return ValBatcher(tf._sets()[2], tf.N, draws=DeviceDraws(VAL_SEED))


def _run(mode):
    """One epoch of tests/test_fit_gpu.py's run; mode None: no validation, "covered": the bare scan set, "decoded": a ValBatcher."""
    from geot_amd.fit import fit
    if mode not in _runs:
        step, batcher = tf._new(5, None)
        tf._seed(11)
        val = None if mode is None else tf._sets()[2] if mode == "covered" else _val_batcher()
        with quiet():
            out = fit(step, batcher, ONE if mode is None else dict(ONE, val_whole=mode), val=val, log=lambda rec: None,
                      generator=torch.Generator().manual_seed(tf.SAMPLER_SEED))
        _runs[mode] = {"step": step, "out": out, "final": tf.snap(step.state_dict())}
    return _runs[mode]


@pytest.mark.parametrize("mode", ["covered", "decoded"])
def test_val_whole_reports_its_validator_and_leaves_training_alone(mode):
    from geot_amd import validation
    from geot_amd.openpoints.dataset.sample_draw import DeviceDraws
    plain, run = _run(None), _run(mode)
    tf.same(run["final"], plain["final"], "the training state behind a run validated with val_whole=%s" % mode)
    rec = run["out"]["records"][-1]
    model = run["step"].model
    was = model.training
    cfg = dict(num_points=tf.N, num_classes=17, epoch=1, epochs=1)
    with quiet(), torch.no_grad():
        if mode == "covered":       # fit() gives a bare scan set a fresh DeviceDraws(cfg.seed or 0) per validation
            want = validation.validate_scans_covered(model, tf._sets()[2], cfg, draws=DeviceDraws(0), batch_size=2)
        else:                       # the batcher's own draws, from the counter fit() found them at
            want = validation.validate_scans_decoded(model, _val_batcher(), cfg, batch_size=2)
            # ... which is get_seg_metrics' aggregate on decode_scans' labels of the same batch
            scans = tf._sets()[2]
            preds = validation.decode_scans(model.eval(), _val_batcher(), [0, 1])
            labels = list(torch.split(scans.labels.to(torch.int64), scans.sizes))
            acc, miou, mdsc = validation.get_seg_metrics(preds, labels, 17)
            metrics = validation.SegMetrics(17, tf.DEV)
            metrics.update(preds, labels, [0, 1])
            out = metrics.read()
            assert [float(v) for v in out["miou_list"]] == [float(v) for v in miou] and [float(v) for v in out["acc_list"]] == [float(v) for v in acc]
            assert all(float(g) == float(out[k]) for g, k in zip(want, ("whole_macc", "whole_miou", "whole_mdsc")))
            assert 0.0 < float(want[0]) < 1.0
    model.train(was)
    got = (rec["val_acc"], rec["val_miou"], rec["val_dsc"])
    assert all(float(g) == float(w) for g, w in zip(got, want)), (got, want)        # the same batches, the same numbers
    assert rec["best_val_miou"] == rec["val_miou"] and run["out"]["best_epoch"] == 1
