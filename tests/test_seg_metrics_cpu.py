"""CPU suite: read()'s host half (geot_amd.validation.seg_metrics_from_counts) and the tests' own restatement of the
reference (tests/_seg_metrics_ref.py) against tests/golden/seg_metrics_ref.npz -- what the reference's get_seg_metrics and
validate (examples/segmentation/train.py:802-832, 716-779) returned when executed in place -- every value and dtype, NaN
matching NaN.  The counts here come from np.bincount; the GPU tests feed the same host half from the kernel."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _seg_metrics_ref as ref  # noqa: E402
from _seg_metrics_ref import quiet  # noqa: E402


@pytest.fixture(scope="module")
def fix():
    return ref.load_fixture()


def test_fixture_was_recorded_under_the_installed_numpy_and_torch():
    ref.load_fixture()


def test_a_version_mismatch_fails_with_a_message(tmp_path, monkeypatch):
    f = dict(np.load(ref.FIXTURE, allow_pickle=False))
    f["numpy_version"] = np.array("1.26.4")
    path = tmp_path / "old.npz"
    np.savez(path, **f)
    monkeypatch.setattr(ref, "FIXTURE", str(path))
    with pytest.raises(AssertionError, match="recorded under numpy 1.26.4"):
        ref.load_fixture()


@pytest.mark.parametrize("tag", ["e0", "e1", "gsm"])
def test_host_arithmetic_on_bincount_counts_equals_the_reference(fix, tag):
    from geot_amd.validation import seg_metrics_from_counts
    pairs, cls, _ = ref.scans(fix, tag)
    counts = np.stack([ref.bincount_counts(p, lab, ref.C) for p, lab in pairs])
    with quiet():
        out = seg_metrics_from_counts(counts, ref.C, [c == 0 for c in cls])
    ref.check_lists((out["acc_list"], out["miou_list"], out["mdsc_list"]), fix, tag)
    assert out["scans"] == len(pairs) and out["labels_out_of_range"] == 0
    if tag != "gsm":
        ref.check_jaws(out, fix, tag)


@pytest.mark.parametrize("tag", ["e0", "e1", "gsm"])
def test_the_restatement_equals_the_reference(fix, tag):
    """Pins the restatement the GPU tests compare the device path with."""
    pairs, cls, batches = ref.scans(fix, tag)
    acc, miou, mdsc = [], [], []
    at = 0
    with quiet():
        for b in batches:
            part = pairs[at:at + b]
            a, i, d = ref.get_seg_metrics_ref([torch.from_numpy(p)[None] for p, _ in part], [torch.from_numpy(lab) for _, lab in part])
            acc, miou, mdsc = acc + a, miou + i, mdsc + d
            at += b
        ref.check_lists((acc, miou, mdsc), fix, tag)
        if tag != "gsm":
            ref.check_jaws(ref.aggregate_ref(acc, miou, mdsc, cls), fix, tag)


def test_a_label_outside_the_classes_is_refused_with_its_count():
    from geot_amd.validation import seg_metrics_from_counts
    label = np.array([0, 3, 17, -1, 3, 255], np.int64)
    counts = ref.bincount_counts(np.zeros(6, np.int64), label, ref.C)[None]
    with pytest.raises(RuntimeError, match="3 labels outside"):
        seg_metrics_from_counts(counts, ref.C, [True])
