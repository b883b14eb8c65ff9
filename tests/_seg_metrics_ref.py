"""Shared by the validation-metric tests (geot_amd/validation.py over csrc/seg_metrics.hip): the fixture the reference's
own get_seg_metrics / validate produced (tests/golden/make_seg_metrics_golden.py), a restatement of those reference
statements in the style of test_epoch_meters_gpu.py's ReferenceMeters, and exact (dtype-checking, NaN-matching)
comparisons."""
import contextlib
import math
import os
import warnings

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seg_metrics_ref.npz")
C = 17
JAW_KEYS = [jaw + "_" + m for jaw in ("mandible", "maxillary", "whole") for m in ("macc", "miou", "mdsc")]


@contextlib.contextmanager
def quiet():
    """Without numpy's empty-mean warnings (the reference's own, for a scan or a jaw without values)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        yield


def load_fixture():
    """The fixture, after checking that it was recorded under the installed numpy / torch major versions (the dtypes it
    pins come from numpy's promotion rules)."""
    fix = np.load(FIXTURE, allow_pickle=False)
    want = {"numpy": str(fix["numpy_version"]), "torch": str(fix["torch_version"])}
    have = {"numpy": np.__version__, "torch": torch.__version__}
    bad = [k for k in want if want[k].split(".")[0] != have[k].split(".")[0]]
    assert not bad, ("seg_metrics_ref.npz was recorded under %s, this is %s: a major version apart, the reference's dtypes "
                     "may differ -- regenerate it with tests/golden/make_seg_metrics_golden.py" %
                     (", ".join("%s %s" % (k, want[k]) for k in bad), ", ".join("%s %s" % (k, have[k]) for k in bad)))
    return fix


def scans(fix, tag):
    """[(pred int64, label int64)] per scan, and the jaw classes, batch sizes of the case."""
    ends = np.cumsum(fix[tag + "_sizes"])
    preds = np.split(fix[tag + "_preds"].astype(np.int64), ends[:-1])
    labels = np.split(fix[tag + "_labels"].astype(np.int64), ends[:-1])
    return list(zip(preds, labels)), fix[tag + "_cls"], [int(b) for b in fix[tag + "_batches"]]


def bincount_counts(pred, label, c):
    """One scan's counts in geot_seg_confusion's layout, with numpy."""
    col = np.where((pred >= 0) & (pred < c), pred, c)
    key = np.where((label >= 0) & (label < c), label * (c + 1) + col, c * (c + 1))
    return np.bincount(key, minlength=c * (c + 1) + 1)


def torch_keys(pred, label, c):
    """The same slots with torch ops (on the tensors' device), for torch.bincount."""
    col = torch.where((pred >= 0) & (pred < c), pred, torch.full_like(pred, c))
    return torch.where((label >= 0) & (label < c), label * (c + 1) + col, torch.full_like(label, c * (c + 1)))


def get_seg_metrics_ref(preds_whole, labels_whole):
    """train.py:802-832, restated: the per-scan accuracy, mIoU and DSC."""
    acc_list, miou_list, mdsc_list = [], [], []
    for index in range(len(preds_whole)):
        pred_whole = preds_whole[index].detach().squeeze().cpu()
        label_whole = labels_whole[index].unsqueeze(0).squeeze().cpu()
        iou, dsc = [], []
        for jcls in torch.unique(label_whole).cpu().numpy():
            if jcls == 0:
                continue
            jcls_and = torch.logical_and(pred_whole == jcls, label_whole == jcls).sum()
            jcls_or = torch.logical_or(pred_whole == jcls, label_whole == jcls).sum()
            iou.append((jcls_and / jcls_or).float())
            dsc.append((2 * iou[-1] / (1 + iou[-1])))
        acc_list.append((pred_whole == label_whole).sum() / (label_whole.view(-1).shape[0]))
        miou_list.append(np.array(iou).mean())
        mdsc_list.append(np.array(dsc).mean())
    return acc_list, miou_list, mdsc_list


def aggregate_ref(acc_list, miou_list, mdsc_list, cls):
    """train.py:747-763, restated: the jaw and whole means -> {JAW_KEYS: value}."""
    lo = {"acc": [], "miou": [], "dsc": []}
    up = {"acc": [], "miou": [], "dsc": []}
    for ii in range(len(acc_list)):
        side = lo if cls[ii] == 0 else up
        side["miou"].append(miou_list[ii])
        side["dsc"].append(mdsc_list[ii])
        side["acc"].append(acc_list[ii])
    out = {}
    for name, side in (("mandible", lo), ("maxillary", up)):
        out[name + "_macc"], out[name + "_miou"], out[name + "_mdsc"] = (np.array(side["acc"]).mean(),
                                                                         np.array(side["miou"]).mean(),
                                                                         np.array(side["dsc"]).mean())
    for key, name in (("acc", "whole_macc"), ("miou", "whole_miou"), ("dsc", "whole_mdsc")):
        out[name] = (np.array(lo[key]).sum() + np.array(up[key]).sum()) / (len(lo[key]) + len(up[key]))
    return out


def same_value(a, b):
    a, b = float(a), float(b)
    return (math.isnan(a) and math.isnan(b)) or a == b


def check_lists(got, fix, tag):
    """(acc_list, miou_list, mdsc_list) against the fixture's per-scan values and types."""
    acc, miou, mdsc = got
    bad = []
    for i, a in enumerate(acc):
        if not (torch.is_tensor(a) and a.dtype == torch.float32 and a.dim() == 0 and same_value(a, fix[tag + "_acc"][i])):
            bad.append("acc[%d]: %r != %r" % (i, a, fix[tag + "_acc"][i]))
    for name, lst in (("miou", miou), ("mdsc", mdsc)):
        for i, v in enumerate(lst):
            want, dt = fix["%s_%s" % (tag, name)][i], str(fix["%s_%s_dtype" % (tag, name)][i])
            if not (type(v).__name__ == dt and same_value(v, want)):
                bad.append("%s[%d]: %r != %s(%r)" % (name, i, v, dt, want))
    assert len(acc) == len(miou) == len(mdsc) == len(fix[tag + "_acc"]), (tag, len(acc), len(fix[tag + "_acc"]))
    assert not bad, (tag, bad[:10])


def check_jaws(got, fix, tag):
    """{JAW_KEYS: value} against the fixture's values and dtypes."""
    bad = []
    for k in JAW_KEYS:
        want = fix["%s_%s" % (tag, k)]
        if not (np.asarray(got[k]).dtype == want.dtype and same_value(got[k], want)):
            bad.append("%s: %r != %r" % (k, got[k], want[()]))
    assert not bad, (tag, bad)
