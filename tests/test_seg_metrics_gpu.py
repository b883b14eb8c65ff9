"""The validation metrics on the device (geot_amd/validation.py over csrc/seg_metrics.hip), all comparisons exact (`==`,
NaN matching NaN, dtype included): the confusion counts against a torch.bincount restatement, the fused interpolate +
arg-max + count path against bincount(label, get_pred_whole(...)) -- the unfused chain, not an oracle --, read() /
get_seg_metrics / validate against the reference's own values (tests/golden/seg_metrics_ref.npz) and the restated
reference statements, and neither update synchronising with the host."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _seg_metrics_ref as ref  # noqa: E402
from _seg_metrics_ref import quiet  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SMALL = dict(trans_dim=384, depth=3, num_heads=4, group_size=32, num_group=128, encoder_dims=256, nclasses=17,
             drop_path_rate=0.0, downsample_targets=[2048, 1024, 512], extract_layers=[1, 2, 3])


def _offsets(sizes):
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=DEV)


def _want_counts(preds, labels, c):
    slots = c * (c + 1) + 1
    return torch.stack([torch.bincount(ref.torch_keys(p, lab, c), minlength=slots) for p, lab in zip(preds, labels)])


def _scan_data(g, m, c):
    """Labels in runs plus noise and a few outside [0, c); predictions = labels, 20 % replaced by values in [-2, c + 3)
    and some 255."""
    runs = torch.randint(0, c, (m // 97 + 1,), generator=g)
    label = runs.repeat_interleave(97)[:m].clone()
    noise = torch.rand(m, generator=g)
    label[noise < 0.05] = torch.randint(0, c, (int((noise < 0.05).sum()),), generator=g)
    label[noise > 0.998] = -1
    label[(noise > 0.996) & (noise <= 0.998)] = c
    pred = label.clone()
    flip = torch.rand(m, generator=g) < 0.2
    pred[flip] = torch.randint(-2, c + 3, (int(flip.sum()),), generator=g)
    pred[torch.rand(m, generator=g) < 0.01] = 255
    return pred.to(DEV), label.to(DEV)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 4097, 100003])
@pytest.mark.parametrize("c", [1, 2, 5, 17, 32])
def test_confusion_counts_equal_bincount(c, m):
    """1-4 ragged scans in one launch (the first of M vertices), accumulated over two launches."""
    from geot_amd.ext._common import call, ptr
    b = 1 + (m + c) % 4
    sizes = [m] + [(m * (k + 2)) // 3 + k for k in range(b - 1)]
    g = torch.Generator().manual_seed(1000 * c + m)
    counts = torch.zeros((b, c * (c + 1) + 1), dtype=torch.int64, device=DEV)
    want = torch.zeros_like(counts)
    for _ in range(2):
        data = [_scan_data(g, s, c) for s in sizes]
        preds, labels = [p for p, _ in data], [lab for _, lab in data]
        offs, pred, label = _offsets(sizes), torch.cat(preds), torch.cat(labels)      # alive until the launch is queued
        call("geot_seg_confusion", DEV, b, c, ptr(offs), ptr(pred), ptr(label), ptr(counts))
        want += _want_counts(preds, labels, c)
    assert torch.equal(counts, want), (counts - want).abs().sum().item()


def test_confusion_refuses_bad_sizes_and_takes_an_empty_batch():
    from geot_amd.ext._common import call, ptr
    pred, label = _scan_data(torch.Generator().manual_seed(5), 100, 17)
    offs = _offsets([100])
    counts = torch.zeros((1, 17 * 18 + 1), dtype=torch.int64, device=DEV)
    prob, idx, d2 = torch.rand(1, 17, 8, device=DEV), torch.zeros(100, 3, dtype=torch.int32, device=DEV), torch.rand(100, 3, device=DEV)
    for b, c in ((1, 0), (1, 33), (-1, 17)):
        with pytest.raises(RuntimeError, match="hipError 1"):
            call("geot_seg_confusion", DEV, b, c, ptr(offs), ptr(pred), ptr(label), ptr(counts))
        with pytest.raises(RuntimeError, match="hipError 1"):
            call("geot_seg_confusion_interp", DEV, b, c, 8, ptr(offs), ptr(prob), ptr(idx), ptr(d2), ptr(label), ptr(counts))
    call("geot_seg_confusion", DEV, 0, 17, ptr(offs), ptr(pred), ptr(label), ptr(counts))
    call("geot_seg_confusion_interp", DEV, 0, 17, 8, ptr(offs), ptr(prob), ptr(idx), ptr(d2), ptr(label), ptr(counts))
    assert int(counts.abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ fused path
def _fused_equals_unfused(logits, pts, wholes, centers, scales, labels):
    from geot_amd.validation import SegMetrics, get_pred_whole
    c = logits.shape[1]
    metrics = SegMetrics(c, DEV)
    metrics.update_from_logits(logits, pts, wholes, centers, scales, labels, [0] * len(wholes))
    got = metrics.counts[:len(wholes)]
    preds = get_pred_whole(logits, pts, wholes, centers, scales)
    want = _want_counts([p.reshape(-1) for p in preds], [lab.to(DEV).reshape(-1) for lab in labels], c)
    diff = (got - want).abs().sum().item()
    print("fused vs unfused: %d vertices, counts differ by %d" % (sum(int(lab.numel()) for lab in labels), diff))
    assert torch.equal(got, want)
    return preds


def test_fused_path_at_the_size_of_a_real_scan():
    """N = 24 000 sampled, M = 100 003 vertices, C = 17, as test_fullsize_gpu.py builds the validation path."""
    from geot_amd.synth import make_batch, make_cloud, region_labels
    rng = np.random.default_rng(21)
    n, m, c = 24000, 100003, 17
    pts = make_batch(1, n, start_index=55)[0]
    whole = (make_cloud(m, 56)[0] * np.float32(1.02)).astype(np.float32)
    logits = (rng.normal(size=(1, c, n)) * 3).astype(np.float32)
    _fused_equals_unfused(torch.from_numpy(logits).to(DEV), torch.from_numpy(pts).to(DEV), [torch.from_numpy(whole)],
                          [torch.zeros(1, 3)], [torch.tensor(1.0)], [torch.from_numpy(region_labels(whole))])


def _two_scans(seed, n=16000, sizes=(60001, 38888)):
    """Two de-normalised scans of different size: sampled points normalised, vertices in scan coordinates."""
    from geot_amd.synth import make_batch, make_cloud, make_logits, region_labels
    pts = make_batch(2, n, start_index=seed)[0]
    centers = [np.array([[1.5, -20.25, 3.0]], np.float32), np.array([[-7.0, 0.5, 11.0]], np.float32)]
    scales = [np.float32(37.5), np.float32(29.0)]
    wholes = [(make_cloud(m, seed + 10 + i)[0] * np.float32(1.01) * scales[i] + centers[i]).astype(np.float32)
              for i, m in enumerate(sizes)]
    labels = [region_labels((w - centers[i]) / scales[i]) for i, w in enumerate(wholes)]
    return make_logits(pts, seed), pts, wholes, centers, scales, labels


def _dev(logits, pts, wholes, centers, scales, labels):
    return (torch.from_numpy(logits).to(DEV), torch.from_numpy(pts).to(DEV), [torch.from_numpy(w).to(DEV) for w in wholes],
            [torch.from_numpy(c).to(DEV) for c in centers], [torch.tensor(s).to(DEV) for s in scales],
            [torch.from_numpy(lab).to(DEV) for lab in labels])


def test_fused_path_two_scans_of_different_size():
    _fused_equals_unfused(*_dev(*_two_scans(3)))


def test_fused_path_with_exact_ties_nans_and_coincident_vertices():
    """Logits tied exactly between classes 3 and 5 as the maximum at half the sampled points (first index wins), NaN logits
    at a few sampled points (their soft-max is NaN in every class: the first NaN, class 0, wins wherever they are a
    neighbour), and vertices that coincide with de-normalised sampled points (d = 0: weight 1 / 1e-8 before normalising)."""
    logits, pts, wholes, centers, scales, labels = _two_scans(9, n=12000, sizes=(40000, 25003))
    rng = np.random.default_rng(9)
    tie = rng.random(logits.shape[2]) < 0.5
    top = logits.max(1) + np.float32(2.0)
    logits[:, 3] = np.where(tie, top, logits[:, 3])
    logits[:, 5] = np.where(tie, top, logits[:, 5])
    logits[0, 7, rng.choice(logits.shape[2], 40, replace=False)] = np.nan
    logits[1, :, rng.choice(logits.shape[2], 25, replace=False)] = np.nan
    for i in range(2):
        on = rng.choice(pts.shape[1], 3000, replace=False)
        at = rng.choice(len(wholes[i]), 3000, replace=False)
        wholes[i][at] = (pts[i, on] * scales[i] + centers[i]).astype(np.float32)     # get_pred_whole's fp32 arithmetic
    preds = _fused_equals_unfused(*_dev(logits, pts, wholes, centers, scales, labels))
    assert all(int((p == 3).sum()) > 0 and int((p == 5).sum()) < int((p == 3).sum()) for p in preds)


# ------------------------------------------------------------------------------------------------ read / get_seg_metrics
def test_device_metrics_equal_the_reference_fixture():
    from geot_amd.validation import SegMetrics, get_seg_metrics
    fix = ref.load_fixture()
    pairs, _, _ = ref.scans(fix, "gsm")
    got = get_seg_metrics([torch.from_numpy(p).to(DEV)[None] for p, _ in pairs], [torch.from_numpy(lab).to(DEV) for _, lab in pairs])
    ref.check_lists(got, fix, "gsm")
    metrics = SegMetrics(17, DEV)
    for tag in ("e0", "e1"):                       # two epochs: reset() in between
        pairs, cls, batches = ref.scans(fix, tag)
        at = 0
        for b in batches:
            part = pairs[at:at + b]
            metrics.update([torch.from_numpy(p).to(DEV)[None] for p, _ in part], [torch.from_numpy(lab).to(DEV) for _, lab in part],
                           torch.from_numpy(cls[at:at + b]).reshape(b, 1))
            at += b
        with quiet():
            out = metrics.read()
        ref.check_lists((out["acc_list"], out["miou_list"], out["mdsc_list"]), fix, tag)
        ref.check_jaws(out, fix, tag)
        assert out["scans"] == len(pairs) and out["labels_out_of_range"] == 0
        metrics.reset()


def test_a_label_outside_the_classes_makes_read_raise():
    from geot_amd.validation import SegMetrics
    metrics = SegMetrics(17, DEV)
    pred, label = (torch.arange(50, device=DEV) % 17 for _ in range(2))
    metrics.update([pred], [label], [1])
    label = label.clone()
    label[[3, 9]] = torch.tensor([17, -1], device=DEV)
    metrics.update([pred], [label], [0])
    with pytest.raises(RuntimeError, match="2 labels outside"):
        metrics.read()
    metrics.reset()
    metrics.update([pred], [pred], [0])
    assert metrics.read()["scans"] == 1


# ------------------------------------------------------------------------------------------------ validate
def _loader(seed, jaws):
    """collate_fn_val-shaped batches (openpoints/dataset/build.py:30-50) of 2 scans, CPU tensors as the loader gives them."""
    batches = []
    for k, cls in enumerate(jaws):
        logits, pts, wholes, centers, scales, labels = _two_scans(seed + 20 * k, n=8000, sizes=(30011 + k, 20000 - 7 * k))
        batches.append({"pos": torch.from_numpy(pts), "x": torch.from_numpy(pts).clone(), "y": torch.zeros(2, 8000, dtype=torch.long),
                        "cls": torch.tensor(cls, dtype=torch.int64).reshape(2, 1),
                        "points": [torch.from_numpy(w) for w in wholes], "labels": [torch.from_numpy(lab) for lab in labels],
                        "center": [torch.from_numpy(c[0]) for c in centers], "scale": [torch.tensor(s) for s in scales],
                        "patient": ["p%d" % k, "q%d" % k]})
    return batches


class _Recorder:
    """Wraps a model; keeps every logits tensor it returned, in call order."""

    def __init__(self, model):
        self.model, self.logits = model, []

    def eval(self):
        self.model.eval()
        return self

    def __call__(self, data):
        out = self.model(data)
        self.logits.append(out[0].clone())
        return out


class _SeededLogits:
    def eval(self):
        return self

    def __call__(self, data):
        pos = data["pos"]
        k = torch.arange(17, device=pos.device, dtype=torch.float32)[None, :, None]
        return torch.sin(pos[:, None, :, 0] * (3.0 + k) + pos[:, None, :, 1] * k) * 4.0, None, None


def _restated_validate(batches, logits_per_batch):
    from geot_amd.validation import get_pred_whole
    acc, miou, mdsc, cls = [], [], [], []
    for data, logits in zip(batches, logits_per_batch):
        preds = get_pred_whole(logits, data["pos"].to(DEV), data["points"], data["center"], data["scale"])
        a, i, d = ref.get_seg_metrics_ref(preds, [lab.to(DEV) for lab in data["labels"]])
        acc, miou, mdsc, cls = acc + a, miou + i, mdsc + d, cls + [c for c in data["cls"]]
    return ref.aggregate_ref(acc, miou, mdsc, cls)


def _check_validate(model, batches):
    from geot_amd.validation import validate
    rec = _Recorder(model)
    cfg = type("Cfg", (), {"num_classes": 17, "epoch": 3, "epochs": 100})()
    with quiet():
        got = validate(rec, [dict(d) for d in batches], cfg)
        want = _restated_validate(batches, rec.logits)
    assert len(rec.logits) == len(batches)
    for g, k in zip(got, ("whole_macc", "whole_miou", "whole_mdsc")):
        print("validate %s: %r (restated %r)" % (k, g, want[k]))
        assert np.asarray(g).dtype == np.asarray(want[k]).dtype and ref.same_value(g, want[k]), (k, g, want[k])


def test_validate_equals_the_restated_reference_loop():
    _check_validate(_SeededLogits(), _loader(31, [[0, 1], [1, 1], [0, 0]]))


def test_validate_with_the_configured_model():
    from geot_amd.openpoints.models.segmentation import WholePartSeg
    torch.manual_seed(0)
    model = WholePartSeg(segmentor_args=dict(NAME="PointTransformer_seg_T", **SMALL)).to(DEV)
    _check_validate(model, _loader(77, [[0, 1]]))


# ------------------------------------------------------------------------------------------------ no host synchronisation
def test_updates_do_not_synchronise():
    """torch's sync debug mode raises on a synchronising HIP call (checked first: .item() under it raises here)."""
    from geot_amd.validation import SegMetrics
    logits, pts, wholes, centers, scales, labels = _dev(*_two_scans(5, n=8000, sizes=(20000, 9999)))
    preds = [torch.randint(0, 17, (1, len(lab)), device=DEV) for lab in labels]
    metrics = SegMetrics(17, DEV)
    metrics.update(preds, labels, [0, 1])                        # warm: the workspace / kernels / pinned pool
    metrics.update_from_logits(logits, pts, wholes, centers, scales, labels, [0, 1])
    metrics.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError, match="synchroniz"):
            logits.sum().item()
        for _ in range(5):                                       # past the first capacity (8 scans): growing does not sync
            metrics.update(preds, labels, torch.tensor([[0], [1]]))
            metrics.update_from_logits(logits, pts, wholes, centers, scales, labels, torch.tensor([[1], [0]]))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert metrics.read()["scans"] == 20
