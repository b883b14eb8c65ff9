"""Validation scoring per batch at the reference's operating point: B = 2 scans (batch_size_val: 2), N = 16 000 sampled
points (the authors' cloud size), ~1e5 vertices per scan, C = 17; the model's forward is not part of it.

    python tools/time_validation.py [--reps 60] [--warmup 5] [--only unfused|fused|resident] [--legs fused,resident]
    python tools/time_validation.py --end-to-end [--scans 16]

(a) unfused: get_pred_whole, then get_seg_metrics' statements (restated in tests/_seg_metrics_ref.py: the .cpu() copies,
    torch.unique, two passes per class) -- what a batch cost before SegMetrics;
(b) fused:   SegMetrics.update_from_logits + read() (a read per batch: more than the per-batch share of the one read an
    epoch needs).
(c) resident: SegMetrics.update_from_scans + read() on the same scans held in a DeviceScanSet: one geot_scan_predict call.
    It starts from the same device-resident logits and sampled points as (b), whose vertices and labels are device tensors
    too: neither leg pays PCIe inside the timed window.
The legs alternate, after warm-up; each repetition is device-synchronised wall time.  Conditions: median(b) <= median(a) +
spread(a), spread = p90 - p10 of (a) in this run (both paths share the three_nn that dominates them); median(c) <=
median(b) + spread(b).  Prints the bytes the fused and the resident kernel stream, for a TB/s figure from a rocprofv3
--kernel-trace time.

--end-to-end: the wall time of one whole evaluation pass over synthetic scans of ~1e5 vertices with the small configured
model, validate() over host batches (collate_fn_val's layout, CPU tensors, made before the clock starts) against
validate_scans() on a DeviceScanSet -- an end-to-end figure (model forward included), not a kernel's."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from geot_amd.synth import make_batch, make_cloud, make_logits, region_labels  # noqa: E402
from geot_amd.validation import SegMetrics, get_pred_whole, validate, validate_scans  # noqa: E402
from _seg_metrics_ref import get_seg_metrics_ref, quiet  # noqa: E402

B, N, C, SIZES = 2, 16000, 17, (100003, 98765)


def batch():
    dev = torch.device("cuda:0")
    pts = make_batch(B, N, start_index=400)[0]
    centers = [np.array([[2.0, -15.5, 4.25]], np.float32), np.array([[-3.0, 1.5, 9.0]], np.float32)]
    scales = [np.float32(36.0), np.float32(31.5)]
    wholes = [(make_cloud(m, 410 + i)[0] * np.float32(1.01) * scales[i] + centers[i]).astype(np.float32)
              for i, m in enumerate(SIZES)]
    labels = [region_labels((w - centers[i]) / scales[i]) for i, w in enumerate(wholes)]
    return (torch.from_numpy(make_logits(pts, 400)).to(dev), torch.from_numpy(pts).to(dev),
            [torch.from_numpy(w).to(dev) for w in wholes], [torch.from_numpy(c[0]).to(dev) for c in centers],
            [torch.tensor(s).to(dev) for s in scales], [torch.from_numpy(lab).to(dev) for lab in labels])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=("unfused", "fused", "resident"), default=None)
    ap.add_argument("--legs", default=None, help="comma-separated subset of unfused,fused,resident")
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--scans", type=int, default=16)
    args = ap.parse_args()
    if args.end_to_end:
        return end_to_end(args.scans)
    logits, pts, wholes, centers, scales, labels = batch()
    metrics = SegMetrics(C, logits.device)
    from geot_amd.openpoints.dataset import DeviceScanSet
    scans = DeviceScanSet(wholes, [lab.to(torch.int32) for lab in labels], cls=[0, 1], device=logits.device)
    held = {"pos": pts, "center": torch.stack(centers), "scale": torch.stack(scales), "scans": scans, "sizes": list(SIZES),
            "scan_ids": torch.arange(B, device=logits.device), "mandible": [True, False]}      # what ValBatcher.batch hands over

    def unfused():
        preds = get_pred_whole(logits, pts, wholes, centers, scales)
        return get_seg_metrics_ref(preds, labels)

    def fused():
        metrics.reset()
        metrics.update_from_logits(logits, pts, wholes, centers, scales, labels, [0, 1])
        return metrics.read()

    def resident():
        metrics.reset()
        metrics.update_from_scans(logits, held)
        return metrics.read()

    paths = {"unfused": unfused, "fused": fused, "resident": resident}
    names = [args.only] if args.only else (args.legs.split(",") if args.legs else list(paths))
    if not names or any(k not in paths for k in names):
        ap.error("--legs takes a comma-separated subset of %s" % ",".join(paths))
    times = {k: [] for k in names}

    def lists(out):
        return list(out[1]) + list(out[2]) if isinstance(out, tuple) else out["miou_list"] + out["mdsc_list"]

    with torch.no_grad(), quiet():
        first = [lists(paths[k]()) for k in names]        # the legs that are timed give the same numbers (a lone leg: nothing to compare)
        same = all(len(v) == len(first[0]) and all(float(x) == float(y) for x, y in zip(v, first[0])) for v in first[1:])
        for i in range(args.warmup + args.reps):
            for k in (names if i % 2 == 0 else names[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                paths[k]()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
    res = {"B": B, "N": N, "C": C, "M": list(SIZES), "reps": args.reps, "same_values": same}
    for k, ts in times.items():
        p10, med, p90 = np.percentile(ts, [10, 50, 90])
        res[k] = {"median_ms": round(float(med), 4), "p10_ms": round(float(p10), 4), "p90_ms": round(float(p90), 4)}
    if "unfused" in times and "fused" in times:
        margin = res["unfused"]["p90_ms"] - res["unfused"]["p10_ms"]
        res["condition"] = "median(fused) %.4f <= median(unfused) %.4f + spread %.4f: %s" % (
            res["fused"]["median_ms"], res["unfused"]["median_ms"], margin,
            res["fused"]["median_ms"] <= res["unfused"]["median_ms"] + margin)
    if "fused" in times and "resident" in times:
        margin = res["fused"]["p90_ms"] - res["fused"]["p10_ms"]
        res["condition_resident"] = "median(resident) %.4f <= median(fused) %.4f + spread %.4f: %s" % (
            res["resident"]["median_ms"], res["fused"]["median_ms"], margin,
            res["resident"]["median_ms"] <= res["fused"]["median_ms"] + margin)
    m = sum(SIZES)
    res["resident_kernel_bytes"] = {"streamed": 16 * m, "prob_once": 4 * B * C * N, "sampled_records": 16 * B * N,
                                    "note": "12 B vertex + 4 B label per vertex; the soft-max table once per slot; the grid's "
                                            "(x, y, z, index) records of the sampled points, L2-resident"}
    res["fused_kernel_bytes"] = {"streamed": 32 * m, "prob_once": 4 * B * C * N,
                                 "note": "idx 12 + dist2 12 + label 8 B per vertex; the soft-max table once per scan"}
    print(json.dumps(res, indent=1))


def end_to_end(count):
    """One evaluation pass over `count` synthetic scans, batch_size_val = 2, N = 8000 sampled points (the small configured
    model of tests/test_seg_metrics_gpu.py), both ways; wall time, device-synchronised, after one warm pass each."""
    import logging
    from geot_amd.openpoints.dataset import DeviceScanSet, draw_val_sel
    from geot_amd.openpoints.models.segmentation import WholePartSeg
    logging.disable(logging.INFO)
    dev = torch.device("cuda:0")
    n = 8000
    from test_seg_metrics_gpu import SMALL as small          # the small configured model of the validation tests
    torch.manual_seed(0)
    model = WholePartSeg(segmentor_args=dict(NAME="PointTransformer_seg_T", **small)).to(dev)
    cfg = type("Cfg", (), {"num_classes": C, "num_points": n, "epoch": 0, "epochs": 1})()
    center, scale = np.array([2.0, -15.5, 4.25], np.float32), np.float32(36.0)
    wholes = [(make_cloud(100003 - 619 * i, 600 + i)[0] * np.float32(1.01) * scale + center).astype(np.float32) for i in range(count)]
    labels = [region_labels((w - center) / scale).astype(np.int32) for w in wholes]
    jaws = [i % 2 for i in range(count)]

    def host_batches():
        """What the reference's workers and collate_fn_val hand over (tooth_dataset.py:116-188), made on the host."""
        out = []
        for at in range(0, count, 2):
            items = []
            for i in range(at, min(at + 2, count)):
                c0 = wholes[i].mean(0)
                m0 = np.sqrt(((wholes[i] - c0) ** 2).sum(1)).max()
                sel = draw_val_sel([len(wholes[i])], n)[0]
                pos = ((wholes[i] - c0) / m0)[sel].astype(np.float32)
                c1 = pos.mean(0, keepdims=True)
                cen = pos - c1
                items.append((cen / np.sqrt((cen ** 2).sum(1)).max(), pos, c0.astype(np.float32), np.float32(m0)))
            ids = list(range(at, at + len(items)))
            out.append({"pos": torch.from_numpy(np.stack([it[0] for it in items]).astype(np.float32)),
                        "x": torch.from_numpy(np.stack([it[1] for it in items])), "y": torch.zeros(len(items), n, dtype=torch.long),
                        "cls": torch.tensor([[jaws[i]] for i in ids]), "points": [torch.from_numpy(wholes[i]) for i in ids],
                        "labels": [torch.from_numpy(labels[i]).long() for i in ids],
                        "center": [torch.from_numpy(it[2]) for it in items], "scale": [torch.tensor(it[3]) for it in items]})
        return out

    scans = DeviceScanSet(wholes, labels, cls=jaws, device=dev)
    res = {"scans": count, "N": n, "batch_size": 2, "vertices": int(sum(len(w) for w in wholes)),
           "note": "end-to-end wall time of one evaluation pass, model forward included; host batches are made before the clock "
                   "starts (the reference's workers overlap with it), so the host leg pays the uploads only"}

    def timed(name, run):
        np.random.seed(1)
        run()                                                        # warm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run()
        torch.cuda.synchronize()
        res[name] = {"pass_ms": round((time.perf_counter() - t0) * 1e3, 2), "whole_miou": float(out[1])}

    with torch.no_grad(), quiet():
        made = [host_batches(), host_batches()]                      # validate() moves a batch's tensors: one list per pass
        timed("validate_host_batches", lambda: validate(model, made.pop(), cfg))
        timed("validate_scans", lambda: validate_scans(model, scans, cfg))
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
