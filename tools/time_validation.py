"""Validation scoring per batch at the reference's operating point: B = 2 scans (batch_size_val: 2), N = 16 000 sampled
points (the authors' cloud size), ~1e5 vertices per scan, C = 17; the model's forward is not part of it.

    python tools/time_validation.py [--reps 60] [--warmup 5] [--only unfused|fused]

(a) unfused: get_pred_whole, then get_seg_metrics' statements (restated in tests/_seg_metrics_ref.py: the .cpu() copies,
    torch.unique, two passes per class) -- what a batch cost before SegMetrics;
(b) fused:   SegMetrics.update_from_logits + read() (a read per batch: more than the per-batch share of the one read an
    epoch needs).
The two alternate, after warm-up; each repetition is device-synchronised wall time.  Condition: median(b) <= median(a) +
spread(a), spread = p90 - p10 of (a) in this run (both paths share the three_nn that dominates them).  Prints the bytes the
fused kernel streams, for a TB/s figure from its rocprofv3 --kernel-trace time."""
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
from geot_amd.validation import SegMetrics, get_pred_whole  # noqa: E402
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
    ap.add_argument("--only", choices=("unfused", "fused"), default=None)
    args = ap.parse_args()
    logits, pts, wholes, centers, scales, labels = batch()
    metrics = SegMetrics(C, logits.device)

    def unfused():
        preds = get_pred_whole(logits, pts, wholes, centers, scales)
        return get_seg_metrics_ref(preds, labels)

    def fused():
        metrics.reset()
        metrics.update_from_logits(logits, pts, wholes, centers, scales, labels, [0, 1])
        return metrics.read()

    paths = {"unfused": unfused, "fused": fused}
    names = [args.only] if args.only else list(paths)
    times = {k: [] for k in names}
    with torch.no_grad(), quiet():
        a, b = unfused(), fused()          # the same numbers both ways
        same = all(float(x) == float(y) for x, y in zip(a[1] + a[2], b["miou_list"] + b["mdsc_list"]))
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
    if len(times) == 2:
        margin = res["unfused"]["p90_ms"] - res["unfused"]["p10_ms"]
        res["condition"] = "median(fused) %.4f <= median(unfused) %.4f + spread %.4f: %s" % (
            res["fused"]["median_ms"], res["unfused"]["median_ms"], margin,
            res["fused"]["median_ms"] <= res["unfused"]["median_ms"] + margin)
    m = sum(SIZES)
    res["fused_kernel_bytes"] = {"streamed": 32 * m, "prob_once": 4 * B * C * N,
                                 "note": "idx 12 + dist2 12 + label 8 B per vertex; the soft-max table once per scan"}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
