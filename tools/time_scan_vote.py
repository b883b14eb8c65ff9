"""Device time of one vote of geot_scan_vote against geot_scan_predict, and of a whole voted validation pass.

    python tools/time_scan_vote.py [--reps 40] [--warmup 5] [--scans 4] [--out profiles/scan_vote_timing.txt]

At B = 2 scans of ~1e5 vertices, C = 17, n = 16 000 and 24 000 sampled points, in ONE process, the legs alternating after
warm-up, each repetition timed with device events around the C-ABI call (the grid build over the sampled points, five small
launches, is part of both entry points):

    predict        geot_scan_predict writing the counts -- the parent kernel, the yardstick
    vote set       the first vote (GEOT_VOTE_SET): the accumulator is written, not read
    vote add       a middle vote: one read and one write of the accumulator (2 x M C 4 bytes on top of predict's traffic)
    vote finish    the last vote (GEOT_VOTE_FINISH): the add, the arg-max of the sums and the counts

each vote leg in both forms of the accumulator access, GEOT_VOTE_IMPL=row and =tile (csrc/scan_predict.hip).  The
expectation: a middle vote within 1.25 x predict (27 MB more traffic at this shape).  Then, wall time with a device synchronise (model forward included, the small
configured model of the validation tests, N = 8000): validate_scans against validate_scans_voted at V = 1, 4, 10 over `--scans`
synthetic scans.  The text goes to --out as well as to stdout."""
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
from geot_amd import _lib  # noqa: E402
from geot_amd.ext._common import call, ptr  # noqa: E402
from geot_amd.synth import make_cloud, make_logits, region_labels  # noqa: E402
from geot_amd.validation import scan_work_table, validate_scans, validate_scans_voted  # noqa: E402
from _seg_metrics_ref import quiet  # noqa: E402

B, C, SIZES = 2, 17, (100003, 98765)
CENTER, SCALE = np.array([2.0, -15.5, 4.25], np.float32), np.float32(36.0)


def kernel_legs(n, reps, warmup):
    from geot_amd.openpoints.dataset import DeviceScanSet
    dev = torch.device("cuda:0")
    wholes = [(make_cloud(m, 410 + i)[0] * np.float32(1.01) * SCALE + CENTER).astype(np.float32) for i, m in enumerate(SIZES)]
    labels = [region_labels((w - CENTER) / SCALE).astype(np.int32) for w in wholes]
    scans = DeviceScanSet(wholes, labels, cls=[0, 1], device=dev)
    unit = np.stack([make_cloud(n, 400 + s)[0] for s in range(B)])
    known = torch.from_numpy((unit * SCALE + CENTER).astype(np.float32)).to(dev)
    prob = torch.softmax(torch.from_numpy(make_logits(unit, 400)).to(dev), dim=1).contiguous()
    total = sum(SIZES)
    work = torch.from_numpy(scan_work_table(SIZES)).to(dev)
    offs = torch.tensor([0, SIZES[0]], dtype=torch.int64, device=dev)
    ids = torch.arange(B, dtype=torch.int64, device=dev)
    acc = torch.zeros((total, C), device=dev)
    counts = torch.zeros((B, C * (C + 1) + 1), dtype=torch.int64, device=dev)
    nbytes = int(_lib.load().geot_scan_predict_ws_bytes(B, n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    head = (dev, B, C, n, len(scans), int(scans.points.shape[0]), ptr(scans.points), ptr(scans.labels), ptr(scans.offsets), ptr(ids),
            ptr(known), ptr(prob), int(work.shape[0]), ptr(work), ptr(offs))

    def predict():
        call("geot_scan_predict", *head, None, ptr(counts), ptr(ws), nbytes)

    def vote(form, mode):
        def run():
            os.environ["GEOT_VOTE_IMPL"] = form                # the library reads it at every call
            call("geot_scan_vote", *head, ptr(acc), mode, None, ptr(counts) if mode & _lib.VOTE_FINISH else None, ptr(ws), nbytes)
        return run
    legs = {"predict": predict}
    for form in ("row", "tile"):
        legs["vote set " + form] = vote(form, _lib.VOTE_SET)
        legs["vote add " + form] = vote(form, 0)
        legs["vote finish " + form] = vote(form, _lib.VOTE_FINISH)
    names = list(legs)
    times = {k: [] for k in names}
    for i in range(warmup + reps):
        for k in (names if i % 2 == 0 else names[::-1]):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            legs[k]()
            stop.record()
            stop.synchronize()
            if i >= warmup:
                times[k].append(start.elapsed_time(stop))
    os.environ.pop("GEOT_VOTE_IMPL", None)
    res = {}
    for k, ts in times.items():
        p10, med, p90 = np.percentile(ts, [10, 50, 90])
        res[k] = {"median_ms": round(float(med), 4), "p10_ms": round(float(p10), 4), "p90_ms": round(float(p90), 4)}
    for form in ("row", "tile"):
        res["vote add %s / predict" % form] = round(res["vote add " + form]["median_ms"] / res["predict"]["median_ms"], 3)
    res["accumulator_bytes_per_add"] = 2 * total * C * 4
    return res


def end_to_end(count, votes=(1, 4, 10)):
    import logging
    from geot_amd.openpoints.dataset import DeviceScanSet
    from geot_amd.openpoints.models.segmentation import WholePartSeg
    from test_seg_metrics_gpu import SMALL as small          # the small configured model of the validation tests
    logging.disable(logging.INFO)
    dev = torch.device("cuda:0")
    n = 8000
    torch.manual_seed(0)
    model = WholePartSeg(segmentor_args=dict(NAME="PointTransformer_seg_T", **small)).to(dev)
    cfg = type("Cfg", (), {"num_classes": C, "num_points": n, "epoch": 0, "epochs": 1})()
    wholes = [(make_cloud(100003 - 619 * i, 600 + i)[0] * np.float32(1.01) * SCALE + CENTER).astype(np.float32) for i in range(count)]
    labels = [region_labels((w - CENTER) / SCALE).astype(np.int32) for w in wholes]
    scans = DeviceScanSet(wholes, labels, cls=[i % 2 for i in range(count)], device=dev)
    res = {"scans": count, "N": n, "batch_size": 2, "vertices": int(sum(len(w) for w in wholes)),
           "note": "wall time of one evaluation pass, device-synchronised, model forward included, after one warm pass each"}

    def timed(name, run):
        np.random.seed(1)
        torch.manual_seed(1)
        run()                                                        # warm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run()
        torch.cuda.synchronize()
        res[name] = {"pass_ms": round((time.perf_counter() - t0) * 1e3, 2), "whole_miou": float(out[1])}

    with torch.no_grad(), quiet():
        timed("validate_scans", lambda: validate_scans(model, scans, cfg))
        for v in votes:
            timed("validate_scans_voted V=%d" % v, lambda v=v: validate_scans_voted(model, scans, cfg, num_votes=v))
    return res


HEAD = """One vote of geot_scan_vote against geot_scan_predict (csrc/scan_predict.hip), and a whole voted validation pass
(tools/time_scan_vote.py; the legs are described there).  B = 2 scans of ~1e5 vertices, C = 17, one process, the legs
alternating after warm-up, device events around each C-ABI call; the end-to-end figures are device-synchronised wall time with
the model's forward pass inside.

The two forms of the accumulator access, as compiled for gfx950 (grid search; -Rpass-analysis=kernel-resource-usage):
  predict  91 SGPRs, 40 VGPRs, 16 912 B LDS per workgroup of 256 (the counts' histograms)
  row      106 SGPRs, 43 VGPRs, the same LDS: lanes < C read the vertex's 4 C-byte row in front of the ring walk, which hides the
           read, and write it after the interpolation -- partial-line stores, but one line per vertex either way
  tile     106 SGPRs, 48 VGPRs, + 4 x 64 x (C | 1) x 4 B of dynamic LDS (17 408 B at C = 17): 34 320 B per workgroup leave 4
           workgroups on a CU where the other forms have 8, and the ring walk is latency-bound on the waves in flight
Both give the same bits (tests/test_scan_vote_gpu.py runs every case in both).  The default is the form with the smaller
"vote add / predict" below; GEOT_VOTE_IMPL=row|tile picks one for a call.
"""


def report(res):
    """The text of profiles/scan_vote_timing.txt: the head, a verdict per n, the figures."""
    lines = [HEAD]
    for key, leg in res.items():
        if key.startswith("n="):
            row, tile = leg["vote add row / predict"], leg["vote add tile / predict"]
            lines.append("%s: a middle vote is %.3f x predict in the row form, %.3f x in the tile form (expected: within 1.25 x); "
                         "predict %.4f ms" % (key, row, tile, leg["predict"]["median_ms"]))
    return "\n".join(lines) + "\n\n" + json.dumps(res, indent=1) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scans", type=int, default=4, help="scans of the end-to-end pass (0: skip it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_vote_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_scan_vote: needs a GPU (a timing taken anywhere else says nothing)")
    res = {"device": torch.cuda.get_device_name(0), "B": B, "C": C, "M": list(SIZES), "reps": args.reps}
    for n in (16000, 24000):
        res["n=%d" % n] = kernel_legs(n, args.reps, args.warmup)
    if args.scans > 0:
        res["end_to_end"] = end_to_end(args.scans)
    text = report(res)
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
