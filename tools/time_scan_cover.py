"""Device time of one geot_scan_cover call against one geot_scan_vote call, and of cover_scans against vote_scans.

    python tools/time_scan_cover.py [--reps 40] [--warmup 5] [--e2e-reps 5] [--out profiles/scan_cover_timing.txt]

B = 2 scans of ~1e5 vertices, C = 17, n = 16 000 and 24 000 samples per scan, ONE process.  Kernel legs, alternating after
warm-up, device events around each C-ABI call:

    vote add a / b      a middle vote of geot_scan_vote (the grid build over the samples, the search, the interpolation, one
                        read and one write of the accumulator) -- csrc/scan_predict.hip's kernel is the parent commit's, so this
                        is the parent's call; timed TWICE (a, b): their difference is the spread of this method
    cover add a / b     a middle pass of geot_scan_cover (pass 1 of round 1: every sample owns a vertex), timed twice too
    cover set           pass 0 of round 0: rows stored, not read
    cover finish        the last pass with GEOT_VOTE_FINISH and counts: the scatter plus the arg-max launch over every vertex
    vote finish         the last vote with GEOT_VOTE_FINISH and counts

The one claim checked: cover add is below vote add by more than the spread of the two vote timings (it does no search).
Then, with the configured model (TOOTH_SEG_CFG) on the same scans, device time between events of cover_scans(rounds=1) -- P =
ceil(M / n) passes -- against vote_scans(num_votes=P), per pass and per scan, and the C-ABI calls each makes (counted through
ext._common.trace).  The text goes to --out as well as to stdout."""
import argparse
import collections
import json
import logging
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geot_amd import _lib  # noqa: E402
from geot_amd.ext import _common  # noqa: E402
from geot_amd.ext._common import call, ptr  # noqa: E402
from geot_amd.synth import make_cloud, make_logits, region_labels  # noqa: E402
from geot_amd.validation import cover_scans, scan_work_table, vote_scans  # noqa: E402

B, C, SIZES = 2, 17, (100003, 98765)
CENTER, SCALE = np.array([2.0, -15.5, 4.25], np.float32), np.float32(36.0)
# kernel launches per C-ABI call at these shapes, from the entry points' contracts (include/geot_hip.h)
LAUNCHES = {"geot_scan_vote": 6, "geot_scan_cover": 1, "geot_scan_cover finish": 2}


def make_scans(dev):
    from geot_amd.openpoints.dataset import DeviceScanSet
    wholes = [(make_cloud(m, 410 + i)[0] * np.float32(1.01) * SCALE + CENTER).astype(np.float32) for i, m in enumerate(SIZES)]
    labels = [(region_labels((w - CENTER) / SCALE) % C).astype(np.int32) for w in wholes]
    return DeviceScanSet(wholes, labels, cls=[0, 1], device=dev)


def kernel_legs(scans, n, reps, warmup):
    from geot_amd.openpoints.dataset import sample_draw_cover
    dev = scans.device
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
    passes = max(-(-m // n) for m in SIZES)
    sels = [sample_draw_cover(scans, ids, n, 5, 0, p)[0] for p in (0, 1, passes - 1)]
    vote_head = (dev, B, C, n, len(scans), int(scans.points.shape[0]), ptr(scans.points), ptr(scans.labels), ptr(scans.offsets),
                 ptr(ids), ptr(known), ptr(prob), int(work.shape[0]), ptr(work), ptr(offs), ptr(acc))
    cover_head = (dev, B, C, n, len(scans), int(scans.points.shape[0]), ptr(scans.labels), ptr(scans.offsets), ptr(ids))
    cover_tail = (int(work.shape[0]), ptr(work), ptr(offs), ptr(acc))

    def vote(mode):
        return lambda: call("geot_scan_vote", *vote_head, mode, None, ptr(counts) if mode & _lib.VOTE_FINISH else None, ptr(ws), nbytes)

    def cover(sel, p, mode):
        return lambda: call("geot_scan_cover", *cover_head, ptr(sel), ptr(prob), p, *cover_tail, mode, None,
                            ptr(counts) if mode & _lib.VOTE_FINISH else None)
    legs = collections.OrderedDict([
        ("vote add a", vote(0)), ("cover add a", cover(sels[1], 1, 0)), ("cover set", cover(sels[0], 0, _lib.VOTE_SET)),
        ("cover finish", cover(sels[2], passes - 1, _lib.VOTE_FINISH)), ("vote finish", vote(_lib.VOTE_FINISH)),
        ("cover add b", cover(sels[1], 1, 0)), ("vote add b", vote(0))])
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
    res = {"passes": passes}
    for k, ts in times.items():
        p10, med, p90 = np.percentile(ts, [10, 50, 90])
        res[k] = {"median_ms": round(float(med), 4), "p10_ms": round(float(p10), 4), "p90_ms": round(float(p90), 4)}
    va, vb, ca, cb = (res[k]["median_ms"] for k in ("vote add a", "vote add b", "cover add a", "cover add b"))
    res["vote_spread_ms"] = round(abs(va - vb), 4)
    res["cover_spread_ms"] = round(abs(ca - cb), 4)
    res["vote_minus_cover_ms"] = round(min(va, vb) - max(ca, cb), 4)
    res["cover_below_vote_by_more_than_the_spread"] = bool(min(va, vb) - max(ca, cb) > abs(va - vb))
    res["kernel_launches"] = {"vote": LAUNCHES["geot_scan_vote"], "cover": LAUNCHES["geot_scan_cover"],
                              "cover with finish": LAUNCHES["geot_scan_cover finish"]}
    return res


def end_to_end(scans, model, n, reps):
    from geot_amd.openpoints.dataset import DeviceDraws, VoteBatcher
    passes = max(-(-m // n) for m in SIZES)
    batcher = VoteBatcher(scans, n, C, draws=DeviceDraws(9))
    runs = {"cover_scans": lambda: cover_scans(model, batcher, [0, 1]),
            "vote_scans": lambda: vote_scans(model, batcher, [0, 1], passes)}
    res = {"passes": passes}
    calls = {}
    for name, run in runs.items():                 # warm, and the C-ABI calls of one run
        run()
        seen = collections.Counter()

        def spy(launch, entry, seen=seen):
            seen[entry] += 1
            return launch()
        _common.trace = spy
        try:
            run()
        finally:
            _common.trace = None
        calls[name] = seen
    times = {k: [] for k in runs}
    names = list(runs)
    for i in range(reps):
        for k in (names if i % 2 == 0 else names[::-1]):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            runs[k]()
            stop.record()
            stop.synchronize()
            times[k].append(start.elapsed_time(stop))
    for k, ts in times.items():
        med = float(np.median(ts))
        scan_entry = "geot_scan_cover" if k == "cover_scans" else "geot_scan_vote"
        res[k] = {"ms": round(med, 3), "ms_min": round(float(min(ts)), 3), "ms_max": round(float(max(ts)), 3),
                  "ms_per_pass": round(med / passes, 3), "ms_per_scan": round(med / B, 3), "c_abi_calls": int(sum(calls[k].values())),
                  "scan_calls": int(calls[k][scan_entry]), "draw_calls": int(calls[k]["geot_sample_draw"] + calls[k]["geot_sample_draw_cover"])}
    res["cover_vs_vote"] = round(res["cover_scans"]["ms"] / res["vote_scans"]["ms"] - 1.0, 4)
    return res


def report(res):
    lines = [__doc__.split("\n\n")[0].strip(), "", "device %s, %d repetitions after %d warm-up rounds per kernel leg, %d per end-to-end leg; B = %d "
             "scans of %s vertices, C = %d" % (res["device"], res["reps"], res["warmup"], res["e2e_reps"], B, list(SIZES), C), "",
             "median ms between device events around one C-ABI call",
             "%-10s%-14s%-14s%-14s%-14s%-12s%-14s%-12s" % ("n", "vote add a", "vote add b", "cover add a", "cover add b", "cover set",
                                                            "cover finish", "vote finish")]
    verdicts = []
    for key, leg in res.items():
        if key.startswith("n="):
            lines.append("%-10s" % key + "".join("%-*.4f" % (w, leg[k]["median_ms"]) for k, w in (
                ("vote add a", 14), ("vote add b", 14), ("cover add a", 14), ("cover add b", 14), ("cover set", 12), ("cover finish", 14),
                ("vote finish", 12))))
            verdicts.append("%s: the covering call is %.4f ms below the voted call; the voted call's two timings differ by %.4f ms: %s.  "
                            "Kernel launches per call: vote %d, cover %d (%d with the finish)." %
                            (key, leg["vote_minus_cover_ms"], leg["vote_spread_ms"],
                             "BELOW by more than the spread, as expected" if leg["cover_below_vote_by_more_than_the_spread"]
                             else "NOT below by more than the spread", leg["kernel_launches"]["vote"], leg["kernel_launches"]["cover"],
                             leg["kernel_launches"]["cover with finish"]))
    lines += [""] + verdicts + ["", "cover_scans(rounds=1) against vote_scans(num_votes=P), the configured model's forward passes inside "
                                "(median ms between device events)"]
    for key, leg in res.items():
        if key.startswith("N="):
            c, v = leg["cover_scans"], leg["vote_scans"]
            lines.append("%s P=%d: cover_scans %.3f ms (%.3f per pass, %.3f per scan; %d C-ABI calls, %d of them geot_scan_cover), vote_scans "
                         "%.3f ms (%.3f per pass, %.3f per scan; %d C-ABI calls, %d of them geot_scan_vote): %+.1f %%" %
                         (key, leg["passes"], c["ms"], c["ms_per_pass"], c["ms_per_scan"], c["c_abi_calls"], c["scan_calls"], v["ms"],
                          v["ms_per_pass"], v["ms_per_scan"], v["c_abi_calls"], v["scan_calls"], 100 * leg["cover_vs_vote"]))
    return "\n".join(lines) + "\n\n" + json.dumps(res, indent=1) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--e2e-reps", type=int, default=5, help="repetitions of the end-to-end legs (0: skip them)")
    ap.add_argument("--n", type=int, nargs="+", default=[16000, 24000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_cover_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_scan_cover: needs a GPU (a timing taken anywhere else says nothing)")
    logging.disable(logging.INFO)
    dev = torch.device("cuda:0")
    scans = make_scans(dev)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "e2e_reps": args.e2e_reps}
    for n in args.n:
        res["n=%d" % n] = kernel_legs(scans, n, args.reps, args.warmup)
        print("n=%d" % n, json.dumps(res["n=%d" % n]), flush=True)
    if args.e2e_reps > 0:
        from geot_amd.openpoints.models.backbone.transformer import TOOTH_SEG_CFG
        from geot_amd.openpoints.models.segmentation import WholePartSeg
        torch.manual_seed(0)
        model = WholePartSeg(segmentor_args=dict(NAME="PointTransformer_seg_T", **TOOTH_SEG_CFG)).to(dev).eval()
        with torch.no_grad():
            for n in args.n:
                res["N=%d" % n] = end_to_end(scans, model, n, args.e2e_reps)
                print("N=%d" % n, json.dumps(res["N=%d" % n]), flush=True)
    text = report(res)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
