"""Passes per second and host time per pass of the whole-scan validation loop under the graph= / lookahead= switches of
geot_amd/validation.py, against the defaults and against the parent commit's loop.

    git show <parent>:geot_amd/validation.py > /tmp/parent_validation.py
    python tools/time_val_replay.py --parent-validation /tmp/parent_validation.py --parent-hash <parent> \
        [--reps 11] [--warmup 3] [--out profiles/val_replay_timing.txt]

The configured model (TOOTH_SEG_CFG inside WholePartSeg, eval mode, no_grad) on synthetic scans of ~1e5 vertices, 17 classes;
N = 16 000 and 24 000 sampled points, batch_size B = 1 and 2, num_votes V = 0 (ValBatcher, geot_scan_predict per pass) and 10
(VoteBatcher, geot_scan_vote per pass); the batcher has a side stream, as a user who wants the overlap gives it one.  A run
is validation's own loop -- _passes and the per-pass scoring of _validate, without the final read() -- over 16 groups (V = 0)
or 4 groups (V = 10) of B scans: 16 / 40 passes.  Modes, all in ONE process, one run each per repetition in alternating order
after `--warmup` runs each (the warm-up holds every capture):

    parent a / b   the parent commit's _passes (its validation.py loaded beside this one), timed twice per repetition:
                   the difference between the two medians is the run-to-run spread every other comparison is read against
                   (eager is "within" when it lies in the band the two span, widened by that difference on either side)
    eager          this commit, the defaults (graph=False, lookahead=0)
    lookahead      lookahead=True alone: G = max(V, 1) passes drawn ahead, one geometry call for them, eager launches
    graph          graph=True alone: G = 1, the geometry and the forward pass replayed from hipGraphs
    both           graph=True, lookahead=True

passes/s: passes over the time between two device events around the run; host ms/pass: the host clock over the loop (it
ends before the device does) over the passes.  Before the timing every mode's SegMetrics counts are compared with the eager
mode's on the same seeded draws: they must be equal.  The text goes to --out as well as to stdout."""
import argparse
import importlib.util
import json
import logging
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geot_amd import validation as V  # noqa: E402
from geot_amd.synth import make_cloud, region_labels  # noqa: E402

C = 17
CENTER, SCALE = np.array([2.0, -15.5, 4.25], np.float32), np.float32(36.0)
MODES = ("parent a", "eager", "lookahead", "graph", "both", "parent b")
SWITCHES = {"eager": (False, 0), "lookahead": (False, True), "graph": (True, 0), "both": (True, True)}


def load_parent(path):
    """The parent commit's validation.py as a module of this package (its relative imports resolve here: nothing else changed)."""
    spec = importlib.util.spec_from_file_location("geot_amd._parent_validation", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def drive(mod, model, batcher, groups, votes, extra):
    """validation._validate's loop without the final read(): every pass scored as the validators score it."""
    metrics = mod.SegMetrics(C, batcher.device)
    ballots = None
    for data, logits, first, last in mod._passes(model, batcher, groups, max(votes, 1), None, *extra):
        if votes and first:
            ballots = mod.ScanVotes(data, C)
        if not last:
            ballots.add(logits, data)
        elif votes:
            metrics.update_from_votes(ballots, logits, data)
        else:
            metrics.update_from_scans(logits, data)
    return metrics


def shape_legs(model, scans, parent, n, b, votes, reps, warmup):
    from geot_amd.openpoints.dataset import ValBatcher, VoteBatcher
    count = (4 if votes else 16) * b
    groups = [list(range(at, at + b)) for at in range(0, count, b)]
    passes = len(groups) * max(votes, 1)
    stream = torch.cuda.Stream()
    batcher = VoteBatcher(scans, n, C, stream=stream) if votes else ValBatcher(scans, n, C, stream=stream)

    def run(mode, seed):
        np.random.seed(seed)            # every host generator a batcher draws from
        random.seed(seed)
        torch.manual_seed(seed)
        if mode.startswith("parent"):
            return drive(parent, model, batcher, groups, votes, ())
        g, graphed = V._replay_switches(*SWITCHES[mode], votes, model, "time_val_replay")
        return drive(V, model, batcher, groups, votes, (g, graphed))
    # the same counts in every mode, on the same seeded draws (the last of these runs are warm-up too)
    for _ in range(warmup):
        want = run("eager", 7).counts.clone()
        for mode in MODES:
            got = run(mode, 7).counts
            if not torch.equal(got, want):
                raise SystemExit("time_val_replay: N=%d B=%d V=%d: the counts of mode %r differ from the eager mode's" % (n, b, votes, mode))
    times = {m: {"device_ms": [], "host_ms": []} for m in MODES}
    for rep in range(reps):
        for mode in (MODES if rep % 2 == 0 else MODES[::-1]):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            t0 = time.perf_counter()
            run(mode, 100 + rep)
            host = time.perf_counter() - t0
            stop.record()
            stop.synchronize()
            times[mode]["device_ms"].append(start.elapsed_time(stop))
            times[mode]["host_ms"].append(host * 1e3)
    res = {"passes": passes, "scans": count}
    for mode, t in times.items():
        dev = np.asarray(t["device_ms"])
        res[mode] = {"passes_per_s": round(float(passes / np.median(dev) * 1e3), 2), "ms_per_pass": round(float(np.median(dev) / passes), 3),
                     "ms_per_pass_min": round(float(dev.min() / passes), 3), "ms_per_pass_max": round(float(dev.max() / passes), 3),
                     "host_ms_per_pass": round(float(np.median(t["host_ms"]) / passes), 3)}
    a, bb, e = (res[m]["ms_per_pass"] for m in ("parent a", "parent b", "eager"))
    res["spread"] = round(abs(a - bb) / min(a, bb), 4)
    res["eager_vs_parent"] = round(e / (0.5 * (a + bb)) - 1.0, 4)
    res["eager_within_spread"] = bool(min(a, bb) * (1.0 - res["spread"]) <= e <= max(a, bb) * (1.0 + res["spread"]))
    for mode in ("lookahead", "graph", "both"):
        res[mode + "_vs_eager"] = round(res[mode]["ms_per_pass"] / e - 1.0, 4)
    return res


def report(res):
    lines = [__doc__.split("\n\n")[0].strip(), "", "device %s, parent commit %s, %d repetitions after %d warm-up runs per mode" %
             (res["device"], res["parent"], res["reps"], res["warmup"]), "",
             "ms per pass between device events (median; passes/s = 1000 / it) | host ms per pass",
             "%-22s" % "shape" + "".join("%-19s" % m for m in MODES)]
    verdicts = []
    for key, leg in res.items():
        if not key.startswith("N="):
            continue
        lines.append("%-22s" % key + "".join("%-19s" % ("%7.3f | %6.3f" % (leg[m]["ms_per_pass"], leg[m]["host_ms_per_pass"])) for m in MODES))
        spread = leg["spread"]
        verdicts.append("%s: spread (parent a vs b) %.1f %%; eager vs the parents' mean %+.1f %% (%s); lookahead %+.1f %%, graph %+.1f %%, both %+.1f %% "
                        "vs eager (both: %s)" % (key, 100 * spread, 100 * leg["eager_vs_parent"],
                                                 "within" if leg["eager_within_spread"] else "OUTSIDE the spread",
                                                 100 * leg["lookahead_vs_eager"], 100 * leg["graph_vs_eager"], 100 * leg["both_vs_eager"],
                                                 "not slower than the spread allows" if leg["both_vs_eager"] <= spread else "SLOWER"))
    legs = [leg for key, leg in res.items() if key.startswith("N=")]
    verdicts += ["", "all shapes: the parent's two timings differ by %.1f .. %.1f %% (the run-to-run spread of this method, %d pairs); eager vs the "
                 "parents' mean %+.1f .. %+.1f %%; both vs eager %+.1f .. %+.1f %%" %
                 (100 * min(g["spread"] for g in legs), 100 * max(g["spread"] for g in legs), len(legs),
                  100 * min(g["eager_vs_parent"] for g in legs), 100 * max(g["eager_vs_parent"] for g in legs),
                  100 * min(g["both_vs_eager"] for g in legs), 100 * max(g["both_vs_eager"] for g in legs))]
    return "\n".join(lines + [""] + verdicts) + "\n\n" + json.dumps(res, indent=1) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-validation", required=True, help="the parent commit's geot_amd/validation.py")
    ap.add_argument("--parent-hash", default="unknown")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, nargs="+", default=[16000, 24000])
    ap.add_argument("--b", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--votes", type=int, nargs="+", default=[0, 10])
    ap.add_argument("--vertices", type=int, default=100003)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "val_replay_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_val_replay: needs a GPU (a timing taken anywhere else says nothing)")
    from geot_amd.openpoints.dataset import DeviceScanSet
    from geot_amd.openpoints.models.backbone.transformer import TOOTH_SEG_CFG
    from geot_amd.openpoints.models.segmentation import WholePartSeg
    logging.disable(logging.INFO)
    dev = torch.device("cuda:0")
    parent = load_parent(args.parent_validation)
    torch.manual_seed(0)
    model = WholePartSeg(segmentor_args=dict(NAME="PointTransformer_seg_T", **TOOTH_SEG_CFG)).to(dev).eval()
    count = 16 * max(args.b)
    wholes = [(make_cloud(args.vertices - 619 * i, 600 + i)[0] * np.float32(1.01) * SCALE + CENTER).astype(np.float32) for i in range(count)]
    labels = [(region_labels((w - CENTER) / SCALE) % C).astype(np.int32) for w in wholes]
    scans = DeviceScanSet(wholes, labels, cls=[i % 2 for i in range(count)], device=dev)
    res = {"device": torch.cuda.get_device_name(0), "parent": args.parent_hash, "reps": args.reps, "warmup": args.warmup,
           "vertices_per_scan": "%d..%d" % (len(wholes[-1]), len(wholes[0]))}
    with torch.no_grad():
        for n in args.n:
            for b in args.b:
                for votes in args.votes:
                    key = "N=%d B=%d V=%d" % (n, b, votes)
                    res[key] = shape_legs(model, scans, parent, n, b, votes, args.reps, args.warmup)
                    print(key, json.dumps(res[key]), flush=True)
    text = report(res)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
