"""Timing of the connected-pieces clean-up (geot_scan_islands, validation.scan_neighbours / clean_scans, islands= on the
validators); profiles/scan_islands_timing.txt holds one run's output.  Device events around windows of calls, the legs alternated
in one process, every leg timed in two series so that the spread shows, every shape warmed first.

  kernel   B = 2 synthetic scans of about 1e5 vertices in a spatially coherent vertex order, C = 17, labels 95 % right plus
           clusters of wrong labels: scan_neighbours alone (k = 8: two geot_knn_sorted_ws calls); geot_scan_islands alone on a
           fresh copy of the labels (the copy is timed on its own) in both GEOT_SCAN_ISLANDS_IMPL forms, and its
           components-only form (four of the six launches); clean_scans end to end; one geot_scan_refine call (n = 10) on the
           same labels for scale.  The two forms are compared bit for bit before anything is timed.
  paths    validate_scans and validate_scans_decoded on the small segmentor over four such scans, with islands off and on, each
           leg timed --repeats times, alternating.  --package-root times the off path of another checkout (the parent
           commit's) with the same script, for the comparison the file states.

    python tools/time_scan_islands.py [--legs kernel,paths] [--package-root DIR] [--vertices 100000]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_tooth_scores import SMALL, C, coherent_scan, summary, window      # noqa: E402


def noisy_labels(points, labels, seed):
    """A prediction 95 % right with stray vertices, plus clusters of 2 .. 40 nearby vertices of one wrong class."""
    rng = np.random.default_rng(seed)
    pred = labels.astype(np.int64).copy()
    flip = rng.random(len(pred)) < 0.05
    pred[flip] = rng.integers(0, C, size=int(flip.sum()))
    for _ in range(len(pred) // 500):
        at = int(rng.integers(len(pred)))
        lo, hi = max(0, at - 2000), min(len(pred), at + 2000)         # the order is coherent: look nearby only
        near = lo + np.argsort(((points[lo:hi] - points[at]) ** 2).sum(1), kind="stable")[:int(rng.integers(2, 41))]
        pred[near] = int(rng.integers(C))
    return pred


def kernel_legs(args):
    import torch
    from geot_amd import validation as V
    from geot_amd.ext import _common
    from geot_amd.openpoints.dataset import DeviceScanSet
    dev = torch.device("cuda:0")
    sizes = [args.vertices, args.vertices - 3217]
    scans = [coherent_scan(m, 900 + i) for i, m in enumerate(sizes)]
    dset = DeviceScanSet([p for p, _ in scans], [l for _, l in scans], cls=[0, 1], device=dev)
    batch = {"scans": dset, "sizes": list(sizes), "scan_ids": torch.arange(2, device=dev), "mandible": [True, False],
             "points": list(torch.split(dset.points, sizes))}
    noisy = torch.from_numpy(np.concatenate([noisy_labels(p, l, 40 + i) for i, (p, l) in enumerate(scans)])).to(dev)
    work = noisy.clone()
    views = [p.view(1, -1) for p in torch.split(work, sizes)]
    table = V.scan_neighbours(batch, 8)

    def fresh():
        work.copy_(noisy)

    def islands(**kw):
        def go():
            fresh()
            V.clean_scans(views, batch, nbr=table, num_classes=C, **kw)
        return go

    def components():
        V.scan_components(views, batch, nbr=table, num_classes=C)

    def clean():
        fresh()
        V.clean_scans(views, batch, num_classes=C)

    def refine():
        fresh()
        V.refine_scans(views, batch, 10, num_classes=C)

    legs = {"copy of the labels (in every leg below but two)": (None, fresh),
            "scan_neighbours, k = 8 (no copy)": (None, lambda: V.scan_neighbours(batch, 8)),
            "geot_scan_islands, combined, table given": ("combined", islands()),
            "geot_scan_islands, basic, table given": ("basic", islands()),
            "geot_scan_islands, components only (no copy)": ("combined", components),
            "clean_scans end to end (search + islands)": ("combined", clean),
            "geot_scan_refine, n = 10, the same labels": (None, refine)}

    def run(name):
        impl, fn = legs[name][:2]
        if impl == "basic":
            os.environ["GEOT_SCAN_ISLANDS_IMPL"] = "basic"
        else:
            os.environ.pop("GEOT_SCAN_ISLANDS_IMPL", None)
        return fn
    # the same bits from both forms, before anything is timed
    outs = {}
    for name in ("geot_scan_islands, combined, table given", "geot_scan_islands, basic, table given"):
        run(name)()
        outs[name] = work.clone()
    a, b = outs.values()
    assert torch.equal(a, b)
    fresh()
    _, stats = V.clean_scans(views, batch, nbr=table, num_classes=C, stats=True)
    print("kernel: B = 2 scans of %d and %d vertices, C = %d, table (sum M, 9); both forms relabel the same %d vertices; stats "
          "(components, islands, changed, stranded) %s" % (sizes[0], sizes[1], C, int((a != noisy).sum()), stats.cpu().tolist()))
    for name in legs:
        fn = run(name)
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - before
        seen = []
        _common.trace = lambda launch, entry: (seen.append(entry), launch())[1]
        try:
            fn()
        finally:
            _common.trace = None
        torch.cuda.synchronize()
        legs[name] = legs[name] + ("calls %s; peak memory above the inputs %.2f MB" % (", ".join(seen) or "none", peak / 1e6),)
    times = {name: ([], []) for name in legs}
    for name in legs:
        window(run(name), 5)                                         # warm
    for series in (0, 1):                                            # every leg twice: the spread between series shows
        for _ in range(args.rounds):
            for name in legs:                                        # alternating
                times[name][series].append(window(run(name), args.calls))
    os.environ.pop("GEOT_SCAN_ISLANDS_IMPL", None)
    for name in legs:
        print("  %-50s series 1 %s; series 2 %s; %s" % (name, summary(times[name][0]), summary(times[name][1]), legs[name][2]))


def path_legs(args):
    import logging
    import torch
    from geot_amd import validation as V
    from geot_amd.ext import _common
    from geot_amd.openpoints.dataset import DeviceScanSet, ValBatcher
    from geot_amd.openpoints.dataset.sample_draw import DeviceDraws
    from geot_amd.openpoints.models.segmentation import WholePartSeg
    logging.disable(logging.CRITICAL)
    dev = torch.device("cuda:0")
    sizes = [args.vertices, args.vertices - 3217, args.vertices + 1741, args.vertices - 12345]
    scans = [coherent_scan(m, 900 + i) for i, m in enumerate(sizes)]
    dset = DeviceScanSet([p for p, _ in scans], [l for _, l in scans], cls=[0, 1, 0, 1], device=dev)
    torch.manual_seed(5)
    model = WholePartSeg(segmentor_args=dict(NAME="PointTransformer_seg_T", **SMALL)).to(dev).eval()
    cfg = {"num_classes": C, "num_points": 4096, "epoch": 1, "epochs": 1}
    has_islands = hasattr(V, "clean_scans")
    print("paths: %d scans of %s vertices, batches of 2, 4096 samples, the small segmentor; package %s (%s)" %
          (len(sizes), sizes, os.path.dirname(V.__file__), "with islands=" if has_islands else "before the feature"))

    def leg(fn, on):
        def go():
            return fn(model, ValBatcher(dset, 4096, draws=DeviceDraws(5)), cfg, **({"islands": True} if on else {}))
        return go
    legs = {}
    for label, fn in (("validate_scans", V.validate_scans), ("validate_scans_decoded", V.validate_scans_decoded)):
        legs[label + " islands off"] = leg(fn, False)
        if has_islands:
            legs[label + " islands=True"] = leg(fn, True)
    results, times, calls = {}, {name: [] for name in legs}, {}
    for name, go in legs.items():
        results[name] = go()                                         # warm
        seen = []
        _common.trace = lambda launch, entry: (seen.append(entry), launch())[1]
        try:
            go()
        finally:
            _common.trace = None
        own = [s for s in seen if s.startswith(("geot_scan", "geot_seg_confusion", "geot_knn_sorted_ws", "geot_tooth"))]
        calls[name] = ", ".join("%s x %d" % (s, own.count(s)) for s in dict.fromkeys(own))
    for _ in range(args.repeats):
        for name, go in legs.items():                                # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            go()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    batches = len(sizes) // 2
    for name in legs:
        print("  %-40s %s ms per call (host clock, ends in a synchronise), %d batches; (macc, miou, mdsc) = %s" %
              (name, ", ".join("%.3f" % v for v in times[name]), batches, tuple(float(v) for v in results[name])))
        print("      whole-scan calls of one validation (the model's own searches among the geot_knn_sorted_ws): %s" % calls[name])
    if has_islands:
        for label in ("validate_scans", "validate_scans_decoded"):
            off, on = times[label + " islands off"], times[label + " islands=True"]
            print("  %s: islands=True adds %.3f ms per batch (medians %.3f -> %.3f ms per call)" %
                  (label, (np.median(on) - np.median(off)) / batches, np.median(off), np.median(on)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="kernel,paths")
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose geot_amd is timed (default: this one)")
    ap.add_argument("--vertices", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=6)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    assert torch.cuda.is_available(), "tools/time_scan_islands.py needs a GPU"
    print("device: %s" % torch.cuda.get_device_name(0))
    for leg in args.legs.split(","):
        {"kernel": kernel_legs, "paths": path_legs}[leg](args)


if __name__ == "__main__":
    main()
