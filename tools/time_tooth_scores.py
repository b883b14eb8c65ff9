"""Timing of the Teeth3DS challenge scores (geot_tooth_moments, validation.ToothScores); profiles/tooth_scores_timing.txt holds
one run's output.  Device events around windows of calls, the legs alternated in one process, every shape warmed first.

  kernel   B = 2 synthetic scans of about 1e5 vertices in a spatially coherent vertex order, C = 17: geot_tooth_moments in both
           GEOT_TOOTH_MOMENTS_IMPL forms and at several record lengths, against the same moments made with torch ops
           (index_add_ / scatter_reduce_ on int64); the three are compared bit for bit before anything is timed.  Launches,
           peak memory and the achieved bytes per second against the 24 B per vertex the shapes require.
  paths    validate_scans and validate_scans_decoded on the small segmentor over four such scans, with teeth=None and with a
           ToothScores, each leg timed --repeats times, alternating.  --package-root times the off path of another checkout
           (the parent commit's) with the same script, for the comparison the file states.

    python tools/time_tooth_scores.py [--legs kernel,paths] [--package-root DIR] [--vertices 100000]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(trans_dim=384, depth=3, num_heads=4, group_size=32, num_group=128, encoder_dims=256, nclasses=17,
             drop_path_rate=0.0, downsample_targets=[2048, 1024, 512], extract_layers=[1, 2, 3])
C = 17
BYTES_PER_VERTEX = 24       # 12 of position, 4 of label, 8 of prediction


def coherent_scan(m, index):
    """A synthetic scan in millimetres whose vertex order is spatially coherent (sorted by coarse grid cell), with
    region_labels' classes: (points (m, 3) fp32, labels (m,) int32)."""
    from geot_amd.synth import make_cloud, region_labels
    unit = make_cloud(m, index)[0]
    cell = np.floor((unit + 1.0) * 8).astype(np.int64)
    order = np.lexsort((unit[:, 0], cell[:, 0], cell[:, 1], cell[:, 2]))
    unit = unit[order]
    points = (unit * np.float32(31.5) + np.array([14.0, -37.0, 61.0], np.float32)).astype(np.float32)
    return points, (region_labels(unit) % C).astype(np.int32)


def window(fn, calls):
    """Device time of `calls` consecutive fn() in ms per call."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def summary(values):
    v = sorted(values)
    return "median %.4f ms (min %.4f, max %.4f, %d windows)" % (v[len(v) // 2], v[0], v[-1], len(v))


def op_counter():
    """A dispatch mode that counts the aten ops a block issues (the torch composite's launches: each op is at least one kernel)."""
    from torch.utils._python_dispatch import TorchDispatchMode

    class Counter(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.n += 1
            return func(*args, **(kwargs or {}))
    return Counter()


def torch_moments(points, labels, pred, center, slot, b):
    """The same rows with torch ops: 2 x (1 + 3 index_add_ + 6 scatter_reduce_) + 3 index_add_ over int64."""
    import torch
    words = 21 * C + 2
    rows = torch.zeros(b * words, dtype=torch.int64, device=points.device)
    d = points - center[slot]
    usable = (d.abs() < 16384).all(1)
    q = torch.round(d * 65536.0).nan_to_num(0.0, 0.0, 0.0).to(torch.int64)
    lab = labels.to(torch.int64)
    base = slot * words
    one = torch.ones_like(base)
    l_in, p_in = usable & (lab >= 0) & (lab < C), usable & (pred >= 0) & (pred < C)
    for side, key, on in ((0, lab, l_in), (10, pred, p_in)):
        at, qq = (base + key * 21 + side)[on], q[on]
        rows.index_add_(0, at, one[on])
        for a in range(3):
            rows.index_add_(0, at + 1 + a, qq[:, a])
            rows.scatter_reduce_(0, at + 4 + a, qq[:, a] + (1 << 30), "amax")
            rows.scatter_reduce_(0, at + 7 + a, (1 << 30) - qq[:, a], "amax")
    hit = l_in & (lab == pred)
    rows.index_add_(0, (base + lab * 21 + 20)[hit], one[hit])
    both = l_in & p_in & (lab >= 1) & (pred >= 1)
    rows.index_add_(0, (base + words - 2)[both], one[both])
    rows.index_add_(0, (base + words - 1)[~usable], one[~usable])
    return rows.view(b, words)


def kernel_legs(args):
    import torch
    from geot_amd.ext import _common
    from geot_amd.ext._common import call, ptr
    from geot_amd.validation import scan_work_table
    dev = torch.device("cuda:0")
    sizes = [args.vertices, args.vertices - 3217]
    scans = [coherent_scan(m, 900 + i) for i, m in enumerate(sizes)]
    rng = np.random.default_rng(1)
    pred_np = np.concatenate([l for _, l in scans]).astype(np.int64)
    flip = rng.random(len(pred_np)) < 0.05                          # a prediction 95 % right
    pred_np[flip] = rng.integers(0, C, size=int(flip.sum()))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    points, labels, pred = t(np.concatenate([p for p, _ in scans])), t(np.concatenate([l for _, l in scans])), t(pred_np)
    offsets = t(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    scan_ids, out_offsets = t(np.arange(2, dtype=np.int64)), t(np.array([0, sizes[0]], np.int64))
    center = t(np.stack([p.mean(0) for p, _ in scans]).astype(np.float32))
    slot = torch.repeat_interleave(torch.arange(2, device=dev), t(np.asarray(sizes, np.int64)))
    total, words = sum(sizes), 21 * C + 2
    rows = torch.zeros((2, words), dtype=torch.int64, device=dev)
    tables = {chunk: t(scan_work_table(sizes, min_chunk=chunk)) for chunk in args.chunks}

    def ours(chunk):
        work = tables[chunk]
        rows.zero_()
        call("geot_tooth_moments", dev, 2, C, 2, total, ptr(points), ptr(labels), ptr(offsets), ptr(scan_ids), ptr(center),
             int(work.shape[0]), ptr(work), ptr(out_offsets), ptr(pred), ptr(rows))

    legs = {}
    for chunk in args.chunks:
        for impl in ("combined", "basic"):
            legs["hip %s, records of %d (%d workgroups)" % (impl, chunk, tables[chunk].shape[0])] = (impl, lambda chunk=chunk: ours(chunk))
    legs["torch composite"] = (None, lambda: torch_moments(points, labels, pred, center, slot, 2))

    def run(name):
        impl, fn = legs[name][:2]
        if impl == "basic":
            os.environ["GEOT_TOOTH_MOMENTS_IMPL"] = "basic"
        else:
            os.environ.pop("GEOT_TOOTH_MOMENTS_IMPL", None)
        return fn
    # the same bits from every leg, before anything is timed
    want = torch_moments(points, labels, pred, center, slot, 2)
    for name in legs:
        if legs[name][0] is not None:
            run(name)()
            assert torch.equal(rows, want), name
    print("kernel: B = 2 scans of %d and %d vertices, C = %d; every leg gives the same %d x %d int64 rows" % (sizes[0], sizes[1], C, 2, words))
    # launches (traced entry points, aten ops) and peak memory of one call
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
            with op_counter() as ops:
                fn()
        finally:
            _common.trace = None
        torch.cuda.synchronize()
        launches = "%d library launches, %d aten ops (each at least one kernel or memset)" % (len(seen), ops.n)
        legs[name] = legs[name] + ("%s, peak memory above the inputs %.2f MB" % (launches, peak / 1e6),)
    times = {name: [] for name in legs}
    for name in legs:
        window(run(name), 10)                                        # warm
    for _ in range(args.rounds):
        for name in legs:                                            # alternating
            times[name].append(window(run(name), args.calls))
    os.environ.pop("GEOT_TOOTH_MOMENTS_IMPL", None)
    need = BYTES_PER_VERTEX * total
    print("required traffic: %d B per vertex x %d vertices = %.2f MB per call; each hip leg includes the zeroing of the rows" %
          (BYTES_PER_VERTEX, total, need / 1e6))
    for name in legs:
        med = sorted(times[name])[len(times[name]) // 2]
        print("  %-52s %s; %.1f GB/s of required bytes; %s" % (name, summary(times[name]), need / med / 1e6, legs[name][2]))


def path_legs(args):
    import torch
    from geot_amd.openpoints.dataset import DeviceScanSet, ValBatcher
    from geot_amd.openpoints.dataset.sample_draw import DeviceDraws
    from geot_amd.openpoints.models.segmentation import WholePartSeg
    from geot_amd import validation as V
    import logging
    logging.disable(logging.CRITICAL)
    dev = torch.device("cuda:0")
    sizes = [args.vertices, args.vertices - 3217, args.vertices + 1741, args.vertices - 12345]
    scans = [coherent_scan(m, 900 + i) for i, m in enumerate(sizes)]
    dset = DeviceScanSet([p for p, _ in scans], [l for _, l in scans], cls=[0, 1, 0, 1], device=dev)
    torch.manual_seed(5)
    model = WholePartSeg(segmentor_args=dict(NAME="PointTransformer_seg_T", **SMALL)).to(dev).eval()
    cfg = {"num_classes": C, "num_points": 4096, "epoch": 1, "epochs": 1}
    has_teeth = hasattr(V, "ToothScores")
    print("paths: %d scans of %s vertices, batches of 2, 4096 samples, the small segmentor; package %s (%s)" %
          (len(sizes), sizes, os.path.dirname(V.__file__), "with teeth=" if has_teeth else "before the feature"))

    def leg(fn, teeth):
        def go():
            kw = {"teeth": V.ToothScores(C, dev)} if teeth else {}
            out = fn(model, ValBatcher(dset, 4096, draws=DeviceDraws(5)), cfg, **kw)
            return out, (kw["teeth"].read() if teeth else None)
        return go
    legs = {}
    for label, fn in (("validate_scans", V.validate_scans), ("validate_scans_decoded", V.validate_scans_decoded)):
        legs[label + " teeth=None"] = leg(fn, False)
        if has_teeth:
            legs[label + " teeth=ToothScores"] = leg(fn, True)
    results, times = {}, {name: [] for name in legs}
    for name, go in legs.items():
        results[name] = go()                                         # warm
    for _ in range(args.repeats):
        for name, go in legs.items():                                # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            go()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    batches = len(sizes) // 2
    for name in legs:
        print("  %-44s %s ms per call (host clock, ends in a synchronise), %d batches; (macc, miou, mdsc) = %s" %
              (name, ", ".join("%.3f" % v for v in times[name]), batches, tuple(float(v) for v in results[name][0])))
    for label in ("validate_scans", "validate_scans_decoded"):
        if has_teeth:
            off, on = times[label + " teeth=None"], times[label + " teeth=ToothScores"]
            print("  %s: teeth= adds %.3f ms per batch (medians %.3f -> %.3f ms per call); the three-tuple is %s" %
                  (label, (np.median(on) - np.median(off)) / batches, np.median(off), np.median(on),
                   "unchanged" if all(float(a) == float(b) or (a != a and b != b) for a, b in
                                      zip(results[label + " teeth=None"][0], results[label + " teeth=ToothScores"][0])) else "CHANGED"))
            out = results[label + " teeth=ToothScores"][1]
            print("    tsa %.5f tsa_instance %.5f tla %.5f tir %.5f score %.5f" % tuple(out[k] for k in ("tsa", "tsa_instance", "tla", "tir", "score")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="kernel,paths")
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose geot_amd is timed (default: this one)")
    ap.add_argument("--vertices", type=int, default=100000)
    ap.add_argument("--chunks", type=lambda s: [int(v) for v in s.split(",")], default=[64, 256, 1024, 4096])
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    assert torch.cuda.is_available(), "tools/time_tooth_scores.py needs a GPU"
    print("device: %s" % torch.cuda.get_device_name(0))
    for leg in args.legs.split(","):
        {"kernel": kernel_legs, "paths": path_legs}[leg](args)


if __name__ == "__main__":
    main()
