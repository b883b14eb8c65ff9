"""Timing of the scan meshes' one-ring tables (geot_mesh_neighbours, validation.mesh_neighbours, mesh= on clean_scans, islands=
{"mesh": ...} on the validators) against the kNN table they replace, and of the set's table cache (DeviceScanSet.keep_tables);
profiles/mesh_neighbours_timing.txt holds one run's output.  Device events around windows of calls, the legs alternated in one
process, every leg timed in two series so that the spread shows, every shape warmed first.

  kernel   B = 2 synthetic meshes -- triangulated height fields of 317 x 317 and 311 x 311 vertices: about 1e5 vertices and 2e5
           faces each, the faces in a shuffled order -- C = 17, labels in bands plus clusters of wrong labels:
           mesh_neighbours(k = 16) in both GEOT_MESH_NEIGHBOURS_IMPL forms, scan_neighbours(k = 8), clean_scans end to end on
           either table, and the same two with the cache warm.  The two forms are compared bit for bit before anything is timed.
  paths    validate_scans on the small segmentor over four such meshes: islands off, islands=True and islands={"mesh": True},
           the last two with the cache off and on, each leg timed --repeats times, alternating.  --package-root times the off
           path of another checkout (the parent commit's) with the same script, for the comparison the file states.

    python tools/time_mesh_neighbours.py [--legs kernel,paths] [--package-root DIR] [--side 317]"""
import argparse
import inspect
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_tooth_scores import SMALL, C, summary, window      # noqa: E402


def height_field(side, seed):
    """A triangulated height field of side x side vertices in millimetres, row-major (a spatially coherent vertex order):
    (points (side^2, 3) fp32, labels (side^2,) int32 in bands of teeth around a gingiva, faces (2 (side - 1)^2, 3) int32 in a
    shuffled order with turned corners)."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    u, v = x.reshape(-1) * 0.2, y.reshape(-1) * 0.2                    # 0.2 mm edges: about 63 mm across
    z = 3.0 * np.sin(u / 5.0 + seed) * np.cos(v / 7.0) + 0.02 * rng.standard_normal(u.size)
    points = (np.stack([u, v, z], 1) + np.array([14.0, -37.0, 61.0])).astype(np.float32)
    tooth = 1 + (x.reshape(-1) * 8 // side) + 8 * (y.reshape(-1) * 2 // side)
    labels = np.where((y.reshape(-1) % (side // 2)) < side // 8, 0, tooth).astype(np.int32) % C
    a = (y[:-1, :-1] * side + x[:-1, :-1]).reshape(-1)
    faces = np.stack([np.stack([a, a + 1, a + side], 1), np.stack([a + 1, a + side + 1, a + side], 1)], 1).reshape(-1, 3)
    turn = rng.integers(0, 3, size=len(faces))
    faces = np.stack([np.take_along_axis(faces, ((turn + j) % 3)[:, None], 1)[:, 0] for j in range(3)], 1)
    return points, labels, np.ascontiguousarray(faces[rng.permutation(len(faces))].astype(np.int32))


def noisy_labels(labels, side, seed):
    """A prediction with stray vertices and square clusters of 2 x 2 .. 6 x 6 vertices of one wrong class."""
    rng = np.random.default_rng(seed)
    pred = labels.astype(np.int64).copy()
    flip = rng.random(len(pred)) < 0.02
    pred[flip] = rng.integers(0, C, size=int(flip.sum()))
    grid = pred.reshape(side, side)
    for _ in range(len(pred) // 500):
        r, c, e = int(rng.integers(side - 6)), int(rng.integers(side - 6)), int(rng.integers(2, 7))
        grid[r:r + e, c:c + e] = int(rng.integers(C))
    return pred


def scan_set(sides, dev, cls):
    """-> (set, the meshes, whether this package's DeviceScanSet takes faces)."""
    from geot_amd.openpoints.dataset import DeviceScanSet
    meshes = [height_field(side, 900 + i) for i, side in enumerate(sides)]
    has_faces = "faces" in inspect.signature(DeviceScanSet.__init__).parameters
    kw = {"faces": [f for _, _, f in meshes]} if has_faces else {}
    return DeviceScanSet([p for p, _, _ in meshes], [l for _, l, _ in meshes], cls=cls, device=dev, **kw), meshes, has_faces


def kernel_legs(args):
    import torch
    from geot_amd import validation as V
    from geot_amd.ext import _common
    dev = torch.device("cuda:0")
    sides = [args.side, args.side - 6]
    dset, meshes, _ = scan_set(sides, dev, [0, 1])
    sizes = list(dset.sizes)
    batch = {"scans": dset, "sizes": sizes, "scan_ids": torch.arange(2, device=dev), "mandible": [True, False],
             "points": list(torch.split(dset.points, sizes)), "ids": [0, 1]}
    noisy = torch.from_numpy(np.concatenate([noisy_labels(l, side, 40 + i) for i, ((_, l, _), side) in enumerate(zip(meshes, sides))])).to(dev)
    work = noisy.clone()
    views = [p.view(1, -1) for p in torch.split(work, sizes)]

    def fresh():
        work.copy_(noisy)

    def clean(**kw):
        def go():
            fresh()
            V.clean_scans(views, batch, num_classes=C, **kw)
        return go
    # name -> (GEOT_MESH_NEIGHBOURS_IMPL, the set's cache on, the call)
    legs = {"copy of the labels (in every clean_scans leg)": (None, False, fresh),
            "mesh_neighbours, k = 16, combined": (None, False, lambda: V.mesh_neighbours(batch, 16)),
            "mesh_neighbours, k = 16, basic": ("basic", False, lambda: V.mesh_neighbours(batch, 16)),
            "scan_neighbours, k = 8": (None, False, lambda: V.scan_neighbours(batch, 8)),
            "clean_scans, kNN table (search + islands)": (None, False, clean()),
            "clean_scans, mesh=True (one-ring + islands)": (None, False, clean(mesh=True)),
            "clean_scans, kNN table, cache warm": (None, True, clean()),
            "clean_scans, mesh=True, cache warm": (None, True, clean(mesh=True))}

    def run(name):
        impl, keep, fn = legs[name][:3]
        if impl:
            os.environ["GEOT_MESH_NEIGHBOURS_IMPL"] = impl
        else:
            os.environ.pop("GEOT_MESH_NEIGHBOURS_IMPL", None)
        if keep != dset._keep:
            dset.keep_tables(keep)          # (switching off drops the tables; the first call after switching on builds them)
        return fn
    # the same bits from both forms and from the cache, before anything is timed
    table, stats = V.mesh_neighbours(batch, 16, stats=True)
    assert torch.equal(run("mesh_neighbours, k = 16, basic")(), table)
    dset.keep_tables()
    assert torch.equal(V.mesh_neighbours(batch, 16), table) and torch.equal(V.mesh_neighbours(batch, 16), table)
    dset.keep_tables(False)
    outs = []
    for kw in ({}, {"mesh": True}):
        fresh()
        _, st = V.clean_scans(views, batch, num_classes=C, stats=True, **kw)
        outs.append((work.clone(), st.cpu().tolist()))
    print("kernel: B = 2 meshes of %s vertices and %s faces, C = %d; mesh table (sum M, 16), stats (usable faces, ignored, truncated, "
          "longest row) %s; kNN table (sum M, 9)" % (sizes, dset.face_sizes, C, stats.cpu().tolist()))
    print("  clean_scans stats (components, islands, changed, stranded): kNN table %s, mesh table %s; the two cleaned label sets "
          "differ on %d of %d vertices" % (outs[0][1], outs[1][1], int((outs[0][0] != outs[1][0]).sum()), sum(sizes)))
    notes = {}
    for name in legs:
        fn = run(name)
        fn()
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
        notes[name] = "calls %s; peak memory above the inputs %.2f MB" % (", ".join(seen) or "none", peak / 1e6)
    times = {name: ([], []) for name in legs}
    for series in (0, 1):                                            # every leg twice: the spread between series shows
        for _ in range(args.rounds):
            for name in legs:                                        # alternating
                fn = run(name)
                window(fn, 3)                                        # warm (and, after a cache switch, build)
                times[name][series].append(window(fn, args.calls))
    os.environ.pop("GEOT_MESH_NEIGHBOURS_IMPL", None)
    dset.keep_tables(False)
    for name in legs:
        print("  %-48s series 1 %s; series 2 %s; %s" % (name, summary(times[name][0]), summary(times[name][1]), notes[name]))


def path_legs(args):
    import logging
    import torch
    from geot_amd import validation as V
    from geot_amd.ext import _common
    from geot_amd.openpoints.dataset import ValBatcher
    from geot_amd.openpoints.dataset.sample_draw import DeviceDraws
    from geot_amd.openpoints.models.segmentation import WholePartSeg
    logging.disable(logging.CRITICAL)
    dev = torch.device("cuda:0")
    sides = [args.side, args.side - 6, args.side + 3, args.side - 20]
    dset, _, has_mesh = scan_set(sides, dev, [0, 1, 0, 1])
    torch.manual_seed(5)
    model = WholePartSeg(segmentor_args=dict(NAME="PointTransformer_seg_T", **SMALL)).to(dev).eval()
    cfg = {"num_classes": C, "num_points": 4096, "epoch": 1, "epochs": 1}
    print("paths: %d meshes of %s vertices, batches of 2, 4096 samples, the small segmentor; package %s (%s)" %
          (len(sides), list(dset.sizes), os.path.dirname(V.__file__), "with faces= and mesh=" if has_mesh else "before the feature"))

    def leg(islands, keep):
        def go():
            if has_mesh and keep != dset._keep:
                dset.keep_tables(keep)
            return V.validate_scans(model, ValBatcher(dset, 4096, draws=DeviceDraws(5)), cfg, **({} if islands is None else {"islands": islands}))
        return go
    legs = {"validate_scans, islands off": leg(None, False)}
    if has_mesh:
        legs.update({"validate_scans, islands=True, cache off": leg(True, False),
                     "validate_scans, islands={'mesh': True}, cache off": leg({"mesh": True}, False),
                     "validate_scans, islands=True, cache on": leg(True, True),
                     "validate_scans, islands={'mesh': True}, cache on": leg({"mesh": True}, True)})
    results, times, calls = {}, {name: [] for name in legs}, {}
    for name, go in legs.items():
        go()
        results[name] = go()                                         # warm (twice: the first call with the cache on builds)
        seen = []
        _common.trace = lambda launch, entry: (seen.append(entry), launch())[1]
        try:
            go()
        finally:
            _common.trace = None
        own = [s for s in seen if s.startswith(("geot_scan", "geot_seg_confusion", "geot_knn_sorted_ws", "geot_mesh"))]
        calls[name] = ", ".join("%s x %d" % (s, own.count(s)) for s in dict.fromkeys(own))
    for _ in range(args.repeats):
        for name, go in legs.items():                                # alternating
            go()                                                     # (after a cache switch: builds the tables again)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            go()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    batches = len(sides) // 2
    for name in legs:
        print("  %-50s %s ms per call (host clock, ends in a synchronise), %d batches; (macc, miou, mdsc) = %s" %
              (name, ", ".join("%.3f" % v for v in times[name]), batches, tuple(float(v) for v in results[name])))
        print("      whole-scan calls of one validation (the model's own searches among the geot_knn_sorted_ws): %s" % calls[name])
    off = np.median(times["validate_scans, islands off"])
    for name in legs:
        if name != "validate_scans, islands off":
            print("  %s: adds %.3f ms per batch over islands off (medians %.3f -> %.3f ms per call)" %
                  (name, (np.median(times[name]) - off) / batches, off, np.median(times[name])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="kernel,paths")
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose geot_amd is timed (default: this one)")
    ap.add_argument("--side", type=int, default=317, help="vertices along one side of the first mesh (317: 100 489 vertices)")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=6)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    assert torch.cuda.is_available(), "tools/time_mesh_neighbours.py needs a GPU"
    print("device: %s" % torch.cuda.get_device_name(0))
    for leg in args.legs.split(","):
        {"kernel": kernel_legs, "paths": path_legs}[leg](args)


if __name__ == "__main__":
    main()
