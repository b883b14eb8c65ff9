"""Timing of the scan meshes' curvature (geot_mesh_angle_defects, geot_scan_ball_sum in both GEOT_BALL_SUM_IMPL forms,
geot_curvature_sample, DeviceScanSet.compute_curvature, curvatures=True on the batchers) against a torch composite of the same
definition; profiles/mesh_curvature_timing.txt holds one run's output.  Device events around windows of calls, the legs
alternated in one process, every leg timed in two series so that the spread shows, every shape warmed first.

  kernel   the two height-field meshes of tools/time_mesh_neighbours.py (about 1e5 vertices and 2e5 faces each, 0.2 mm edges,
           63 mm across: 32 cells of 2 mm per axis at any radius below that): the defect call over both, the ball sum of the
           first in both forms at the default radius 0.1 (below the edge: a ball holds its centre alone) and at 0.5 (a few tens
           of members), compute_curvature over both, the sample launch, and the torch composite -- index_add_ on the angles,
           chunked cdist for the ball (in float64: the fp32 matmul form moves members across the radius) -- which is the
           comparison, never the code under test.  The two forms are compared bit for bit, and the composite's largest
           difference is printed, before anything is timed.
  batch    a ValBatcher and a FixMatchBatcher batch with the switch on and off.  --package-root times the off legs of another
           checkout (the parent commit's) with the same script, for the comparison the file states.

    python tools/time_mesh_curvature.py [--legs kernel,batch] [--package-root DIR] [--side 317]"""
import argparse
import inspect
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_mesh_neighbours import scan_set      # noqa: E402
from time_tooth_scores import summary, window      # noqa: E402


def composite_defects(points, faces):
    """The defects of one scan with torch ops: fp32 angles by atan2, index_add_ per corner -> (M,) float32."""
    import torch
    p = points[faces.long()]                                  # (F, 3, 3)
    total = torch.zeros(points.shape[0], dtype=torch.float32, device=points.device)
    for e in range(3):
        u, v = p[:, (e + 1) % 3] - p[:, e], p[:, (e + 2) % 3] - p[:, e]
        ang = torch.atan2(torch.linalg.cross(u, v).norm(dim=1), (u * v).sum(1))
        total.index_add_(0, faces[:, e].long(), ang)
    return 2 * np.pi - total


def composite_ball(points, value, radius, chunk=1024):
    """The closed-ball sum with chunked cdist -> (M,) float32.  In float64: cdist's fp32 matmul form errs by about 1e-4 in d^2 at
    these coordinates, which moves members across the radius."""
    import torch
    out = torch.empty(points.shape[0], dtype=torch.float32, device=points.device)
    wide = points.double()
    for first in range(0, points.shape[0], chunk):
        inside = torch.cdist(wide[first:first + chunk], wide) <= radius
        out[first:first + chunk] = (inside * value[None, :]).sum(1)
    return out


def timed(legs, args, prepare=None):
    import torch
    times = {name: ([], []) for name in legs}
    for series in (0, 1):                                            # every leg twice: the spread between series shows
        for _ in range(args.rounds):
            for name, (fn, calls) in legs.items():                   # alternating
                if prepare:
                    prepare(name)
                window(fn, min(2, calls))                            # warm
                times[name][series].append(window(fn, calls))
    torch.cuda.synchronize()
    for name in legs:
        print("  %-58s series 1 %s; series 2 %s" % (name, summary(times[name][0]), summary(times[name][1])))


def kernel_legs(args):
    import torch
    from geot_amd import _lib
    from geot_amd.ext._common import call, ptr
    from geot_amd.openpoints.dataset.scan_set import curvature_sample
    dev = torch.device("cuda:0")
    dset, _, _ = scan_set([args.side, args.side - 6], dev, [0, 1])
    sizes, lib = list(dset.sizes), _lib.load()
    m0 = sizes[0]
    pts0, faces0 = dset.points[:m0], dset.faces[:dset.face_sizes[0]]
    st = dset.compute_curvature(0.5, stats=True)
    defects, cur5 = dset.defects.clone(), dset.curvature.clone()
    print("kernel: 2 meshes of %s vertices and %s faces; defect stats (usable, ignored, degenerate faces, vertices in no usable face) %s"
          % (sizes, dset.face_sizes, st.cpu().tolist()))
    # both forms give the same bits; the composite agrees within fp32 summation error
    out = torch.empty(m0, dtype=torch.float32, device=dev)
    keys = torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.geot_scan_ball_sum_ws_bytes(m0)), dtype=torch.uint8, device=dev)

    def ball(radius):
        return lambda: call("geot_scan_ball_sum", dev, m0, radius, ptr(pts0), ptr(defects), ptr(out), ptr(keys), ptr(ws), ws.numel())
    for radius in (0.1, 0.5):
        bits = []
        for impl in (None, "basic"):
            os.environ.pop("GEOT_BALL_SUM_IMPL", None)
            if impl:
                os.environ["GEOT_BALL_SUM_IMPL"] = impl
            ball(radius)()
            bits.append((out.clone(), keys.clone()))
        os.environ.pop("GEOT_BALL_SUM_IMPL", None)
        assert torch.equal(bits[0][0], bits[1][0]) and torch.equal(bits[0][1], bits[1][1])
        comp_d = composite_defects(pts0, faces0)
        comp = composite_ball(pts0, comp_d, radius)
        members = composite_ball(pts0, torch.ones_like(comp_d), radius)
        print("  radius %.1f: ball members mean %.1f, max %d; |kernel - composite| max %.3g on curvature in [%.3g, %.3g]"
              % (radius, float(members.mean()), int(members.max()), float((bits[0][0] - comp).abs().max()), float(comp.min()), float(comp.max())))
    assert torch.equal(cur5[:m0], bits[0][0])
    b_ws = torch.empty(int(lib.geot_mesh_angle_defects_ws_bytes(sum(sizes))), dtype=torch.uint8, device=dev)
    dq = torch.empty(sum(sizes), dtype=torch.int64, device=dev)
    chunk = dset._curvature_tables[0][0]

    def defect_call():
        call("geot_mesh_angle_defects", dev, chunk[0], 2, sum(sizes), int(dset.faces.shape[0]), ptr(dset.points), ptr(dset.faces),
             ptr(dset.offsets), ptr(dset.face_offsets), ptr(chunk[2]), ptr(chunk[3]), ptr(chunk[4]), chunk[1], sum(sizes), ptr(dq),
             None, ptr(b_ws), b_ws.numel())
    ids = torch.tensor([0, 1, 0, 1], dtype=torch.int64, device=dev)
    sel = torch.randint(0, min(sizes), (4, args.points), device=dev)
    legs = {"geot_mesh_angle_defects, both meshes": (defect_call, args.calls),
            "geot_scan_ball_sum, first mesh, radius 0.1, lane per vertex": (ball(0.1), args.calls),
            "geot_scan_ball_sum, first mesh, radius 0.1, basic (wave per vertex)": (ball(0.1), args.calls),
            "geot_scan_ball_sum, first mesh, radius 0.5, lane per vertex": (ball(0.5), args.calls),
            "geot_scan_ball_sum, first mesh, radius 0.5, basic (wave per vertex)": (ball(0.5), args.calls),
            "compute_curvature(0.1), both meshes": (lambda: dset.compute_curvature(0.1), args.calls),
            "geot_curvature_sample, 4 slots of %d" % args.points: (lambda: curvature_sample(dset, ids, sel), args.calls),
            "torch composite: defects, first mesh": (lambda: composite_defects(pts0, faces0), args.calls),
            "torch composite: ball sum (chunked float64 cdist), first mesh": (lambda: composite_ball(pts0, comp_d, 0.1), 1)}

    def prepare(name):
        os.environ.pop("GEOT_BALL_SUM_IMPL", None)
        if "basic" in name:
            os.environ["GEOT_BALL_SUM_IMPL"] = "basic"
    timed(legs, args, prepare)
    os.environ.pop("GEOT_BALL_SUM_IMPL", None)


def batch_legs(args):
    import torch
    from geot_amd.openpoints.dataset import FixMatchBatcher, ValBatcher
    from geot_amd.openpoints.dataset.sample_draw import DeviceDraws
    dev = torch.device("cuda:0")
    has = "curvatures" in inspect.signature(ValBatcher.__init__).parameters
    sets = [scan_set([args.side, args.side - 6], dev, [0, 1])[0] for _ in range(2)]
    if has:
        for s in sets:
            s.compute_curvature(0.1)
    print("batch: sets of 2 meshes of %s vertices, %d samples, device draws; package %s (%s)"
          % (list(sets[0].sizes), args.points, os.path.dirname(inspect.getfile(ValBatcher)), "with curvatures=" if has else "before the feature"))
    legs = {}
    for on in ((False, True) if has else (False,)):
        kw = {"curvatures": True} if on else {}
        val = ValBatcher(sets[0], args.points, draws=DeviceDraws(5), **kw)
        fix = FixMatchBatcher(sets[0], sets[1], args.points, draws=DeviceDraws(5, views=True), **kw)
        legs["ValBatcher.batch, 2 scans, curvatures %s" % ("on" if on else "off")] = (lambda val=val: val.batch([0, 1]), args.calls)
        legs["FixMatchBatcher.batch, 2 + 2 scans, curvatures %s" % ("on" if on else "off")] = (lambda fix=fix: fix.batch([0, 1], [1, 0]), args.calls)
    timed(legs, args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="kernel,batch")
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose geot_amd is timed (default: this one)")
    ap.add_argument("--side", type=int, default=317, help="vertices along one side of the first mesh (317: 100 489 vertices)")
    ap.add_argument("--points", type=int, default=16000, help="samples per batch slot")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    assert torch.cuda.is_available(), "tools/time_mesh_curvature.py needs a GPU"
    print("device: %s" % torch.cuda.get_device_name(0))
    for leg in args.legs.split(","):
        {"kernel": kernel_legs, "batch": batch_legs}[leg](args)


if __name__ == "__main__":
    main()
