"""Transform lists as view programs (geot_view_program), timed.  A report; leg (iii) also prints the comparison that decides
whether the hard-wired views kernel can be retired.

    python tools/time_view_program.py [--reps 60] [--warmup 8] [--legs i,ii,iii]

(i)  one supervised batch at the configured size, 8 scans x 24 000 points of ~1e5-vertex scans, default.yaml's `train` list:
     SupervisedBatcher.batch (geot_cloud_sample_batch + ONE geot_view_program launch) against the same batch composed from
     what the package offered before: cloud_sample_batch + torch elementwise / reduction ops for the five transforms.  Both
     get the same pre-drawn indices, scales, noise and drop flags; both upload the noise through pinned memory inside the
     timed window.
(ii) the three configured FixMatch lists, 2 labelled + 2 weak + 2 strong views (the configured batch: 6 jobs), through
     view_program_views and through fixmatch_views (geot_fixmatch_views, the kernel FixMatchBatcher keeps by default), at
     m = 16 000 and 24 000 (register-resident) and 30 000 (streaming).
(iii) one FixMatch batch, B_l = B_u = 2 on the same scans, at m = 16 000 and 24 000: FixMatchBatcher.batch(idx_l, idx_u,
     sel_l=, sel_u=, params=) with everything given, so the host draws nothing, once from a batcher built with
     transforms=None (params are s / R / t dicts) and once from one built with transforms=CONFIGURED_LISTS (params are
     ViewProgram.draw lists holding the same values).  Where the two are two kernels this is the comparison of the batch a
     training loop pays for; the line `gate` holds the second to the first's median plus the first's own p10 .. p90 spread.

The legs of a pair alternate after warm-up.  Per repetition two figures: `dev` = the time between two events recorded on the
stream around the call (the device's view: kernels, copies and any gap the host leaves between them) and `wall` = the
device-synchronised wall time of the call.  Medians, with the spread p10 .. p90.  Launch counts are the device kernels
torch.profiler sees in one call (copies not counted).
"""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geot_amd.openpoints.dataset import (DEFAULT_TRAIN, DEFAULT_TRAIN_KWARGS, TOOTH_VIEW_KWARGS, DeviceScanSet, FixMatchBatcher,  # noqa: E402
                                         SupervisedBatcher, ViewProgram, cloud_sample_batch, draw_view_params, fixmatch_views,
                                         view_program_views)
from geot_amd.openpoints.dataset.fixmatch_batch import CONFIGURED_LISTS  # noqa: E402

DEV = torch.device("cuda:0")
B, M, VERTICES = 8, 24000, (100003, 98765, 120011, 90001, 110503, 99991, 104729, 95003)
CONFIGURED = {"train": ["PointsToTensor", "PointCloudScaling", "PointCloudCenterAndNormalize"],
              "train_w": ["PointsToTensor", "PointCloudCenterAndNormalize"],
              "train_s": ["PointsToTensor", "PointCloudScaling_s", "PointCloudCenterAndNormalize", "PointCloudRotation_s",
                          "PointCloudTranslation_s"]}


def scans(part=slice(None)):
    rng = np.random.default_rng(3)
    pts = [(rng.standard_normal((n, 3)) * np.array([30, 20, 8]) + np.array([250, -400, 120])).astype(np.float32) for n in VERTICES]
    return DeviceScanSet(pts[part], [rng.integers(0, 17, n).astype(np.int32) for n in VERTICES][part], device=DEV)


def measure(legs, reps, warmup):
    """legs: name -> callable.  -> name -> (dev ms list, wall ms list), the legs alternating."""
    out = {k: ([], []) for k in legs}
    for r in range(warmup + reps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if r >= warmup:
                out[name][0].append(a.elapsed_time(b))
                out[name][1].append((t1 - t0) * 1e3)
    return out


def kernels(fn):
    """Device kernels of one call, by torch.profiler (None when the profiler is unavailable)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and "Memcpy" not in e.name and "Memset" not in e.name]
        return len(names)
    except Exception as e:      # noqa: BLE001
        print("  (kernel count unavailable: %s)" % str(e)[:120])
        return None


def line(tag, name, res, launches):
    dev, wall = (np.array(v) for v in res)
    q = lambda v: (np.median(v), np.percentile(v, 10), np.percentile(v, 90))     # noqa: E731
    print("  %-4s %-34s dev %7.3f ms (p10 %7.3f .. p90 %7.3f)   wall %7.3f ms (p10 %7.3f .. p90 %7.3f)   kernels %s"
          % ((tag, name) + q(dev) + q(wall) + ("n/a" if launches is None else launches,)))
    return float(np.median(dev))


def leg_i(reps, warmup):
    print("(i) one supervised batch, %d x %d points, list %s" % (B, M, DEFAULT_TRAIN[1:]))
    sset = scans()
    batcher = SupervisedBatcher(sset, M)
    np.random.seed(1)
    torch.manual_seed(1)
    random.seed(1)
    idx = list(range(B))
    sel, params = batcher.draw(idx)
    scale = np.stack([p[1]["scale"] for p in params])
    noise = np.stack([p[3]["noise"] for p in params])
    keep = np.array([0.0 if p[4]["drop"] else 1.0 for p in params], np.float32)
    g = DEFAULT_TRAIN_KWARGS["gravity_dim"]

    def program():
        return batcher.batch(idx, sel=sel, params=params)

    def composed():
        s = cloud_sample_batch(sset, idx, sel, 17, check=False)
        up = lambda a: torch.from_numpy(a).pin_memory().to(DEV, non_blocking=True)     # noqa: E731
        sc, nz, kp = up(scale), up(noise), up(keep)
        pos = s["raw"] * sc[:, None, :]                                   # PointCloudScaling (x is pos)
        x = pos.transpose(1, 2).contiguous()
        col = pos[:, :, g:g + 1]
        heights = col - col.amin(dim=1, keepdim=True)                     # PointCloudCenterAndNormalize
        pos = pos - pos.mean(dim=1, keepdim=True)
        pos = pos / pos.pow(2).sum(-1, keepdim=True).sqrt().amax(dim=1, keepdim=True)
        pos = pos + nz                                                    # PointCloudJitter
        x = x * kp[:, None, None]                                         # ChromaticDropGPU
        cls = sset.cls.index_select(0, s["scan_ids"]).view(-1, 1)
        return {"pos": pos, "x": x, "heights": heights, "y": s["y"], "cls": cls, "class_weights": s["class_weights"]}

    a, b = program(), composed()
    torch.cuda.synchronize()
    print("  max |pos(program) - pos(composed)| = %.3e, x equal: %s" % (float((a["pos"] - b["pos"]).abs().max()), bool(torch.equal(a["x"], b["x"]))))
    res = measure({"program": program, "composed": composed}, reps, warmup)
    p = line("(i)", "SupervisedBatcher.batch", res["program"], kernels(program))
    c = line("(i)", "cloud_sample_batch + torch ops", res["composed"], kernels(composed))
    print("  program / composed (median dev): %.2f" % (p / c))


def leg_ii(reps, warmup):
    print("(ii) the three configured lists, 6 jobs (2 labelled, 2 weak, 2 strong)")
    kwargs = dict(TOOTH_VIEW_KWARGS)
    programs = {k: ViewProgram(v, kwargs) for k, v in CONFIGURED.items()}
    for m in (16000, 24000, 30000):
        rng = np.random.default_rng(m)
        raw = torch.from_numpy((rng.standard_normal((4, m, 3)) * np.array([.3, .2, .08])).astype(np.float32)).to(DEV)
        np.random.seed(m)
        torch.manual_seed(m)
        old, new = [], []
        for row, (src, kind) in enumerate(((0, "train"), (1, "train"), (2, "train_w"), (3, "train_w"), (2, "train_s"), (3, "train_s"))):
            p = draw_view_params(kind, kwargs)
            pick = {"PointCloudScaling": {"scale": p["s"]}, "PointCloudScaling_s": {"scale": p["s"]},
                    "PointCloudRotation_s": {"R": p["R"]}, "PointCloudTranslation_s": {"t": p["t"]}}
            old.append((src, row, p))
            new.append((src, row, programs[kind], [dict(pick.get(n, {})) for n in CONFIGURED[kind]]))
        hard = lambda: fixmatch_views(raw, old, kwargs["gravity_dim"], 6)      # noqa: E731
        prog = lambda: view_program_views(raw, new, 6)                          # noqa: E731
        a, b = hard(), prog()
        torch.cuda.synchronize()
        same = all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in ("pos", "x", "heights"))
        res = measure({"views": hard, "program": prog}, reps, warmup)
        print("  m = %d (%s), bits equal: %s" % (m, "registers" if m <= 24576 else "streaming", same))
        h = line("(ii)", "geot_fixmatch_views", res["views"], kernels(hard))
        p = line("(ii)", "geot_view_program", res["program"], kernels(prog))
        print("  program / views (median dev): %.2f" % (p / h))


def _as_lists(kind, p):
    """The s / R / t dict of one view as the ViewProgram.draw list of its configured list."""
    pick = {"PointCloudScaling": {"scale": p["s"]}, "PointCloudScaling_s": {"scale": p["s"]},
            "PointCloudRotation_s": {"R": p["R"]}, "PointCloudTranslation_s": {"t": p["t"]}}
    return [dict(pick.get(n, {})) for n in CONFIGURED_LISTS[kind]]


def leg_iii(reps, warmup):
    print("(iii) FixMatchBatcher.batch, B_l = B_u = 2, sel and params given; transforms=None against transforms=CONFIGURED_LISTS")
    lab, unl = scans(slice(0, 4)), scans(slice(4, 8))
    idx_l, idx_u = [0, 1], [2, 3]
    for m in (16000, 24000):
        none = FixMatchBatcher(lab, unl, m)
        lists = FixMatchBatcher(lab, unl, m, transforms=CONFIGURED_LISTS)
        np.random.seed(m)
        torch.manual_seed(m)
        sel, params = none.draw(idx_l, idx_u)
        as_lists = [_as_lists("train", p) for p in params[:2]] + [(_as_lists("train_w", w), _as_lists("train_s", s)) for w, s in params[2:]]
        hard = lambda: none.batch(idx_l, idx_u, sel_l=sel[:2], sel_u=sel[2:], params=params)         # noqa: E731
        prog = lambda: lists.batch(idx_l, idx_u, sel_l=sel[:2], sel_u=sel[2:], params=as_lists)     # noqa: E731
        a, b = hard(), prog()
        torch.cuda.synchronize()
        same = all(torch.equal(a[i][k].view(torch.int32), b[i][k].view(torch.int32)) for i in (0, 1) for k in a[i] if a[i][k].dtype == torch.float32)
        res = measure({"none": hard, "lists": prog}, reps, warmup)
        print("  m = %d, bits equal: %s" % (m, same))
        line("(iii)", "transforms=None", res["none"], kernels(hard))
        line("(iii)", "transforms=CONFIGURED_LISTS", res["lists"], kernels(prog))
        for what, h, p in (("dev", res["none"][0], res["lists"][0]), ("wall", res["none"][1], res["lists"][1])):
            bound = np.median(h) + np.percentile(h, 90) - np.percentile(h, 10)
            print("  gate %-4s lists median %7.3f ms <= None median + its p10 .. p90 spread %7.3f ms: %s"
                  % (what, np.median(p), bound, "holds" if np.median(p) <= bound else "FAILS"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--legs", default="i,ii")
    args = ap.parse_args()
    print("device: %s, torch %s, reps %d after %d warm-up, legs alternating" % (torch.cuda.get_device_name(0), torch.__version__, args.reps, args.warmup))
    if "i" in args.legs.split(","):
        leg_i(args.reps, args.warmup)
    if "ii" in args.legs.split(","):
        leg_ii(args.reps, args.warmup)
    if "iii" in args.legs.split(","):
        leg_iii(args.reps, args.warmup)


if __name__ == "__main__":
    main()
