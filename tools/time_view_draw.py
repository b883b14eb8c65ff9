"""The transform lists' draws on the host and on the device (geot_view_draw), timed.  Report only: nothing here is a gate.

    python tools/time_view_draw.py [--reps 40] [--warmup 6]

Batches of 8 (supervised) or 8 + 8 (FixMatch) synthetic scans of 120 000 vertices at m = 16 000 and m = 24 000:

    SupervisedBatcher.batch, the default list (scaling, centring, jitter, chromatic drop)
    FixMatchBatcher.batch, the three configured lists

each with two legs that both draw the vertex sample on the device:

    rows   draws=DeviceDraws(seed)               the list's draws on the host: torch / numpy / random, pinned staging
    views  draws=DeviceDraws(seed, views=True)   one geot_view_draw launch, no host draw, no staging

Per repetition, after a device synchronise: `host` = the wall time of the call alone, until batch() returns (what the
launching thread pays), `wall` = until the device has finished the batch as well, `dev` = the time between two events
recorded on the stream around the call.  The legs alternate after warm-up.  Medians with the spread p10 .. p90.

The kernel's own time: CHAIN launches of geot_view_draw queued back to back between two events, divided by CHAIN.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geot_amd.openpoints.dataset import (DeviceDraws, DeviceScanSet, FixMatchBatcher, SupervisedBatcher,  # noqa: E402
                                         view_draw)

DEV = torch.device("cuda:0")
B, VERTICES, CHAIN = 8, 120000, 20


def scans(seed):
    rng = np.random.default_rng(seed)
    pts = [(rng.standard_normal((VERTICES, 3)) * np.array([30, 20, 8]) + np.array([250, -400, 120])).astype(np.float32) for _ in range(B)]
    return DeviceScanSet(pts, [rng.integers(0, 17, VERTICES).astype(np.int32) for _ in range(B)], device=DEV)


def quantiles(v):
    v = np.array(v)
    return float(np.median(v)), float(np.percentile(v, 10)), float(np.percentile(v, 90))


def time_legs(legs, reps, warmup):
    res = {k: ([], [], []) for k in legs}
    for r in range(warmup + reps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            t1 = time.perf_counter()
            b.record()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if r >= warmup:
                res[name][0].append((t1 - t0) * 1e3)
                res[name][1].append((t2 - t0) * 1e3)
                res[name][2].append(a.elapsed_time(b))
    med = []
    for name, (host, wall, dev) in res.items():
        print("  %-46s host %7.3f ms (p10 %7.3f .. p90 %7.3f)   wall %7.3f ms (p10 %7.3f .. p90 %7.3f)   dev %7.3f ms (p10 %7.3f .. p90 %7.3f)"
              % ((name,) + quantiles(host) + quantiles(wall) + quantiles(dev)))
        med.append(quantiles(host)[0])
    print("  host time of batch(), views / rows (medians): %.3f" % (med[1] / med[0]))


def time_kernel(layout, reps, warmup, what):
    chain = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(CHAIN):
            view_draw(layout, 0x1234567, r * CHAIN + k)
        b.record()
        torch.cuda.synchronize()
        if r >= warmup:
            chain.append(a.elapsed_time(b) / CHAIN * 1e3)
    print("  geot_view_draw, %s (events around %d launches back to back, per launch): %.1f us (p10 %.1f .. p90 %.1f)"
          % ((what, CHAIN) + quantiles(chain)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    args = ap.parse_args()
    print("device: %s, torch %s, reps %d after %d warm-up, legs alternating" % (torch.cuda.get_device_name(0), torch.__version__, args.reps, args.warmup))
    lab, unl = scans(1), scans(2)
    idx = list(range(B))
    np.random.seed(1)
    torch.manual_seed(1)
    for m in (16000, 24000):
        rows, views = DeviceDraws(0x1234567), DeviceDraws(0x1234567, views=True)
        sup = SupervisedBatcher(lab, m)
        print("SupervisedBatcher.batch: %d scans of %d vertices, m = %d, the default list" % (B, VERTICES, m))
        time_legs({"rows  (DeviceDraws(seed): host view draws)": lambda: sup.batch(idx, draws=rows),
                   "views (DeviceDraws(seed, views=True))": lambda: sup.batch(idx, draws=views)}, args.reps, args.warmup)
        time_kernel(sup._layout(B), args.reps, args.warmup, "%d jobs x %d points, one noise row each" % (B, m))
        fm = FixMatchBatcher(lab, unl, m)
        print("FixMatchBatcher.batch: %d + %d scans of %d vertices, m = %d, the configured lists" % (B, B, VERTICES, m))
        time_legs({"rows  (DeviceDraws(seed): host view draws)": lambda: fm.batch(idx, idx, draws=rows),
                   "views (DeviceDraws(seed, views=True))": lambda: fm.batch(idx, idx, draws=views)}, args.reps, args.warmup)
        time_kernel(fm._layout(B, B), args.reps, args.warmup, "%d jobs x %d points, scalars only" % (3 * B, m))


if __name__ == "__main__":
    main()
