"""The batchers' vertex sample on the host and on the device (geot_sample_draw), timed.  Report only: nothing here is a gate.

    python tools/time_sample_draw.py [--reps 60] [--warmup 8]

One FixMatch batch of 8 labelled + 8 unlabelled synthetic scans of 120 000 vertices, m = 24 000, the configured view lists:

    host    FixMatchBatcher.batch(idx_l, idx_u)                         np.random.choice per item (the default)
    device  FixMatchBatcher.batch(idx_l, idx_u, draws=DeviceDraws(..))  one geot_sample_draw launch

Per repetition, after a device synchronise: `host` = the wall time of the call alone, until batch() returns (what the
launching thread pays; the kernels it queued may still run), `wall` = the wall time until the device has finished the batch
as well, `dev` = the time between two events recorded on the stream around the call.  The two legs alternate after warm-up.
Medians with the spread p10 .. p90.

The kernel's own time: CHAIN launches of geot_sample_draw (16 slots x 24 000) queued back to back between two events, the
elapsed time divided by CHAIN -- a single launch between two events would measure the launch path as much as the kernel.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geot_amd.openpoints.dataset import DeviceDraws, DeviceScanSet, FixMatchBatcher, sample_draw  # noqa: E402

DEV = torch.device("cuda:0")
B, M, VERTICES, CHAIN = 8, 24000, 120000, 20


def scans(seed):
    rng = np.random.default_rng(seed)
    pts = [(rng.standard_normal((VERTICES, 3)) * np.array([30, 20, 8]) + np.array([250, -400, 120])).astype(np.float32) for _ in range(B)]
    return DeviceScanSet(pts, [rng.integers(0, 17, VERTICES).astype(np.int32) for _ in range(B)], device=DEV)


def quantiles(v):
    v = np.array(v)
    return float(np.median(v)), float(np.percentile(v, 10)), float(np.percentile(v, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=8)
    args = ap.parse_args()
    print("device: %s, torch %s, reps %d after %d warm-up, legs alternating" % (torch.cuda.get_device_name(0), torch.__version__, args.reps, args.warmup))
    print("FixMatchBatcher.batch: %d + %d scans of %d vertices, m = %d" % (B, B, VERTICES, M))
    batcher = FixMatchBatcher(scans(1), scans(2), M)
    draws = DeviceDraws(0x1234567)
    idx = list(range(B))
    np.random.seed(1)
    torch.manual_seed(1)
    legs = {"host   (np.random.choice per item)": lambda: batcher.batch(idx, idx),
            "device (geot_sample_draw)": lambda: batcher.batch(idx, idx, draws=draws)}
    res = {k: ([], [], []) for k in legs}
    for r in range(args.warmup + args.reps):
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
            if r >= args.warmup:
                res[name][0].append((t1 - t0) * 1e3)
                res[name][1].append((t2 - t0) * 1e3)
                res[name][2].append(a.elapsed_time(b))
    med = {}
    for name, (host, wall, dev) in res.items():
        print("  %-36s host %7.3f ms (p10 %7.3f .. p90 %7.3f)   wall %7.3f ms (p10 %7.3f .. p90 %7.3f)   dev %7.3f ms (p10 %7.3f .. p90 %7.3f)"
              % ((name,) + quantiles(host) + quantiles(wall) + quantiles(dev)))
        med[name] = quantiles(host)[0]
    names = list(legs)
    print("  host time of batch(), device / host draws (medians): %.3f" % (med[names[1]] / med[names[0]]))

    ids = torch.tensor(idx + [B + i for i in idx], dtype=torch.int64, device=DEV)
    chain = []
    for r in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(CHAIN):
            sample_draw(batcher.scans, ids, M, draws.seed, r * CHAIN + k)
        b.record()
        torch.cuda.synchronize()
        if r >= args.warmup:
            chain.append(a.elapsed_time(b) / CHAIN * 1e3)
    print("geot_sample_draw, %d slots x %d (events around %d launches back to back, per launch): %.1f us (p10 %.1f .. p90 %.1f)"
          % ((2 * B, M, CHAIN) + quantiles(chain)))


if __name__ == "__main__":
    main()
