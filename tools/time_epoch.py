"""What an epoch costs under the training driver (geot_amd/fit.py), beside the same iterations from a loop written out by hand.

    python tools/time_epoch.py [--epochs 3] [--scans 32] [--out profiles/epoch_timing.txt]

Per point count (16 000 and 24 000), in one process: the configured 27.1 M-parameter FixMatch+NTM step (build_fixmatch, fused
tail, clipping, the meters on) behind a GraphedFixMatchStep, 2 + 2 clouds per iteration, drawn by a FixMatchBatcher with
DeviceDraws(seed, views=True) on a side stream from synthetic device-resident scan sets of about 1e5 vertices each.  Two
warm-up epochs of fit() capture the graphs; then, on the same wrapper,

    hand loop A     --epochs epochs of the loop of INTEGRATION.md "Training batches", written out below from calls that
                    existed before the driver: torch's samplers, batcher.batch / join, the wrapper's call, set_epoch, the
                    meters' reset / read, fill_ of the learning-rate tensors
    fit             the same number of epochs of fit() (prior=False, no validation, no files)
    hand loop B     the hand loop again

An epoch's time is wall time from its first batch to the return of meters.read(), which synchronises; per iteration it is
that time over the epoch's iterations, the median over the epochs.  The host time per iteration is the median distance
between two entries into the wrapper's call inside an epoch: the host runs ahead of the device, so that is what the loop
around the call and the call itself cost the host.  Last, the validation pass as fit() runs it (validate_scans, defaults)
over 4 scans, synchronised wall time.

No threshold: the claim to check is that fit's per-iteration time lies inside the spread of the hand loop's two timings.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from torch.utils.data import BatchSampler, RandomSampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_CFG = dict(fused_tail=True, grad_norm_clip=1.0)
CFG = dict(lr=1e-3, sched="multistep", decay_epochs=[220], decay_rate=0.1, warmup_epochs=0, sched_on_epoch=True, val_freq=1000,
           test_freq=1000, batch_size_l=2, batch_size_u=2, batch_size_val=2, num_classes=17, num_votes=0, supervised_epochs=0,
           run_name="timing")


def scan_set(count, first, dev, rng):
    from geot_amd.openpoints.dataset import DeviceScanSet
    from geot_amd.synth import make_cloud, region_labels
    sizes = [int(m) for m in rng.integers(90000, 110001, size=count)]
    units = [make_cloud(m, first + i)[0] for i, m in enumerate(sizes)]
    return DeviceScanSet([(u * np.float32(31.5)).astype(np.float32) for u in units],
                         [(region_labels(u) % 17).astype(np.int32) for u in units], cls=[i % 2 for i in range(count)], device=dev)


class Stamped:
    """The wrapper with the host's clock read at every entry into its call."""

    def __init__(self, call):
        self.call, self.step, self.stamps = call, call.step, []

    def set_epoch(self, epoch):
        self.stamps.append(None)          # an epoch's start: no distance across it
        self.call.set_epoch(epoch)

    def __call__(self, *args, **kwargs):
        self.stamps.append(time.perf_counter())
        return self.call(*args, **kwargs)

    def host_ms(self):
        gaps = [(b - a) * 1e3 for a, b in zip(self.stamps, self.stamps[1:]) if a is not None and b is not None]
        self.stamps = []
        return float(np.median(gaps))


def hand_epochs(stamped, batcher, sizes, generator, first, count, lrs):
    """The loop by hand -> seconds per epoch."""
    n_l, n_u = sizes
    seconds = []
    for epoch in range(first, first + count):
        t0 = time.perf_counter()
        lab = list(BatchSampler(RandomSampler(range(n_l), generator=generator), 2, drop_last=True))
        unl = iter(BatchSampler(RandomSampler(range(n_u), generator=generator), 2, drop_last=True))
        unl = [next(unl) for _ in lab]
        stamped.set_epoch(epoch)
        stamped.step.meters.reset()
        cur = batcher.batch(lab[0], unl[0])
        batcher.join(*cur)
        for it in range(len(lab)):
            nxt = None
            if it + 1 < len(lab):
                nxt = batcher.batch(lab[it + 1], unl[it + 1])
                batcher.join(*nxt)
            stamped(cur[0], cur[1], next_batches=nxt) if nxt is not None else stamped(cur[0], cur[1])
            cur = nxt
        stamped.step.meters.read()
        for lr in lrs:
            lr.fill_(1e-3)
        seconds.append(time.perf_counter() - t0)
    return seconds


def measure(n, args, dev):
    from geot_amd import graph_step as gs, train_step as ts
    from geot_amd.fit import fit
    from geot_amd.openpoints.dataset import DeviceDraws, FixMatchBatcher
    from geot_amd.validation import validate_scans
    rng = np.random.default_rng(n)
    lab, unl, val = scan_set(args.scans, 0, dev, rng), scan_set(args.scans, 1000, dev, rng), scan_set(4, 2000, dev, rng)
    torch.manual_seed(1609)
    step = ts.build_fixmatch(dev, cfg=dict(ts.NTM_CFG, **STEP_CFG), use_ddp=False, meters=True)
    batcher = FixMatchBatcher(lab, unl, n, stream=torch.cuda.Stream(dev), draws=DeviceDraws(1609, views=True))
    stamped = Stamped(gs.GraphedFixMatchStep(step, warmup=2))
    g = torch.Generator().manual_seed(1609)
    cfg = dict(CFG, num_points=n)
    iters = args.scans // 2
    fit(stamped, batcher, dict(cfg, epochs=2), generator=g, log=lambda rec: None)          # the prior, the captures
    assert stamped.call.captured, sorted(stamped.call.graphs)
    captured = sorted(stamped.call.graphs)
    lrs = [group["lr"] for opt in step.optimizers() for group in opt.param_groups]
    stamped.stamps = []
    e = args.epochs
    hand_a = hand_epochs(stamped, batcher, (len(lab), len(unl)), g, 3, e, lrs)
    host_hand_a = stamped.host_ms()
    records = fit(stamped, batcher, dict(cfg, start_epoch=3 + e, epochs=2 + 2 * e), generator=g, prior=False,
                  log=lambda rec: None)["records"]
    host_fit = stamped.host_ms()
    hand_b = hand_epochs(stamped, batcher, (len(lab), len(unl)), g, 3 + 2 * e, e, lrs)
    host_hand_b = stamped.host_ms()
    assert sorted(stamped.call.graphs) == captured          # nothing was captured anew
    per_it = lambda secs: float(np.median(secs)) / iters * 1e3      # noqa: E731
    fit_secs = [r["seconds"] for r in records]
    walls = []
    for i in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        validate_scans(step.model, val, dict(cfg, epoch=0, epochs=0), batch_size=2)
        torch.cuda.synchronize()
        if i:
            walls.append((time.perf_counter() - t0) * 1e3)
    return {"points per cloud": n, "iterations per epoch": iters, "epochs timed": e,
            "fit ms per iteration": round(per_it(fit_secs), 3), "fit clouds per s": round(4 * iters / float(np.median(fit_secs)), 1),
            "hand loop A ms per iteration": round(per_it(hand_a), 3), "hand loop B ms per iteration": round(per_it(hand_b), 3),
            "host ms per iteration": {"fit": round(host_fit, 3), "hand loop A": round(host_hand_a, 3), "hand loop B": round(host_hand_b, 3)},
            "epoch seconds": {"fit": [round(s, 4) for s in fit_secs], "hand loop A": [round(s, 4) for s in hand_a],
                              "hand loop B": [round(s, 4) for s in hand_b]},
            "validation pass ms (4 scans)": round(float(np.median(walls)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--scans", type=int, default=32)
    ap.add_argument("--points", type=int, nargs="+", default=[16000, 24000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epoch_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_epoch: needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    results, lines = [], []
    for n in args.points:
        r = measure(n, args, dev)
        results.append(r)
        a, b, f = r["hand loop A ms per iteration"], r["hand loop B ms per iteration"], r["fit ms per iteration"]
        lo, hi = min(a, b), max(a, b)
        where = "inside their spread" if lo <= f <= hi else "%.3f ms %s it" % ((f - hi, "above") if f > hi else (lo - f, "below"))
        host = r["host ms per iteration"]
        lines.append("N = %d, 2 + 2 clouds, %d iterations per epoch: fit %.3f ms per iteration (%.1f clouds/s); the hand-written "
                     "loop %.3f and %.3f ms -- fit is %s; host time per iteration: fit %.3f ms, the loop %.3f and %.3f ms; "
                     "validation pass over 4 scans: %.1f ms"
                     % (n, r["iterations per epoch"], f, r["fit clouds per s"], a, b, where, host["fit"], host["hand loop A"],
                        host["hand loop B"], r["validation pass ms (4 scans)"]))
    head = ("An epoch under fit() (geot_amd/fit.py) beside the same iterations from the loop written out by hand, timed twice, on\n"
            "one replayed FixMatch+NTM step in one process (tools/time_epoch.py; the legs are described there).  Medians over\n"
            "the timed epochs; every epoch's seconds below.\n")
    text = head + "\n" + "\n".join(lines) + "\n\n" + json.dumps({"device": torch.cuda.get_device_name(0), "cfg": STEP_CFG,
                                                                  "runs": results}, indent=1) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
