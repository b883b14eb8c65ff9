"""Device time of geot_pseudo_refine (csrc/pseudo_refine.hip) at the FixMatch step's sizes, beside the composite it replaces.

    python tools/time_pseudo_refine.py [--reps 20] [--out profiles/pseudo_refine_timing.txt] [--no-step]

B = 2 clouds of N = 16 000 and 24 000 points, C = 17, n = 4, k = 1 (cfg pseudo_refine_size / pseudo_refine_neighbors at their
defaults), th = 0.9.  The probabilities are the soft-max of unit noise plus 6 on the class of nine coherent regions
(geot_amd.synth.region_labels).  One process, every pair of legs alternating after warm-up, device events around windows of
calls (a single call is tens of microseconds: a window of one would time the clock):
    kernel     the launch alone, in both forms of sharing the classes out (GEOT_PSEUDO_REFINE_IMPL=point|split), on a
               neighbour table computed before; 200 launches per window
    call       pseudo_refine_mask(pred, th, pos) against the composite pseudo_label_refine(pred, th, pos) it replaces, the
               neighbour search (pointops.knn) included on both sides; 20 calls per window.  The masks must be equal.  The
               kernels of one call of each are counted with torch.profiler, and the peak of the allocator above its level
               before the call is read for both: the composite's (B, C, N, n) gather, its n copies and the stack
    iteration  GraphedFixMatchStep on the configured model (bench.py's fixmatch workload: 2 labelled + 2 unlabelled clouds,
               two alternating batches with look-ahead), cfg pseudo_refine off and "max" at the cfg's default threshold 0.0
               (a freshly initialised model is confident nowhere; the launches do not depend on what is kept): replayed
               iterations, 10 per window
The kernel's own device time per form is read from torch.profiler's records of one launch as well.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geot_amd.synth import make_batch, region_labels  # noqa: E402
from geot_amd.utils import pseudo_mask as pm  # noqa: E402

B, C, SIZE, K, TH = 2, 17, 4, 1, 0.9


def event_ms(run, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        run()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def alternate(legs, calls, warmup, reps):
    """{name: run} -> {name: {median_us, p10_us, p90_us}} per call, the legs taking turns window by window."""
    times = {k: [] for k in legs}
    for i in range(warmup + reps):
        for k, run in legs.items():
            t = event_ms(run, calls)
            if i >= warmup:
                times[k].append(t * 1e3)
    out = {}
    for k, ts in times.items():
        p10, med, p90 = np.percentile(ts, [10, 50, 90])
        out[k] = {"median_us": round(float(med), 2), "p10_us": round(float(p10), 2), "p90_us": round(float(p90), 2)}
    return out


def kernel_count(run):
    """Kernels one call launches, from torch.profiler's device records."""
    from torch.profiler import ProfilerActivity, profile
    try:
        run()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            run()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as e:      # noqa: BLE001 -- a convenience: the event timings stand without it
        return "unavailable: %s" % str(e)[:120]


def kernel_device_us(run):
    """Device time of the geot_pseudo_refine kernel in one call, from torch.profiler's device records."""
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            run()
            torch.cuda.synchronize()
        ts = [float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0)) for e in prof.key_averages()
              if "pseudo_refine_kernel" in e.key]
        return round(sum(ts), 2) if ts else "no kernel record"
    except Exception as e:      # noqa: BLE001
        return "unavailable: %s" % str(e)[:120]


def peak_bytes(run):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = run()
    torch.cuda.synchronize()
    del out
    return int(torch.cuda.max_memory_allocated() - base)


def inputs(n, dev):
    pos_np, _ = make_batch(B, n, start_index=10_000)
    rng = np.random.default_rng(n)
    logits = rng.standard_normal((B, C, n)).astype(np.float32)
    region = region_labels(pos_np, 9)
    np.put_along_axis(logits, region[:, None, :], np.take_along_axis(logits, region[:, None, :], 1) + np.float32(6.0), 1)
    return torch.softmax(torch.from_numpy(logits).to(dev), dim=1).contiguous(), torch.from_numpy(pos_np).to(dev)


def fixmatch_batches(n, dev):
    out = []
    for seed in (0, 100_003):
        xl, xu = make_batch(B, n, start_index=seed)[0], make_batch(B, n, start_index=seed + 10_000)[0]
        lab, unl = torch.from_numpy(xl).to(dev), torch.from_numpy(xu).to(dev)
        strong = (unl * 1.04).contiguous()
        z = torch.zeros(B, 1, dtype=torch.long, device=dev)
        out.append(({"pos": lab, "x": lab.transpose(1, 2).contiguous(), "cls": z, "y": torch.from_numpy(region_labels(xl)).to(dev)},
                    {"pos_w": unl, "x_w": unl.transpose(1, 2).contiguous(), "cls_w": z, "pos_s": strong,
                     "x_s": strong.transpose(1, 2).contiguous(), "cls_s": z, "raw_pos": unl}))
    return out


def iteration_legs(n, dev):
    from geot_amd import graph_step as gs, train_step as ts
    batches = fixmatch_batches(n, dev)
    legs, kept = {}, {}
    for name, refine in (("off", False), ("max", "max")):
        torch.manual_seed(1609)
        step = ts.build_fixmatch(dev, cfg=dict(ts.NTM_CFG, pseudo_refine=refine), use_ddp=False)
        graphed = gs.GraphedFixMatchStep(step, warmup=2)
        turn = [0]

        def run(graphed=graphed, turn=turn, name=name):
            cur, nxt = batches[turn[0] % 2], batches[(turn[0] + 1) % 2]
            turn[0] += 1
            out = graphed(cur[0], cur[1], next_batches=nxt)
            kept[name] = out.get("kept")
        for _ in range(6):
            run()
        torch.cuda.synchronize()
        assert graphed.captured, sorted(graphed.graphs)
        legs["iteration, pseudo_refine " + name] = run
    return legs, kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="skip the replayed FixMatch iteration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pseudo_refine_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_pseudo_refine: needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "B": B, "C": C, "n": SIZE, "k": K, "th": TH, "reps": args.reps}
    lines = []
    for n in (16000, 24000):
        pred, pos = inputs(n, dev)
        nbr = pm.neighbours(pos, SIZE)

        def kernel(form):
            def run():
                os.environ["GEOT_PSEUDO_REFINE_IMPL"] = form            # the library reads it at every call
                pm.pseudo_refine_mask(pred, TH, None, SIZE, K, nbr=nbr)
            return run
        leg = {"kernel": alternate({"point": kernel("point"), "split": kernel("split")}, 200, args.warmup, args.reps)}
        leg["kernel"]["device time of one launch, us (torch.profiler)"] = {f: kernel_device_us(kernel(f)) for f in ("point", "split")}
        os.environ.pop("GEOT_PSEUDO_REFINE_IMPL", None)
        fused = lambda: pm.pseudo_refine_mask(pred, TH, pos, SIZE, K)      # noqa: E731
        composite = lambda: pm.pseudo_label_refine(pred, TH, pos, SIZE, K)  # noqa: E731
        leg["call"] = alternate({"pseudo_refine_mask": fused, "composite pseudo_label_refine": composite}, 20, args.warmup, args.reps)
        keep, want = fused(), composite()
        leg["mask"] = {"kept": int(keep.sum()), "of": keep.numel(), "differ from the composite": int((keep.bool() != want).sum()),
                       "differ from the unrefined threshold mask": int((want != pred.max(1)[0].ge(TH)).sum())}
        leg["kernels of one call"] = {"pseudo_refine_mask": kernel_count(fused), "composite": kernel_count(composite),
                                      "neighbours alone": kernel_count(lambda: pm.neighbours(pos, SIZE))}
        leg["peak bytes above the level before the call"] = {
            "pseudo_refine_mask": peak_bytes(fused), "composite": peak_bytes(composite),
            "neighbours alone": peak_bytes(lambda: pm.neighbours(pos, SIZE)), "(B, C, N, n) fp32": B * C * n * SIZE * 4}
        c, k = leg["call"], leg["kernel"]
        lines.append("N = %d: kernel %.1f us (split) / %.1f us (point); pseudo_refine_mask %.1f us against the composite's %.1f us "
                     "per call with the neighbour search on both sides, %s against %s kernels, %d masks differ" % (
                         n, k["split"]["median_us"], k["point"]["median_us"], c["pseudo_refine_mask"]["median_us"],
                         c["composite pseudo_label_refine"]["median_us"], leg["kernels of one call"]["pseudo_refine_mask"],
                         leg["kernels of one call"]["composite"], leg["mask"]["differ from the composite"]))
        if not args.no_step:
            legs, kept = iteration_legs(n, dev)
            leg["iteration"] = alternate(legs, 10, args.warmup, args.reps)
            leg["iteration"]["kept"] = int(kept["max"])
            it = leg["iteration"]
            lines.append("N = %d: replayed FixMatch iteration %.3f ms with pseudo_refine off, %.3f ms with \"max\"" % (
                n, it["iteration, pseudo_refine off"]["median_us"] / 1e3, it["iteration, pseudo_refine max"]["median_us"] / 1e3))
            del legs
            torch.cuda.empty_cache()
        res["N = %d" % n] = leg
    head = ("geot_pseudo_refine (csrc/pseudo_refine.hip) at B = 2, C = 17, n = 4, k = 1, beside the composite pseudo_label_refine\n"
            "of geot_amd/utils/pseudo_mask.py (tools/time_pseudo_refine.py; the legs are described there).  One process, the legs\n"
            "of a pair alternating after warm-up, device time between events around windows of calls, per call.\n\n"
            "The kernels as compiled for gfx950 (-Rpass-analysis=kernel-resource-usage of the cross-compile), none with scratch,\n"
            "the <k list, ids in registers> instance of n = 4, k = 1: point 28 VGPRs, no LDS; split 30 VGPRs, 1 536 B LDS.\n")
    text = head + "\n" + "\n".join(lines) + "\n\n" + json.dumps(res, indent=1) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
