"""Device time of the gated tail behind cfg step_per_update (OptimTail(accumulate=k), csrc/optim_tail.hip: accumulate sweep, gated
finish, gated update sweep) call by call, beside the k = 1 tail and the same semantics in torch ops, and of the replayed
FixMatch iteration with step_per_update 1, 2 and 4.

    python tools/time_accumulate.py [--reps 12] [--out profiles/accumulate_timing.txt] [--no-step] [--parent TREE]

    tail       the configured model's full parameter set (build_fixmatch: two AdamW optimizers of two groups each) with random
               gradients, max_norm 1 and the teacher's EMA.  Device events around EVERY call of windows of k calls, k = 2 and 4:
               position 1 .. k-1 of a window is a call that only accumulates, position k the update; the k = 1 tail, the
               composite at k = 1 and the composite at k (torch._foreach_add_ into kept gradients; its update call) are timed
               the same way, the legs taking turns window by window after warm-up.  Every window starts behind a 2 ms spin
               kernel, so that the host has queued the window's calls when the device starts on them (the fused tails: 0.15 ms
               of host time per call; the composite's 0.6-1 ms per call outlasts the lead, its figures hold issue time).  Launches: the tails' own count, the
               composite's kernels under torch.profiler (the update call's for k > 1).
    iteration  GraphedFixMatchStep on the configured model (bench.py's fixmatch workload, two alternating batches with
               look-ahead) at 16 000 and 24 000 points with cfg fused_tail, grad_norm_clip 1 and step_per_update 1, 2, 4, every
               leg in a child process of its own (several step objects in one process can share a hardware queue:
               tools/time_optim_tail.py), per iteration over windows of 10 -- at k = 4 a window holds two or three updates.
    parent     --parent TREE: a built checkout of the parent commit; its replayed iteration under fused_tail + grad_norm_clip 1
               (the same batches, seeds and windows) before and after the legs above: what the k = 1 leg has to equal within
               the spread the two show.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_contrast import kernels_of               # noqa: E402
from time_optim_tail import child_iteration        # noqa: E402


LEAD_CYCLES = 4_000_000      # ~2 ms in front of every timed window


def tail_leg(dev, k):
    """(step, OptimTail) on a freshly built parameter set with random gradients; k None: built without the argument."""
    from geot_amd import train_step as ts
    from geot_amd.optim_tail import OptimTail
    torch.manual_seed(1609)
    step = ts.build_fixmatch(dev, use_ddp=False)
    kw = {} if k is None else {"accumulate": k}
    tail = OptimTail(step.optimizers(), clip_params=list(step.model.parameters()), max_norm=1.0, teacher=step.model_t,
                     student=step.model, ema_decay=0.99, **kw)
    g = torch.Generator(device=dev).manual_seed(7)
    grads = [(p, torch.randn(p.shape, generator=g, device=dev) * 1e-2) for p, _, _ in tail.params]

    def give():
        for p, gr in grads:
            p.grad = gr
    give()
    return step, tail, give


def per_position(legs, warmup, reps):
    """{name: (run, calls per window)} -> {name: [{median_us, p10_us, p90_us} per position of the window]}: device events
    around every call, the legs taking turns window by window."""
    times = {name: [[] for _ in range(calls)] for name, (_, calls) in legs.items()}
    for i in range(warmup + reps):
        for name, (run, calls) in legs.items():
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
            torch.cuda._sleep(LEAD_CYCLES)       # the host queues the window while the device waits: device time, not issue time
            evs[0].record()
            for j in range(calls):
                run()
                evs[j + 1].record()
            torch.cuda.synchronize()
            if i >= warmup:
                for j in range(calls):
                    times[name][j].append(evs[j].elapsed_time(evs[j + 1]) * 1e3)
    out = {}
    for name, per in times.items():
        out[name] = []
        for ts in per:
            p10, med, p90 = np.percentile(ts, [10, 50, 90])
            out[name].append({"median_us": round(float(med), 2), "p10_us": round(float(p10), 2), "p90_us": round(float(p90), 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="skip the replayed FixMatch iteration")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accumulate_timing.txt"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if not torch.cuda.is_available():
        sys.exit("time_accumulate: needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps}
    lines = []
    med = lambda v: "%.1f" % v["median_us"]      # noqa: E731
    for k in (2, 4):
        keep = {name: tail_leg(dev, kk) for name, kk in (("gated", k), ("k = 1", None), ("composite", None), ("composite, k", k))}

        def composite_k(tail=keep["composite, k"][1], give=keep["composite, k"][2]):
            give()                     # (the update call hands the sums back as .grad: every call starts from the gradients)
            tail.composite()
        legs = {"gated": (keep["gated"][1].step, k), "k = 1": (keep["k = 1"][1].step, k),
                "composite": (keep["composite"][1].composite, k), "composite, k": (composite_k, k)}
        for run, calls in legs.values():                 # state, tables and kept gradients exist; every window starts at 0
            for _ in range(calls):
                run()
        leg = {"call": per_position(legs, args.warmup, args.reps * 5)}
        gated, one = keep["gated"][1], keep["k = 1"][1]
        leg["parameters"] = int(sum(p.numel() for p, _, _ in gated.params))
        leg["records"] = len(gated._table)
        leg["accumulator MB"] = round(gated.accumulator.numel() * 4 / 2 ** 20, 1)
        # (every leg stands at the head of a window here: at k = 2 the profiled call, the second, is the update)
        leg["launches"] = {"gated": gated.launches, "k = 1": one.launches, "composite": kernels_of(keep["composite"][1].composite),
                           "composite, k, update call": kernels_of(composite_k) if k == 2 else "not counted"}
        c = leg["call"]
        inside = c["gated"][:-1]
        lines.append("k = %d: the gated tail takes %s us of device time on a call that only accumulates and %s us on the update "
                     "call, against %s us of the k = 1 tail and %s us of the composite per call (the composite at k: %s us "
                     "accumulating, %s us on its update call); %d launches on every call against %d (%d parameters in %d records, "
                     "a %.1f MB accumulator)" % (
                         k, " / ".join(med(v) for v in inside), med(c["gated"][-1]), med(c["k = 1"][-1]), med(c["composite"][-1]),
                         " / ".join(med(v) for v in c["composite, k"][:-1]), med(c["composite, k"][-1]), gated.launches,
                         one.launches, leg["parameters"], leg["records"], leg["accumulator MB"]))
        worst = max(v["median_us"] for v in inside)
        if worst > c["k = 1"][-1]["median_us"]:
            lines.append("        FINDING: a call that only accumulates (%.1f us) costs more than the whole k = 1 tail (%.1f us)"
                         % (worst, c["k = 1"][-1]["median_us"]))
        res["tail, k = %d" % k] = leg
        sys.stderr.write(lines[-1] + "\n")
        del keep, legs, gated, one
        torch.cuda.empty_cache()
    if not args.no_step:
        ms = lambda v: "%.3f ms" % (v["median_us"] / 1e3) if isinstance(v, dict) else str(v)      # noqa: E731
        base = dict(fused_tail=True, grad_norm_clip=1.0)
        for n in (16000, 24000):
            leg = {}
            if args.parent:
                leg["parent commit, before"] = child_iteration(args.parent, n, args.reps, args.warmup, base)
            for k in (1, 2, 4):
                leg["step_per_update %d" % k] = child_iteration(ROOT, n, args.reps, args.warmup, dict(base, step_per_update=k))
            if args.parent:
                leg["parent commit, after"] = child_iteration(args.parent, n, args.reps, args.warmup, base)
            lines.append("N = %d: replayed FixMatch iteration (fused_tail, grad_norm_clip 1) %s with step_per_update 1, %s with 2, "
                         "%s with 4; the parent commit %s before and %s after" % (
                             n, ms(leg["step_per_update 1"]), ms(leg["step_per_update 2"]), ms(leg["step_per_update 4"]),
                             ms(leg.get("parent commit, before", "not measured")), ms(leg.get("parent commit, after", "not measured"))))
            res["N = %d" % n] = leg
            sys.stderr.write(lines[-1] + "\n")
    head = ("The gated tail behind cfg step_per_update (csrc/optim_tail.hip, geot_amd/optim_tail.py) call by call, beside the\n"
            "k = 1 tail and the same semantics in torch ops (tools/time_accumulate.py; the legs are described there).  Device time\n"
            "between events around every call (tail) or around windows of 10 iterations, per iteration; medians, p10 and p90 below.\n")
    text = head + "\n" + "\n".join(lines) + "\n\n" + json.dumps(res, indent=1) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
