"""Device and host time of the fused tail of an iteration (csrc/optim_tail.hip, geot_amd/optim_tail.py: gradient clip + AdamW +
the teacher's EMA in two sweeps) beside the same semantics in torch ops (OptimTail.composite: clip_grad_norm_ +
optimizer.step() + torch._foreach_lerp_), and of the replayed FixMatch iteration with cfg fused_tail / ema_teacher off and on.

    python tools/time_optim_tail.py [--reps 20] [--out profiles/optim_tail_timing.txt] [--no-step] [--parent TREE]

    tail       the configured model's full parameter set (build_fixmatch: student, teacher, T_predictor; two AdamW optimizers of
               two groups each) with random gradients; variants clip (max_norm 1), EMA (decay 0.99) and both.  One process,
               fused and composite taking turns window by window after warm-up, device events around windows of 5 calls.
               Launches: the fused tail's own count, the composite's kernels under torch.profiler.  Host time: a host clock
               around 20 eager calls between two synchronisations, per call -- for the fused tail that includes the walk over
               the parameters and the rebuild of the gradient pointers in the record table.
    iteration  GraphedFixMatchStep on the configured model (bench.py's fixmatch workload: 2 labelled + 2 unlabelled clouds,
               two alternating batches with look-ahead) at 16 000 and 24 000 points: switches off, fused_tail, ema_teacher +
               fused_tail (the teacher's forward moves out of the look-ahead graph onto the critical path), alternating; then
               grad_norm_clip 1 with fused_tail off and on, alternating; then every one of these legs again in a child process
               of its own ("off" among them: the spread between the "off" figures is what a difference has to exceed).  Several
               step objects in one process can land two of a step's streams on one hardware queue, which costs that leg about
               5 ms at 24 000 points whatever its code (tools/time_contrast.py met the same): where a leg of the alternating
               group stands apart from its own-process figure, the own-process one is the leg's time.
    parent     --parent TREE: a built checkout of the parent commit; its replayed iteration (the same batches, seeds and
               windows) is measured by this file in a child process, before and after the legs above.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_contrast import alternate, fixmatch_batches, kernels_of      # noqa: E402


def tail_legs(dev, clip, ema):
    """(fused, composite, the fused OptimTail) on two separately built parameter sets with random gradients."""
    from geot_amd import train_step as ts
    from geot_amd.optim_tail import OptimTail
    legs = []
    for _ in range(2):
        torch.manual_seed(1609)
        step = ts.build_fixmatch(dev, use_ddp=False)
        tail = OptimTail(step.optimizers(), clip_params=list(step.model.parameters()) if clip else None,
                         max_norm=1.0 if clip else None, teacher=step.model_t if ema else None,
                         student=step.model if ema else None, ema_decay=0.99 if ema else None)
        g = torch.Generator(device=dev).manual_seed(7)
        for p, _, _ in tail.params:
            p.grad = torch.randn(p.shape, generator=g, device=dev) * 1e-2
        legs.append((step, tail))
    return legs[0][1].step, legs[1][1].composite, legs[0][1], legs


def host_us(run, calls=20):
    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        run()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return round((t1 - t0) / calls * 1e6, 1)


def iteration_legs(n, dev, cfgs):
    from geot_amd import graph_step as gs, train_step as ts
    batches = fixmatch_batches(n, dev)
    legs = {}
    for name, extra in cfgs.items():
        torch.manual_seed(1609)
        step = ts.build_fixmatch(dev, cfg=dict(ts.NTM_CFG, **extra), use_ddp=False)
        graphed = gs.GraphedFixMatchStep(step, warmup=2)
        turn = [0]

        def run(graphed=graphed, turn=turn):
            cur, nxt = batches[turn[0] % 2], batches[(turn[0] + 1) % 2]
            turn[0] += 1
            graphed(cur[0], cur[1], next_batches=nxt)
        for _ in range(6):
            run()
        torch.cuda.synchronize()
        assert graphed.captured, sorted(graphed.graphs)
        legs["iteration, " + name] = run
    return legs


def child_iteration(tree, n, reps, warmup, cfg=None):
    """The replayed iteration under cfg (default: every switch off), by this file in a child process whose package is the
    one under `tree`."""
    cmd = [sys.executable, os.path.abspath(__file__), "--tree", os.path.abspath(tree), "--child", str(n), "--reps", str(reps),
           "--warmup", str(warmup), "--child-cfg", json.dumps(cfg or {})]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=os.path.abspath(tree))
    if out.returncode != 0:
        return "failed: %s" % out.stderr[-300:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="skip the replayed FixMatch iteration")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-cfg", default="{}", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_tail_timing.txt"))
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    if not torch.cuda.is_available():
        sys.exit("time_optim_tail: needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    if args.child is not None:          # one leg alone: the parent's tree, or this one again
        legs = iteration_legs(args.child, dev, {"leg": json.loads(args.child_cfg)})
        print(json.dumps(alternate(legs, 10, args.warmup, args.reps)["iteration, leg"]))
        return
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps}
    lines = []
    for name, clip, ema in (("clip", True, False), ("EMA", False, True), ("clip + EMA", True, True)):
        fused, composite, tail, keep = tail_legs(dev, clip, ema)
        leg = {"call": alternate({"fused": fused, "composite": composite}, 5, args.warmup, args.reps)}
        fused()
        leg["parameters"] = int(sum(p.numel() for p, _, _ in tail.params))
        leg["records"] = len(tail._table)
        leg["launches"] = {"fused": tail.launches, "composite": kernels_of(composite)}
        leg["host us per eager call"] = {"fused": host_us(fused), "composite": host_us(composite)}
        c, k = leg["call"], leg["launches"]["composite"]
        lines.append("%s: fused %.1f us against the composite's %.1f us of device time per call (%d parameters in %d records); "
                     "%d launches against %s; host time per eager call %.1f against %.1f us" % (
                         name, c["fused"]["median_us"], c["composite"]["median_us"], leg["parameters"], leg["records"],
                         tail.launches, k["kernels"] if isinstance(k, dict) else "?",
                         leg["host us per eager call"]["fused"], leg["host us per eager call"]["composite"]))
        res["tail, " + name] = leg
        del fused, composite, tail, keep
        torch.cuda.empty_cache()
    if not args.no_step:
        med = lambda v: "%.3f ms" % (v["median_us"] / 1e3) if isinstance(v, dict) else str(v)      # noqa: E731
        for n in (16000, 24000):
            leg = {}
            if args.parent:
                leg["parent commit, before"] = child_iteration(args.parent, n, args.reps, args.warmup)
            groups = ({"off": {}, "fused_tail": dict(fused_tail=True),
                       "ema_teacher + fused_tail": dict(fused_tail=True, ema_teacher=True)},
                      {"clip 1, off": dict(grad_norm_clip=1.0), "clip 1, fused_tail": dict(grad_norm_clip=1.0, fused_tail=True)})
            for cfgs in groups:
                legs = iteration_legs(n, dev, cfgs)
                leg.update(alternate(legs, 10, args.warmup, args.reps))
                del legs
                torch.cuda.empty_cache()
            for cfgs in groups:
                for name, cfg in cfgs.items():
                    key = "iteration, off again" if name == "off" else "own process, " + name
                    leg[key] = child_iteration(ROOT, n, args.reps, args.warmup, cfg)
            if args.parent:
                leg["parent commit, after"] = child_iteration(args.parent, n, args.reps, args.warmup)
            lines.append("N = %d: replayed FixMatch iteration %s with the switches off, %s off again in its own process; the "
                         "parent commit %s before and %s after; fused_tail %s (own process %s); ema_teacher + fused_tail %s "
                         "(own process %s); with grad_norm_clip 1: %s off (own process %s), %s fused_tail (own process %s)" % (
                             n, med(leg["iteration, off"]), med(leg["iteration, off again"]),
                             med(leg.get("parent commit, before", "not measured")),
                             med(leg.get("parent commit, after", "not measured")), med(leg["iteration, fused_tail"]),
                             med(leg["own process, fused_tail"]), med(leg["iteration, ema_teacher + fused_tail"]),
                             med(leg["own process, ema_teacher + fused_tail"]), med(leg["iteration, clip 1, off"]),
                             med(leg["own process, clip 1, off"]), med(leg["iteration, clip 1, fused_tail"]),
                             med(leg["own process, clip 1, fused_tail"])))
            res["N = %d" % n] = leg
    head = ("The fused tail of an iteration (csrc/optim_tail.hip, geot_amd/optim_tail.py) beside the same semantics in torch ops\n"
            "(tools/time_optim_tail.py; the legs are described there).  Legs of a group alternate after warm-up in one process;\n"
            "device time between events around windows of calls, per call; medians, p10 and p90 over the windows below.\n")
    text = head + "\n" + "\n".join(lines) + "\n\n" + json.dumps(res, indent=1) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
