"""What taking and restoring a training state costs (geot_amd/checkpoint.py), beside the iteration it interrupts.

    python tools/time_checkpoint.py [--reps 12] [--n 16000] [--out profiles/checkpoint_timing.txt]

One process, the configured 27.1 M-parameter FixMatch+NTM step (build_fixmatch, cfg fused_tail, grad_norm_clip 1,
step_per_update 2, ema_teacher, use_contrastive, the meters on: the widest state) behind a GraphedFixMatchStep with both
graphs captured:

    state_dict()        the copies on the current stream: device time between two events, and the host time of the call
                        (it does not synchronise: the host returns while the copies run)
    load_state_dict()   of that state (device tensors) into the same wrapper: the same two figures
    save() / load()     checkpoint.save to a file in a temporary directory and checkpoint.load back: wall time, synchronised
                        (the file is written from and read to the host: this leg is the disk's and PCIe's, not the GPU's)
    iteration           one replayed iteration, windows of 10 with look-ahead, per iteration

No threshold: the figures are what they are, and go into the README as measured.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_contrast import event_ms, fixmatch_batches      # noqa: E402

CFG = dict(fused_tail=True, grad_norm_clip=1.0, step_per_update=2, ema_teacher=True, use_contrastive=True)


def both(run, reps, warmup=2):
    """run() -> {device_us, host_us}: medians (p10, p90) of the device time between two events around the call and of the
    host time the call takes to return."""
    dev_us, host_us = [], []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        run()
        t1 = time.perf_counter()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            dev_us.append(a.elapsed_time(b) * 1e3)
            host_us.append((t1 - t0) * 1e6)
    return {"device_us": spread(dev_us), "host_us": spread(host_us)}


def spread(values):
    p10, med, p90 = np.percentile(values, [10, 50, 90])
    return {"median": round(float(med), 1), "p10": round(float(p10), 1), "p90": round(float(p90), 1)}


def state_bytes(obj):
    if torch.is_tensor(obj):
        return obj.numel() * obj.element_size()
    if isinstance(obj, dict):
        return sum(state_bytes(v) for v in obj.values())
    if isinstance(obj, (list, tuple)):
        return sum(state_bytes(v) for v in obj)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--n", type=int, default=16000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_checkpoint: needs a GPU (a timing taken anywhere else says nothing)")
    from geot_amd import checkpoint as ck, graph_step as gs, train_step as ts
    dev = torch.device("cuda:0")
    batches = fixmatch_batches(args.n, dev)
    for _, data_u in batches:          # (the meters read the unlabelled batch's ground truth)
        data_u["y"] = torch.zeros(data_u["pos_w"].shape[:2], dtype=torch.long, device=dev)
    torch.manual_seed(1609)
    step = ts.build_fixmatch(dev, cfg=dict(ts.NTM_CFG, **CFG), use_ddp=False, meters=True)
    graphed = gs.GraphedFixMatchStep(step, warmup=2)
    turn = [0]

    def iterate():
        cur, nxt = batches[turn[0] % 2], batches[(turn[0] + 1) % 2]
        turn[0] += 1
        graphed(cur[0], cur[1], next_batches=nxt)
    for _ in range(6):
        iterate()
    torch.cuda.synchronize()
    assert graphed.captured, sorted(graphed.graphs)
    captured = sorted(graphed.graphs)
    state = graphed.state_dict()
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "points per cloud": args.n, "cfg": CFG,
           "parameters": int(sum(p.numel() for p in step.model.parameters())),
           "state tensors": sum(1 for v in flatten(state) if torch.is_tensor(v)), "state MB": round(state_bytes(state) / 1e6, 1)}
    res["state_dict()"] = both(graphed.state_dict, args.reps)
    res["load_state_dict()"] = both(lambda: graphed.load_state_dict(state), args.reps)
    with tempfile.TemporaryDirectory() as work:
        path = os.path.join(work, "ckpt.pt")
        walls = {"save()": [], "load()": []}
        for i in range(1 + min(args.reps, 5)):
            for name, run in (("save()", lambda: ck.save(path, graphed, rng_device=dev)), ("load()", lambda: ck.load(path, graphed))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize()
                if i:
                    walls[name].append((time.perf_counter() - t0) * 1e3)
        res["file MB"] = round(os.path.getsize(path) / 1e6, 1)
    for name, values in walls.items():
        res[name] = {"wall_ms": spread(values)}
    times = []
    for i in range(2 + args.reps):
        t = event_ms(iterate, 10)
        if i >= 2:
            times.append(t * 1e3)
    res["iteration"] = {"device_us": spread(times)}
    assert sorted(graphed.graphs) == captured          # the loads captured nothing anew
    it = res["iteration"]["device_us"]["median"]
    lines = [
        "state_dict(): %.0f us of device time, %.0f us of host time (%d tensors, %.1f MB)"
        % (res["state_dict()"]["device_us"]["median"], res["state_dict()"]["host_us"]["median"], res["state tensors"], res["state MB"]),
        "load_state_dict() of that state into the same wrapper: %.0f us of device time, %.0f us of host time"
        % (res["load_state_dict()"]["device_us"]["median"], res["load_state_dict()"]["host_us"]["median"]),
        "checkpoint.save() to a file: %.0f ms of wall time; checkpoint.load() from it: %.0f ms (a %.1f MB file)"
        % (res["save()"]["wall_ms"]["median"], res["load()"]["wall_ms"]["median"], res["file MB"]),
        "one replayed iteration of that step (N = %d, 2 + 2 clouds): %.3f ms -- state_dict() is %.2f of it, load_state_dict() %.2f"
        % (args.n, it / 1e3, res["state_dict()"]["device_us"]["median"] / it, res["load_state_dict()"]["device_us"]["median"] / it)]
    head = ("Taking and restoring a training state (geot_amd/checkpoint.py) on the configured FixMatch+NTM step behind its\n"
            "captured graphs, beside one replayed iteration of the same process (tools/time_checkpoint.py; the legs are\n"
            "described there).  Medians; p10 and p90 below.\n")
    text = head + "\n" + "\n".join(lines) + "\n\n" + json.dumps(res, indent=1) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


def flatten(obj):
    if isinstance(obj, dict):
        return [x for v in obj.values() for x in flatten(v)]
    if isinstance(obj, (list, tuple)):
        return [x for v in obj for x in flatten(v)]
    return [obj]


if __name__ == "__main__":
    main()
