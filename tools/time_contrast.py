"""Device time of the fused teacher-student contrastive loss (csrc/contrast.hip, geot_amd/utils/cluster_contrastloss.py)
at the FixMatch step's sizes, beside the closed form written with torch ops, and of the replayed FixMatch iteration with
cfg use_contrastive off and on.

    python tools/time_contrast.py [--reps 20] [--out profiles/contrast_timing.txt] [--no-step] [--parent TREE]

B = 2 clouds of P = 16 000 and 24 000 points, D = 128 channels read channel-first, sample_nums = 1024 (bank 4096), th = 0.9,
about half the points over the threshold.  One process, the legs of a pair alternating after warm-up, device events around
windows of calls:
    call       forward + backward + enqueue.  fused: nativeContrastLoss_t in device mode (no synchronisation, ten
               launches).  torch: the same function in torch ops, in this file's own text (closed_form below): nonzero per
               cloud, a device randperm, the A selected rows normalised, the (A, A) and (A, 4S) matrices, autograd, the bank
               write behind int(pointer) -- two host synchronisations per call, so its time is what an eager loop pays.
               Kernels and their device time per call are read from torch.profiler, the allocator's peak above its level
               before the call for both.
    iteration  GraphedFixMatchStep on the configured model (bench.py's fixmatch workload: 2 labelled + 2 unlabelled clouds,
               two alternating batches with look-ahead), cfg use_contrastive off and on, alternating, at cur_threshold 0.9
               and cfg threshold 0.0; then "off" again in a child process of its own (the spread between the two "off"
               figures is the run-to-run spread a difference has to exceed; a third step object in THIS process measured
               5 ms slower at P = 24 000 than the first, the same code: presumably its streams share a hardware queue).
               A freshly initialised model is confident nowhere, so the teacher's last head layer is scaled (x 8) until
               points pass 0.9; the anchors of the last iteration are reported.
    parent     --parent TREE: a built checkout of the parent commit.  Its replayed iteration (the same batches, seeds and
               windows, the "off" leg alone) is measured by this file in a child process before and after the legs above.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, D, S, TH = 2, 128, 1024, 0.9
TAU, TAU_B = 0.1, 1.0


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


def kernels_of(run, only=None):
    """(kernels one call launches, their summed device time in us[, of those whose name holds `only`]) from torch.profiler."""
    from torch.profiler import ProfilerActivity, profile
    try:
        run()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            run()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        dur = lambda e: float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0) or 0.0)      # noqa: E731
        out = {"kernels": len(ev), "device_us": round(sum(dur(e) for e in ev), 1)}
        if only:
            per = {}
            for e in ev:
                if only in e.name:
                    name = e.name.split("(")[0].split("<")[0].split("::")[-1]
                    per[name] = round(per.get(name, 0.0) + dur(e), 1)
            out["per kernel us"] = per
        return out
    except Exception as e:      # noqa: BLE001 -- a convenience: the event timings stand without it
        return "unavailable: %s" % str(e)[:120]


def peak_bytes(run):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    run()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def closed_form(feat_s, score, feat_t, bank, ptr):
    """Steps 1-5 of geot_amd/utils/cluster_contrastloss.py's docstring with torch ops, features (B, D, P) channel-first."""
    import torch.nn.functional as F
    xs, ts = [], []
    for b in range(feat_s.shape[0]):
        idx = (score[b] >= TH).nonzero(as_tuple=False).squeeze(1)
        idx = idx[torch.randperm(idx.shape[0], device=idx.device)[:S]]
        xs.append(feat_s[b].index_select(1, idx).t())
        ts.append(feat_t[b].index_select(1, idx).t())
    x, t = F.normalize(torch.cat(xs), dim=1), F.normalize(torch.cat(ts), dim=1)
    a = x.shape[0]
    u, v = x @ t.t() / TAU, x @ bank.t() / TAU
    u = u - u.max(1, keepdim=True)[0].detach()
    v = v - v.max(1, keepdim=True)[0].detach()
    z = torch.exp(u).sum(1) + torch.exp(v).sum(1)
    loss = (-(TAU / TAU_B) * (torch.diagonal(u) - torch.log(z))).mean()
    loss.backward()
    with torch.no_grad():
        cnt = min(a, S)
        rows = F.normalize(t[torch.randperm(a, device=t.device)[:cnt]], dim=1)
        at = int(ptr)
        if at + cnt > bank.shape[0]:
            bank[-cnt:] = rows
            ptr.zero_()
        else:
            bank[at:at + cnt] = rows
            ptr.copy_((ptr + cnt) % bank.shape[0])
    return loss


def call_legs(p, dev):
    from geot_amd.openpoints.dataset.sample_draw import DeviceDraws
    from geot_amd.utils.cluster_contrastloss import nativeContrastLoss_t
    g = torch.Generator(device="cpu").manual_seed(p)
    feat_s = torch.randn((B, D, p), generator=g).to(dev).requires_grad_(True)
    feat_t = (0.5 * feat_s.detach() + torch.randn((B, D, p), generator=g).to(dev)).contiguous()
    score = (0.8 + 0.2 * torch.rand((B, p), generator=g)).to(dev)              # half of them at or above 0.9
    bank = torch.nn.functional.normalize(torch.randn((4 * S, D), generator=g), dim=1)
    mod = nativeContrastLoss_t(S, D, TH, dev, DeviceDraws(1), bank=bank)
    bank_t, ptr_t = bank.to(dev).clone(), torch.zeros(1, dtype=torch.long, device=dev)

    def fused():
        feat_s.grad = None
        mod(feat_s, score, feat_t, channels_first=True)[0].backward()

    def torch_form():
        feat_s.grad = None
        closed_form(feat_s, score, feat_t, bank_t, ptr_t)
    return fused, torch_form, mod, int((score >= TH).sum())


def fixmatch_batches(n, dev):
    from geot_amd.synth import make_batch, region_labels
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


def iteration_legs(n, dev, names):
    from geot_amd import graph_step as gs, train_step as ts
    batches = fixmatch_batches(n, dev)
    legs, last = {}, {}
    for name in names:
        torch.manual_seed(1609)
        extra = dict(use_contrastive=True) if name == "on" else {}
        step = ts.build_fixmatch(dev, cfg=dict(ts.NTM_CFG, **extra), use_ddp=False)
        with torch.no_grad():
            step.model_t.segmentor.seg_head[3].weight.mul_(8.0)
        graphed = gs.GraphedFixMatchStep(step, warmup=2)
        turn = [0]

        def run(graphed=graphed, turn=turn, name=name):
            cur, nxt = batches[turn[0] % 2], batches[(turn[0] + 1) % 2]
            turn[0] += 1
            last[name] = graphed(cur[0], cur[1], next_batches=nxt)
        for _ in range(6):
            run()
        torch.cuda.synchronize()
        assert graphed.captured, sorted(graphed.graphs)
        legs["iteration, use_contrastive " + name] = run
    return legs, last


def parent_iteration(tree, n, reps, warmup):
    """The parent checkout's replayed iteration, by this file in a child process whose package is the one under `tree`."""
    cmd = [sys.executable, os.path.abspath(__file__), "--tree", os.path.abspath(tree), "--child", str(n), "--reps", str(reps),
           "--warmup", str(warmup)]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrast_timing.txt"))
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    if not torch.cuda.is_available():
        sys.exit("time_contrast: needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    if args.child is not None:          # the parent's "off" leg alone
        legs, _ = iteration_legs(args.child, dev, ["off"])
        print(json.dumps(alternate(legs, 10, args.warmup, args.reps)["iteration, use_contrastive off"]))
        return
    res = {"device": torch.cuda.get_device_name(0), "B": B, "D": D, "S": S, "th": TH, "reps": args.reps}
    lines = []
    for p in (16000, 24000):
        fused, torch_form, mod, over = call_legs(p, dev)
        leg = {"points at or above the threshold": over, "of": B * p,
               "call": alternate({"fused": fused, "torch closed form": torch_form}, 10, args.warmup, args.reps)}
        leg["anchors"] = int(mod.anchors)
        leg["kernels of one call"] = {"fused": kernels_of(fused, "ct_"), "torch closed form": kernels_of(torch_form)}
        leg["peak bytes above the level before the call"] = {"fused": peak_bytes(fused), "torch closed form": peak_bytes(torch_form)}
        c, k = leg["call"], leg["kernels of one call"]
        lines.append("P = %d: fused %.1f us against the torch closed form's %.1f us per call (forward + backward + enqueue, "
                     "%d anchors); %s against %s kernels, %s against %s us of device time in them; peak %d against %d bytes" % (
                         p, c["fused"]["median_us"], c["torch closed form"]["median_us"], leg["anchors"],
                         k["fused"]["kernels"] if isinstance(k["fused"], dict) else "?",
                         k["torch closed form"]["kernels"] if isinstance(k["torch closed form"], dict) else "?",
                         k["fused"]["device_us"] if isinstance(k["fused"], dict) else "?",
                         k["torch closed form"]["device_us"] if isinstance(k["torch closed form"], dict) else "?",
                         leg["peak bytes above the level before the call"]["fused"],
                         leg["peak bytes above the level before the call"]["torch closed form"]))
        if not args.no_step:
            if args.parent:
                leg["parent commit, before"] = parent_iteration(args.parent, p, args.reps, args.warmup)
            legs, last = iteration_legs(p, dev, ["off", "on"])
            leg["iteration"] = alternate(legs, 10, args.warmup, args.reps)
            leg["iteration"]["anchors of the last iteration"] = int(last["on"]["anchors"])
            leg["iteration"]["contrast of the last iteration"] = float(last["on"]["contrast"])
            del legs
            torch.cuda.empty_cache()
            leg["iteration"]["iteration, use_contrastive off again"] = parent_iteration(ROOT, p, args.reps, args.warmup)
            if args.parent:
                leg["parent commit, after"] = parent_iteration(args.parent, p, args.reps, args.warmup)
            it = leg["iteration"]
            med = lambda v: "%.3f ms" % (v["median_us"] / 1e3) if isinstance(v, dict) else str(v)      # noqa: E731
            lines.append("P = %d: replayed FixMatch iteration %s with use_contrastive off, %s on (%d anchors), %s off again; "
                         "the parent commit %s before and %s after" % (
                             p, med(it["iteration, use_contrastive off"]), med(it["iteration, use_contrastive on"]),
                             it["anchors of the last iteration"], med(it["iteration, use_contrastive off again"]),
                             med(leg.get("parent commit, before", "not measured")),
                             med(leg.get("parent commit, after", "not measured"))))
        res["P = %d" % p] = leg
    head = ("The teacher-student contrastive loss (csrc/contrast.hip, geot_amd/utils/cluster_contrastloss.py) at B = 2, D = 128,\n"
            "S = 1024 (bank 4096), th = 0.9, channel-first features (tools/time_contrast.py; the legs are described there).  One\n"
            "process, the legs of a pair alternating after warm-up, device time between events around windows of 10 calls, per call.\n\n"
            "The streaming pass is the plain fp32 LDS-tiled form (ct_partial_kernel: 64 anchors x 32 keys per tile at D = 128,\n"
            "59 904 B of LDS, no scratch).  The alternative, the fp32 MFMA path of csrc/ntm_generic.hip, was not built: no time of\n"
            "it was taken, so which of the two is faster is open.\n")
    text = head + "\n" + "\n".join(lines) + "\n\n" + json.dumps(res, indent=1) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
