"""Time the switchable criteria of the FixMatch+NTM loop on the GPU (results: profiles/criteria_timing.txt).

    python tools/time_criteria.py [--points 16000 24000] [--reps 200] [--iters 30] [--skip-iteration] [--out FILE]

Two measurements, at B = 2, C = 17 and each N:

1. every new criterion's forward + backward, the fused kernels (csrc/loss.hip) against the class's own torch composite (the
   path it takes when its guard fails), alternating the two in one process, device events around `reps` calls each, three
   rounds: median and spread;
2. the replayed FixMatch+NTM iteration (GraphedFixMatchStep, look-ahead on, the configured segmentor) under the default
   cfg and under each switch: device events around `iters` iterations after the graphs are captured, three rounds.

Needs a GPU: no fall-back.  Prints one line per measurement and a JSON summary at the end.
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, C = 2, 17
SWITCHES = {
    "default": {},
    "criterion=Weight_CELoss": dict(criterion="Weight_CELoss"),
    "criterion_u=Weight_CELoss_U": dict(criterion_u="Weight_CELoss_U"),
    "criterion_u=Poly1FocalLoss_U": dict(criterion_u="Poly1FocalLoss_U"),
    "criterion_u=Poly1FocalLoss_U_T": dict(criterion_u="Poly1FocalLoss_U_T"),
    "use_feat_loss": dict(use_feat_loss=True),
    "use_identity_loss": dict(use_identity_loss=True),
    "use_3d_loss=False": dict(use_3d_loss=False),
}


@contextlib.contextmanager
def composite():
    """The criteria's guards answer no: every class runs its torch composite."""
    from geot_amd.openpoints.loss import build as lb
    saved = lb._fused_ok, lb._wce_fused_ok
    lb._fused_ok = lb._wce_fused_ok = lambda *a, **k: False
    try:
        yield
    finally:
        lb._fused_ok, lb._wce_fused_ok = saved


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps * 1e3       # microseconds per call


def criteria_cases(n, dev):
    from geot_amd.openpoints.loss import build_criterion_from_cfg as build
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(B, C, n, generator=g) * 3).to(dev).requires_grad_(True)
    t = ((torch.rand(B, C, n, generator=g) * 3.75 + 0.25) * (torch.randint(0, 2, (B, C, n), generator=g) * 2 - 1)).to(dev)
    t.requires_grad_(True)
    lab = torch.randint(0, C, (B, n), generator=g).to(dev)
    conf = (torch.rand(B, n, generator=g) * 0.5 + 0.5).to(dev)
    cw = (torch.rand(B, C, generator=g) * 0.1 + 0.01).to(dev)
    mods = {k: build({"NAME": k}) for k in ("Weight_CELoss", "Weight_CELoss_U", "Poly1FocalLoss_U", "Poly1FocalLoss_U_T")}

    def fb(loss_fn):
        def run():
            x.grad = t.grad = None
            loss_fn().backward()
        return run
    return {"Weight_CELoss": fb(lambda: mods["Weight_CELoss"](x, lab, cw)),
            "Weight_CELoss_U": fb(lambda: mods["Weight_CELoss_U"](x, lab, cw, conf, thresh=0.7)),
            "Poly1FocalLoss_U": fb(lambda: mods["Poly1FocalLoss_U"](x, lab, conf, thresh=0.7)),
            "Poly1FocalLoss_U_T": fb(lambda: mods["Poly1FocalLoss_U_T"](x, lab, conf, None, t, thresh=0.7))}


def time_criteria(n, dev, reps, rounds=3):
    out = {}
    for name, fn in criteria_cases(n, dev).items():
        samples = {"fused": [], "composite": []}
        for _ in range(rounds + 1):                        # the first round warms both paths up and is dropped
            samples["fused"].append(timed(fn, reps))
            with composite():
                samples["composite"].append(timed(fn, reps))
        row = {}
        for k, v in samples.items():
            v = v[1:]
            row[k] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}
        row["no_slower"] = row["fused"]["median_us"] <= row["composite"]["median_us"]
        out[name] = row
        print("N=%5d %-20s fused %8.1f us [%.1f .. %.1f]   composite %8.1f us [%.1f .. %.1f]   %s" % (
            n, name, row["fused"]["median_us"], row["fused"]["min_us"], row["fused"]["max_us"], row["composite"]["median_us"],
            row["composite"]["min_us"], row["composite"]["max_us"], "fused no slower" if row["no_slower"] else "FUSED SLOWER"),
            flush=True)
    return out


def fixmatch_batches(n, dev):
    from geot_amd.synth import make_batch, region_labels
    out = []
    for k in range(2):
        xl, xu = make_batch(B, n, start_index=1000 * k)[0], make_batch(B, n, start_index=10_000 + 1000 * k)[0]
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
        lab, unl = T(xl), T(xu)
        strong = (unl * 1.04).contiguous()
        z = torch.zeros(B, 1, dtype=torch.long, device=dev)
        y = T(region_labels(xl))
        hist = torch.stack([torch.bincount(row, minlength=C)[:C] for row in y]).float() / n     # tooth_dataset's class_weights
        out.append(({"pos": lab, "x": lab.transpose(1, 2).contiguous(), "cls": z, "y": y, "class_weights": hist},
                    {"pos_w": unl, "x_w": unl.transpose(1, 2).contiguous(), "cls_w": z, "pos_s": strong,
                     "x_s": strong.transpose(1, 2).contiguous(), "cls_s": z, "raw_pos": unl}))
    return out


def time_iteration(n, dev, iters, rounds=3):
    from geot_amd import graph_step as gs, train_step as ts
    batches = fixmatch_batches(n, dev)
    out = {}
    for name, switches in SWITCHES.items():
        torch.manual_seed(1609)
        step = ts.build_fixmatch(dev, cfg=dict(ts.NTM_CFG, **switches), use_ddp=False)
        call = gs.GraphedFixMatchStep(step, warmup=2)
        turn = [0]

        def one():
            cur, nxt = batches[turn[0] % 2], batches[(turn[0] + 1) % 2]
            turn[0] += 1
            return call(cur[0], cur[1], next_batches=nxt)["loss"]
        for _ in range(6):
            loss = one()
        assert call.captured and torch.isfinite(loss), name
        v = [timed(one, iters) / 1e3 for _ in range(rounds)]
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
        print("N=%5d iteration %-32s %7.2f ms [%.2f .. %.2f]  nodes %s" % (
            n, name, out[name]["median_ms"], min(v), max(v), {k: sum(c.values()) for k, c in call.node_types.items()}), flush=True)
        del call, step
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[16000, 24000])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--skip-iteration", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_criteria.py measures on a GPU; none is visible")
    import geot_amd  # noqa: F401
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "B": B, "C": C, "criteria": {}, "iteration": {}}
    for n in args.points:
        result["criteria"][str(n)] = time_criteria(n, dev, args.reps)
    if not args.skip_iteration:
        for n in args.points:
            result["iteration"][str(n)] = time_iteration(n, dev, args.iters)
    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
