"""Time cfg.filter_outlier's anchors on the GPU (results: profiles/filter_outlier_timing.txt).

    python tools/time_filter_outlier.py [--reps 200] [--iters 30] [--skip-iteration] [--only-off] [--tree DIR] [--out FILE]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/time_filter_outlier.py --trace-run [--reps 50]
    python tools/time_filter_outlier.py --read-trace DIR/.../*_kernel_trace.csv [--reps 50]

At C = 17 and (B, N) = (2, 16 000), (2, 24 000), (8, 24 000), on a random soft-max (logits x 8) and on a saturated one (logits
x 60, half the points pushed to the background class: at least 40 % of class 0 exactly 1.0f, zeros and denormals elsewhere):

1. ntm.filtered_anchors (two launches, csrc/ntm_outlier.hip) against the torch composite ntm._filtered_anchor_rows on the same
   input, alternating the two in one process, device events around `reps` calls each, three rounds after a dropped warm-up
   round: median and spread; the nodes of each captured into a graph (the launch count) and the peak memory above the input;
2. the replayed FixMatch+NTM iteration (GraphedFixMatchStep, look-ahead on, the configured segmentor) with the switch off, on
   (fused) and on with the composite patched in: device events around `iters` iterations after capture, three rounds.
   --only-off --tree DIR measures the switch-off iteration of ANOTHER checkout (the parent commit) for the A/A comparison;
3. per-kernel times: --trace-run makes `reps` fused calls per shape and input in a fixed order and nothing else; run it under
   rocprofv3's kernel trace, in a run of its own, and hand the CSV to --read-trace, which splits the two kernels' dispatches
   back into the shapes by that order.

Needs a GPU: no fall-back.  Prints one line per measurement and a JSON summary at the end.
"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C, Q = 17, 0.97
SHAPES = [(2, 16000), (2, 24000), (8, 24000)]
KINDS = ("random", "saturated")
KERNELS = ("outlier_select_kernel", "outlier_anchor_kernel")


def make_eta(kind, b, n, dev):
    import torch
    g = torch.Generator().manual_seed(1000 * b + n)
    logits = torch.randn(b, C, n, generator=g)
    if kind == "saturated":
        logits[:, 0, :] = torch.where(torch.rand(b, n, generator=g) < 0.5, torch.full((b, n), 5.0), logits[:, 0, :])
        logits = logits * 60
    else:
        logits = logits * 8
    eta = torch.softmax(logits, dim=1).to(dev).contiguous()
    ones = float((eta[:, 0, :] == 1).float().mean())
    assert kind != "saturated" or ones >= 0.4, ones
    return eta, ones


def timed(fn, reps):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps * 1e3       # microseconds per call


def nodes_and_peak(fn, dev):
    """({"kernel": n, ...} of fn captured into a graph, peak bytes allocated above the baseline by one eager call)."""
    import torch
    from geot_amd import streams
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    try:
        with streams.capture(graph, dev):
            fn()
        kinds = streams.node_types(graph)
    except RuntimeError as e:       # a path that cannot be captured is a result, not a failure of the tool
        kinds = {"capture failed": str(e).splitlines()[0][:120]}
    del graph
    return kinds, peak


def time_calls(dev, reps, rounds=3):
    import torch
    from geot_amd import ntm
    out = {}
    for b, n in SHAPES:
        for kind in KINDS:
            eta, ones = make_eta(kind, b, n, dev)
            fns = {"fused": lambda: ntm.filtered_anchors(eta, Q), "composite": lambda: ntm._filtered_anchor_rows(eta, Q)}
            f, c = fns["fused"](), fns["composite"]()
            same = torch.equal(f[0], c[0]) and torch.equal(f[1], c[1])
            samples = {k: [] for k in fns}
            for _ in range(rounds + 1):                        # the first round warms both paths up and is dropped
                for k, fn in fns.items():
                    samples[k].append(timed(fn, reps))
            row = {"class0_exactly_one": ones, "same_class_T_and_v_star": same}
            for k, fn in fns.items():
                v = samples[k][1:]
                kinds, peak = nodes_and_peak(fn, dev)
                row[k] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "nodes": kinds,
                          "peak_bytes": peak}
            row["faster"] = row["fused"]["median_us"] < row["composite"]["median_us"]
            out["%dx%d %s" % (b, n, kind)] = row
            print("B=%d N=%5d %-9s (class 0 == 1.0f: %4.1f %%) fused %7.1f us [%.1f .. %.1f] %s %.2f MB   composite %7.1f us "
                  "[%.1f .. %.1f] %s %.2f MB   %s%s" % (
                      b, n, kind, 100 * ones, row["fused"]["median_us"], row["fused"]["min_us"], row["fused"]["max_us"],
                      row["fused"]["nodes"], row["fused"]["peak_bytes"] / 1e6, row["composite"]["median_us"],
                      row["composite"]["min_us"], row["composite"]["max_us"], row["composite"]["nodes"],
                      row["composite"]["peak_bytes"] / 1e6, "fused faster" if row["faster"] else "FUSED NOT FASTER",
                      "" if same else "   RESULTS DIFFER"), flush=True)
    return out


def fixmatch_batches(b, n, dev):
    import numpy as np
    import torch
    from geot_amd.synth import make_batch, region_labels
    out = []
    for k in range(2):
        xl, xu = make_batch(b, n, start_index=1000 * k)[0], make_batch(b, n, start_index=10_000 + 1000 * k)[0]
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
        lab, unl = T(xl), T(xu)
        strong = (unl * 1.04).contiguous()
        z = torch.zeros(b, 1, dtype=torch.long, device=dev)
        y = T(region_labels(xl))
        hist = torch.stack([torch.bincount(row, minlength=C)[:C] for row in y]).float() / n     # tooth_dataset's class_weights
        out.append(({"pos": lab, "x": lab.transpose(1, 2).contiguous(), "cls": z, "y": y, "class_weights": hist},
                    {"pos_w": unl, "x_w": unl.transpose(1, 2).contiguous(), "cls_w": z, "pos_s": strong,
                     "x_s": strong.transpose(1, 2).contiguous(), "cls_s": z, "raw_pos": unl}))
    return out


def time_iteration(n, dev, iters, only_off, rounds=3):
    import torch
    from geot_amd import graph_step as gs, ntm, train_step as ts
    batches = fixmatch_batches(2, n, dev)
    modes = ["off"] if only_off else ["off", "fused", "composite", "off", "fused", "composite"]     # each twice: the spread
    out = {}
    for turn_no, mode in enumerate(modes):
        real = getattr(ntm, "filtered_anchors", None)
        if mode == "composite":
            ntm.filtered_anchors = lambda eta, q=Q: ntm._filtered_anchor_rows(eta, q) + (None,)
        try:
            torch.manual_seed(1609)
            step = ts.build_fixmatch(dev, cfg=dict(ts.NTM_CFG, filter_outlier=mode != "off"), use_ddp=False)
            call = gs.GraphedFixMatchStep(step, warmup=2)
            turn = [0]

            def one():
                cur, nxt = batches[turn[0] % 2], batches[(turn[0] + 1) % 2]
                turn[0] += 1
                return call(cur[0], cur[1], next_batches=nxt)["loss"]
            for _ in range(6):
                loss = one()
            assert call.captured and torch.isfinite(loss), mode
            v = [timed(one, iters) / 1e3 for _ in range(rounds)]
        except RuntimeError as e:       # (a capture the wrapper refuses: reported)
            out.setdefault(mode, []).append({"refused": str(e).splitlines()[0][:200]})
            print("N=%5d iteration filter_outlier %-9s REFUSED: %s" % (n, mode, out[mode][-1]["refused"]), flush=True)
            continue
        finally:
            if real is not None:
                ntm.filtered_anchors = real
        nodes = {k: sum(c.values()) for k, c in call.node_types.items()}
        kinds = sorted(set().union(*[set(c) for c in call.node_types.values()]))
        out.setdefault(mode, []).append({"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "nodes": nodes,
                                         "node_kinds": kinds, "loss": float(loss)})
        print("N=%5d iteration filter_outlier %-9s run %d %7.2f ms [%.2f .. %.2f]  loss %.6f  nodes %s %s" % (
            n, mode, turn_no // 3 + 1, statistics.median(v), min(v), max(v), float(loss), nodes, kinds), flush=True)
        del call, step
        torch.cuda.empty_cache()
    return out


def trace_run(dev, reps):
    import torch
    from geot_amd import ntm
    for b, n in SHAPES:
        for kind in KINDS:
            eta, _ = make_eta(kind, b, n, dev)
            for _ in range(reps):
                ntm.filtered_anchors(eta, Q)
            torch.cuda.synchronize()
    print("trace run: %d calls for each of %d inputs" % (reps, len(SHAPES) * len(KINDS)))


def read_trace(path, reps):
    rows = {k: [] for k in KERNELS}
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    rows[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    out = {}
    combos = [(b, n, kind) for b, n in SHAPES for kind in KINDS]
    for k in KERNELS:
        rows[k].sort()
        assert len(rows[k]) == reps * len(combos), (k, len(rows[k]), reps * len(combos))
        for i, (b, n, kind) in enumerate(combos):
            d = [ns / 1e3 for _, ns in rows[k][i * reps:(i + 1) * reps]][reps // 5:]      # the first fifth: warm-up
            out.setdefault("%dx%d %s" % (b, n, kind), {})[k] = {"median_us": statistics.median(d), "min_us": min(d),
                                                                "max_us": max(d)}
    for name, row in out.items():
        print("%-18s %s" % (name, "   ".join("%s %6.1f us [%.1f .. %.1f]" % (k.replace("_kernel", ""), row[k]["median_us"],
                                                                           row[k]["min_us"], row[k]["max_us"]) for k in KERNELS)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--points", type=int, nargs="+", default=[16000, 24000])
    ap.add_argument("--skip-iteration", action="store_true")
    ap.add_argument("--only-off", action="store_true", help="the switch-off iteration alone (with --tree: of that checkout)")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose geot_amd is measured (default: this one)")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--read-trace", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.read_trace:
        result = {"kernels": read_trace(args.read_trace, args.reps)}
    else:
        sys.path.insert(0, os.path.abspath(args.tree))
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("time_filter_outlier.py measures on a GPU; none is visible")
        import geot_amd
        dev = torch.device("cuda:0")
        if args.trace_run:
            trace_run(dev, args.reps)
            return
        result = {"device": torch.cuda.get_device_name(0), "tree": os.path.dirname(os.path.dirname(geot_amd.__file__)), "C": C,
                  "q": Q, "calls": {}, "iteration": {}}
        print("package:", result["tree"], flush=True)
        if not args.only_off:
            result["calls"] = time_calls(dev, args.reps)
        if not args.skip_iteration:
            for n in args.points:
                result["iteration"][str(n)] = time_iteration(n, dev, args.iters, args.only_off)
    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
