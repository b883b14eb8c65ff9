"""The replayed FixMatch+NTM iteration at `bench.py --workload fixmatch` sizes (2 labelled + 2 unlabelled clouds of 24 000
points, the tooth configuration, tuned GEMM solutions, look-ahead on): the teacher's phase (epoch <= switch_ep) against the
self-labelling phase after it, each with the epoch meters off and on (geot_amd/meters.py).

    python tools/fixmatch_phase_timing.py [--steps 20] [--rounds 3] [--out profiles/fixmatch_phases.json]

The four GraphedFixMatchSteps are built and captured first, then timed in interleaved rounds of `--steps` replays each
(host clock around the replays, synchronised at both ends); the JSON holds every round and the median per configuration.
A GPU is required: there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--points", type=int, default=24000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fixmatch_phase_timing: no GPU")
    from geot_amd import _lib, graph_step as gs, train_step as ts, tuning
    from geot_amd.synth import make_batch, region_labels
    _lib.load()
    gemm_file = tuning.enable()
    dev = torch.device("cuda:0")
    n, bl, bu = args.points, 2, 2
    rng = np.random.default_rng(1609)

    def batch(seed):
        xyz_np, _ = make_batch(bl, n, start_index=seed)
        xyz_u_np, _ = make_batch(bu, n, start_index=seed + 10_000)
        xyz, xyz_u = torch.from_numpy(xyz_np).to(dev), torch.from_numpy(xyz_u_np).to(dev)
        strong = (xyz_u * torch.from_numpy(rng.uniform(0.8, 1.2, size=(bu, 1, 3)).astype(np.float32)).to(dev)).contiguous()
        z = torch.zeros(bl, 1, dtype=torch.long, device=dev)
        return ({"pos": xyz, "x": xyz.transpose(1, 2).contiguous(), "cls": z, "y": torch.from_numpy(region_labels(xyz_np)).to(dev)},
                {"pos_w": xyz_u, "x_w": xyz_u.transpose(1, 2).contiguous(), "cls_w": z, "pos_s": strong,
                 "x_s": strong.transpose(1, 2).contiguous(), "cls_s": z, "raw_pos": xyz_u,
                 "y": torch.from_numpy(region_labels(xyz_u_np)).to(dev)})
    batches = [batch(0), batch(100003)]
    configs = [("phase1", False), ("phase1", True), ("phase2", False), ("phase2", True)]
    steps = {}
    for phase, meters in configs:
        torch.manual_seed(1609)
        step = ts.build_fixmatch(dev, use_ddp=False, meters=meters)
        step.set_epoch(step.cfg["switch_ep"] + (1 if phase == "phase2" else 0))
        graphed = gs.GraphedFixMatchStep(step)
        turn = [0]

        def one(graphed=graphed, turn=turn):
            cur, nxt = batches[turn[0] % 2], batches[(turn[0] + 1) % 2]
            turn[0] += 1
            return graphed(cur[0], cur[1], next_batches=nxt)["loss"]
        for _ in range(graphed.warmup + 2):          # eager warm-up over the static buffers, the captures, one replay
            one()
        torch.cuda.synchronize()
        tag = "@2" if phase == "phase2" else ""
        assert "M" + tag in graphed.graphs and "P" + tag in graphed.graphs, sorted(graphed.graphs)
        steps[(phase, meters)] = (one, graphed)
    rounds = {"%s_meters_%s" % (p, "on" if m else "off"): [] for p, m in configs}
    for _ in range(args.rounds):
        for phase, meters in configs:
            one = steps[(phase, meters)][0]
            one()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                one()
            torch.cuda.synchronize()
            rounds["%s_meters_%s" % (phase, "on" if meters else "off")].append(1e3 * (time.perf_counter() - t0) / args.steps)
    med = {k: statistics.median(v) for k, v in rounds.items()}
    for phase in ("phase1", "phase2"):
        stats = steps[(phase, True)][1].step.meters.read(strict=False)[0]
        med["%s_meters_read_iterations" % phase] = stats["iterations"]
    res = {"what": "ms per replayed FixMatch+NTM iteration (GraphedFixMatchStep, look-ahead on), %d labelled + %d unlabelled "
                   "clouds x %d points; median of %d rounds of %d replays" % (bl, bu, n, args.rounds, args.steps),
           "median_ms": med, "rounds_ms": rounds, "gemm_file": os.path.basename(gemm_file) if gemm_file else None,
           "device": torch.cuda.get_device_name(dev), "torch": torch.__version__}
    # the two meter kernels alone, at these sizes: device events around 200 updates
    from geot_amd.meters import FixMatchMeters
    c = ts.NTM_CFG["num_classes"]
    m = FixMatchMeters(c, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    prob = torch.softmax(torch.randn(bu, c, n, device=dev, generator=g), 1)
    conf, lab = torch.max(prob, 1)
    y = torch.randint(0, c, (bu, n), device=dev, generator=g)
    s = torch.ones((), device=dev)
    corr = torch.rand(c, c, device=dev, generator=g)
    for _ in range(20):
        m.update(lab, conf, y, prob, s, s, s, s, corr)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200):
        m.update(lab, conf, y, prob, s, s, s, s, corr)
    e1.record()
    torch.cuda.synchronize()
    res["meters_update_us"] = 1e3 * e0.elapsed_time(e1) / 200
    res["meters_update_note"] = ("device time per update (count + finalize, back to back on one stream, launch gaps "
                                 "included), %d x %d points, %d classes" % (bu, n, c))
    res["phase2_over_phase1"] = med["phase2_meters_off"] / med["phase1_meters_off"]
    res["meters_cost_ms"] = {p: med["%s_meters_on" % p] - med["%s_meters_off" % p] for p in ("phase1", "phase2")}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
