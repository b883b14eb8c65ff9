"""Device time of decode_scans against cover_scans and against predict_scans behind one forward pass, and of its three parts.

    python tools/time_scan_decode.py [--reps 7] [--warmup 2] [--n 16000 24000] [--chunk 32768] [--out profiles/scan_decode_timing.txt]

B = 2 scans of ~1e5 vertices, C = 17, the configured model (TOOTH_SEG_CFG) in eval mode, N = 16 000 and 24 000 samples per scan,
ONE process, device events, the legs alternating after warm-up:

    decode a / b     decode_scans: one batch(), one forward pass, then per chunk geot_scan_decode_front, the model's decode_tail
                     (the 1536 -> 384 GEMM, BatchNorm, the head) and geot_scan_decode_finish; timed TWICE (a, b): their
                     difference is the spread of this method
    cover            cover_scans(rounds=1): P = ceil(M / N) forward passes, every vertex predicted directly as well
    interp           one batch(), one forward pass, predict_scans: today's default, every label interpolated
    validate         validate_scans over the two scans (the default path, for the record of what this commit leaves unchanged)

The one claim checked: decode is below cover by more than the spread of the two decode timings.  Then the parts of one decoded
batch, each over all its chunks: front (with the bytes the shapes require -- the rows written, the vertices and the table of
known rows read once -- over its time), tail, finish.  The text goes to --out as well as to stdout."""
import argparse
import json
import logging
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geot_amd.ext._common import call, ptr  # noqa: E402
from geot_amd.validation import (_out_offsets, _to_device, cover_scans, decode_scans, decode_work_table, predict_scans,  # noqa: E402
                                 validate_scans)
from tools.time_scan_cover import B, C, SIZES, make_scans  # noqa: E402


def timed(legs, reps, warmup):
    names = list(legs)
    times = {k: [] for k in names}
    for i in range(warmup + reps):
        for k in (names if i % 2 == 0 else names[::-1]):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            legs[k]()
            stop.record()
            stop.synchronize()
            if i >= warmup:
                times[k].append(start.elapsed_time(stop))
    return {k: {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(min(ts)), 3), "max_ms": round(float(max(ts)), 3)}
            for k, ts in times.items()}


def end_to_end(scans, model, n, chunk, reps, warmup):
    from geot_amd.openpoints.dataset import DeviceDraws, ValBatcher
    batcher = ValBatcher(scans, n, C, draws=DeviceDraws(9))
    cfg = {"num_points": n, "num_classes": C, "epoch": 1, "epochs": 1}

    def interp():
        data = batcher.batch([0, 1])
        return predict_scans(model(data)[0], data)
    legs = {"decode a": lambda: decode_scans(model, batcher, [0, 1], chunk=chunk), "cover": lambda: cover_scans(model, batcher, [0, 1]),
            "interp": interp, "validate": lambda: validate_scans(model, batcher, cfg),
            "decode b": lambda: decode_scans(model, batcher, [0, 1], chunk=chunk)}
    res = timed(legs, reps, warmup)
    a, b, c = res["decode a"]["median_ms"], res["decode b"]["median_ms"], res["cover"]["median_ms"]
    res["passes"] = max(-(-m // n) for m in SIZES)
    res["decode_spread_ms"] = round(abs(a - b), 3)
    res["cover_minus_decode_ms"] = round(c - max(a, b), 3)
    res["decode_below_cover_by_more_than_the_spread"] = bool(c - max(a, b) > abs(a - b))
    res["decode_minus_interp_ms"] = round(min(a, b) - res["interp"]["median_ms"], 3)
    return res


def parts(scans, model, n, chunk, reps, warmup):
    """front / tail / finish of one decoded batch, each over all chunks, on the state of one forward pass."""
    from geot_amd.openpoints.dataset import DeviceDraws, ValBatcher
    seg, dev = model.segmentor, scans.device
    data = ValBatcher(scans, n, C, draws=DeviceDraws(9)).batch([0, 1], affine=True)
    seg.keep_decode_state = True
    model(data)
    p = seg.decode_front_params()
    seg.keep_decode_state, seg.decode_state = False, None
    sizes = [int(m) for m in data["sizes"]]
    m, c_out = int(p["a"].shape[1]), int(p["a"].shape[2])
    table, chunks = decode_work_table(sizes, chunk)
    work = _to_device(table, dev)
    z = torch.empty((max(r for _, _, r in chunks), c_out), device=dev)
    zs = [torch.randn((rows, c_out), device=dev).relu_() for _, _, rows in chunks[:1]]
    logits = torch.randn((C, z.shape[0]), device=dev)
    pred, offs = torch.empty(sum(sizes), dtype=torch.int64, device=dev), _out_offsets(sizes, dev)
    head = (dev, B, m, c_out, int(p["relu"]), len(scans), int(scans.points.shape[0]), ptr(scans.points), ptr(scans.offsets),
            ptr(data["scan_ids"]), ptr(data["center"]), ptr(data["scale"]), ptr(data["view_center"]), ptr(data["view_scale"]),
            ptr(p["known"]), ptr(p["a"]), ptr(p["skip_const"]), ptr(p["w_xyz"]), ptr(p["ch_scale"]), ptr(p["ch_shift"]))

    def front():
        for first, count, rows in chunks:
            call("geot_scan_decode_front", *head, count, ptr(work) + 16 * first, rows, ptr(z), None, None, None)

    def tail():
        for _, _, rows in chunks:
            seg.decode_tail(zs[0][:rows])

    def finish():
        for first, count, rows in chunks:
            lg = logits[:, :rows].contiguous() if rows != logits.shape[1] else logits
            call("geot_scan_decode_finish", dev, B, C, len(scans), int(scans.points.shape[0]), ptr(scans.labels), ptr(scans.offsets),
                 ptr(data["scan_ids"]), count, ptr(work) + 16 * first, rows, ptr(lg), ptr(offs), ptr(pred), None)
    res = timed({"front": front, "tail": tail, "finish": finish, "front b": front}, reps, warmup)
    total = sum(sizes)
    nbytes = total * c_out * 4 + total * 12 + B * m * c_out * 4 + B * m * 12
    res["chunks"], res["rows"], res["m"], res["c_out"] = len(chunks), total, m, c_out
    res["front_bytes"] = nbytes
    res["front_TB_per_s"] = round(nbytes / (res["front"]["median_ms"] * 1e-3) / 1e12, 3)
    res["front_spread_ms"] = round(abs(res["front"]["median_ms"] - res["front b"]["median_ms"]), 3)
    res["distance_evaluations"] = total * m
    res["tail_gflop"] = round(2.0 * total * (c_out * seg.trans_dim + seg.trans_dim * 128 + 128 * C) / 1e9, 1)
    return res


def report(res):
    lines = [__doc__.split("\n\n")[0].strip(), "", "device %s, %d repetitions after %d warm-up rounds per leg, chunk = %d vertices; B = %d scans of %s "
             "vertices, C = %d" % (res["device"], res["reps"], res["warmup"], res["chunk"], B, list(SIZES), C), "",
             "median ms between device events (min .. max)"]
    for key, leg in res.items():
        if key.startswith("N="):
            e, p = leg["end_to_end"], leg["parts"]
            f = lambda k: "%.3f (%.3f .. %.3f)" % (e[k]["median_ms"], e[k]["min_ms"], e[k]["max_ms"])
            lines += ["%s: decode_scans a %s, b %s; cover_scans (P = %d passes) %s; one forward + predict_scans %s; validate_scans %s" %
                      (key, f("decode a"), f("decode b"), e["passes"], f("cover"), f("interp"), f("validate")),
                      "    cover - decode = %.3f ms, the two decode timings differ by %.3f ms: decoded is %s; decode - interp = %.3f ms" %
                      (e["cover_minus_decode_ms"], e["decode_spread_ms"], "CHEAPER than covered by more than the spread"
                       if e["decode_below_cover_by_more_than_the_spread"] else "NOT cheaper than covered by more than the spread",
                       e["decode_minus_interp_ms"]),
                      "    parts over %d chunks (%d rows, m = %d, c_out = %d): front %.3f ms (again %.3f; %.2e bytes required -> %.3f TB/s; "
                      "%.2e distance evaluations), tail %.3f ms (%.1f GFLOP), finish %.3f ms" %
                      (p["chunks"], p["rows"], p["m"], p["c_out"], p["front"]["median_ms"], p["front b"]["median_ms"], p["front_bytes"],
                       p["front_TB_per_s"], p["distance_evaluations"], p["tail"]["median_ms"], p["tail_gflop"], p["finish"]["median_ms"])]
    return "\n".join(lines) + "\n\n" + json.dumps(res, indent=1) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, nargs="+", default=[16000, 24000])
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_decode_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_scan_decode: needs a GPU (a timing taken anywhere else says nothing)")
    logging.disable(logging.INFO)
    dev = torch.device("cuda:0")
    from geot_amd.openpoints.models.backbone.transformer import TOOTH_SEG_CFG
    from geot_amd.openpoints.models.segmentation import WholePartSeg
    scans = make_scans(dev)
    torch.manual_seed(0)
    model = WholePartSeg(segmentor_args=dict(NAME="PointTransformer_seg_T", **TOOTH_SEG_CFG)).to(dev).eval()
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "chunk": args.chunk}
    with torch.no_grad():
        for n in args.n:
            res["N=%d" % n] = {"end_to_end": end_to_end(scans, model, n, args.chunk, args.reps, args.warmup),
                               "parts": parts(scans, model, n, args.chunk, args.reps, args.warmup)}
            print("N=%d" % n, json.dumps(res["N=%d" % n]), flush=True)
    text = report(res)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
