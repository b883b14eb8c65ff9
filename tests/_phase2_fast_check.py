"""Child process of tests/test_fixmatch_phase2_gpu.py: GEOT_GRAPH_LAUNCH=fast (the runtime's graph packet capture stays ON).
GraphedFixMatchStep across switch_ep, with the look-ahead and the epoch meters on: the phase-2 graphs must capture as kernel
nodes alone (the wrapper refuses anything else in this mode) and replay to the eager step's bits with eager launches between
the replays.  Prints "phase2 fast ok <node counts>" at the end."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
assert os.environ.get("GEOT_GRAPH_LAUNCH") == "fast" and "DEBUG_CLR_GRAPH_PACKET_CAPTURE" not in os.environ
import geot_amd  # noqa: E402
import torch  # noqa: E402
from test_fixmatch_phase2_gpu import _batch, _state, _same, SMALL, DEV  # noqa: E402
from geot_amd import train_step as ts, graph_step as gs  # noqa: E402

assert not geot_amd.graph_replay_is_safe()
flood_buf = torch.randn(1 << 16, device=DEV)
cfg = dict(ts.NTM_CFG, threed_k=8)
batches = [_batch(3), _batch(400)]
for d, u in batches:
    u["y"] = d["y"].flip(0).contiguous()
epochs = [48, 49, 50, 50, 51, 51, 52, 52]      # P / M captured and replayed before the switch, P@2 / M@2 after it
runs = {}
for mode in ("eager", "graph"):
    torch.manual_seed(5)
    step = ts.build_fixmatch(DEV, seg_cfg=SMALL, cfg=cfg, use_ddp=False, meters=True)
    call = gs.GraphedFixMatchStep(step, warmup=2) if mode == "graph" else step
    torch.manual_seed(11)
    losses = []
    for i, epoch in enumerate(epochs):
        call.set_epoch(epoch)
        cur, nxt = batches[i % 2], batches[(i + 1) % 2]
        res = call(cur[0], cur[1], next_batches=nxt)
        losses.append({k: v.clone() for k, v in res.items()})
        if i in (3, 6):
            for _ in range(20000):
                flood_buf.mul_(1.0)
    torch.cuda.synchronize()
    stats = step.meters.read()[0]
    runs[mode] = (losses, _state(step), stats)
assert {"P", "M", "P@2", "M@2"} <= set(call.node_types), call.node_types
assert all(set(v) == {"kernel"} for v in call.node_types.values()), call.node_types
for i, (a, b) in enumerate(zip(runs["eager"][0], runs["graph"][0])):
    assert all(torch.equal(a[k], b[k]) for k in a), i
_same(runs["eager"][1], runs["graph"][1], "fast mode")
a, b = runs["eager"][2], runs["graph"][2]
for k in ("train_loss", "th_percentage", "teacher_acc", "student_acc", "mean_pseudo_label_acc", "over_acc_wobg",
          "mean_pseudo_label_acc_classwise", "mean_th_meter_u_classwise_recall"):
    assert a[k] == b[k], (k, a[k], b[k])
assert a["iterations"] == b["iterations"] == len(epochs)
print("phase2 fast ok", {k: v for k, v in call.node_types.items()})
