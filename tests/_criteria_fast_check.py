"""Child process of tests/test_criteria_gpu.py: GEOT_GRAPH_LAUNCH=fast (the runtime's graph packet capture stays ON), where
the wrappers refuse any graph that is not kernel nodes alone.  Two switched FixMatch+NTM configurations replayed across
switch_ep with the look-ahead (and, for the first, the epoch meters) against the eager step, bit for bit, and the supervised
step with Weight_CELoss and its extra static buffer.  Prints "criteria fast ok <node counts>" at the end."""
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
from geot_amd.openpoints.models.backbone.transformer import PointTransformer_seg_T  # noqa: E402

assert not geot_amd.graph_replay_is_safe()
batches = [_batch(3), _batch(400)]
for seed, (d, u) in zip((3, 400), batches):
    d["class_weights"] = (torch.rand(2, 17, generator=torch.Generator().manual_seed(seed)) * 0.1 + 0.01).to(DEV)
    u["y"] = d["y"].flip(0).contiguous()
CONFIGS = {
    "u_t+all": dict(criterion_u="Poly1FocalLoss_U_T", use_feat_loss=True, use_identity_loss=True, use_3d_loss=True),
    "wce+wce_u-3d": dict(criterion="Weight_CELoss", criterion_u="Weight_CELoss_U", use_3d_loss=False),
}
epochs = [49, 50, 50, 50, 51, 51, 51, 51]      # P / M captured and replayed before the switch, P@2 / M@2 after it
census = {}
for tag, switches in CONFIGS.items():
    cfg = dict(ts.NTM_CFG, threed_k=8, feat_k=8, **switches)
    meters = tag == "u_t+all"
    runs = {}
    for mode in ("eager", "graph"):
        torch.manual_seed(5)
        step = ts.build_fixmatch(DEV, seg_cfg=SMALL, cfg=cfg, use_ddp=False, meters=meters)
        call = gs.GraphedFixMatchStep(step, warmup=2) if mode == "graph" else step
        torch.manual_seed(11)
        losses = []
        for i, epoch in enumerate(epochs):
            call.set_epoch(epoch)
            cur, nxt = batches[i % 2], batches[(i + 1) % 2]
            res = call(cur[0], cur[1], next_batches=nxt)
            losses.append({k: v.clone() for k, v in res.items()})
        torch.cuda.synchronize()
        runs[mode] = (losses, _state(step), step.meters.read()[0] if meters else None)
    assert {"P", "M", "P@2", "M@2"} <= set(call.node_types), call.node_types
    assert all(set(v) == {"kernel"} for v in call.node_types.values()), (tag, call.node_types)
    if not cfg["use_3d_loss"]:
        assert "raw_pos" not in call.next[1], sorted(call.next[1])          # the look-ahead no longer reads it
    for i, (a, b) in enumerate(zip(runs["eager"][0], runs["graph"][0])):
        assert set(a) == set(b) and all(torch.isfinite(a[k]) and torch.equal(a[k], b[k]) for k in a), (tag, i)
    _same(runs["eager"][1], runs["graph"][1], tag)
    if meters:
        a, b = runs["eager"][2], runs["graph"][2]
        for k in ("train_loss", "manifold_loss_feat", "insT_identity_loss", "insT_threed_loss"):
            assert a[k] == b[k] and a[k] != 0.0, (k, a[k], b[k])
    census[tag] = dict(call.node_types)

# the supervised step with Weight_CELoss: class_weights is a fourth static buffer
torch.manual_seed(0)
init = PointTransformer_seg_T(**SMALL).state_dict()
runs = {}
for mode in ("eager", "graph"):
    m = PointTransformer_seg_T(**SMALL).to(DEV)
    m.load_state_dict(init)
    step = ts.SupervisedStep(m, criterion="Weight_CELoss")
    call = gs.GraphedSupervisedStep(step, warmup=2) if mode == "graph" else step
    torch.manual_seed(7)
    losses = []
    for i in range(5):
        d = batches[i % 2][0]
        losses.append(call(d["pos"], d["cls"], d["y"], class_weights=d["class_weights"]).clone())
    torch.cuda.synchronize()
    runs[mode] = (losses, {k: v.clone() for k, v in m.state_dict().items()})
assert len(call.x) == 4 and all(set(v) == {"kernel"} for v in call.node_types.values()), call.node_types
assert all(torch.equal(a, b) for a, b in zip(*(runs[k][0] for k in ("eager", "graph"))))
_same(runs["eager"][1], runs["graph"][1], "supervised Weight_CELoss")
census["supervised"] = dict(call.node_types)
print("criteria fast ok", census)
