"""Whole-scan validation and voting with the passes' geometry computed ahead and the forward passes replayed from hipGraphs
(geot_amd/validation.py graph= / lookahead=, geot_amd/graph_eval.py GraphedForward).  Nothing here has a tolerance: the
switches put the same kernels in another order, so every comparison with the default path is exact -- the sliced geometry
against each pass's own, the metrics' counts and per-scan lists, the voted labels, a replay against a fresh eager forward
pass after the weights moved."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (the model of tests/test_graph_step_gpu.py)
SMALL = dict(trans_dim=384, depth=3, num_heads=4, group_size=32, num_group=128, encoder_dims=256, nclasses=17,
             drop_path_rate=0.1, downsample_targets=[2048, 1024, 512], extract_layers=[1, 2, 3])
N = 4096
SIZES, JAWS = [5003, 9001, 7000, 6111, 8192], [0, 1, 1, 0, 1]       # batch_size 2: two full batches and a short one
CFG = dict(num_points=N, num_classes=17, num_votes=3, epoch=1, epochs=1)
CENTER, SCALE = np.array([14.0, -37.0, 61.0], np.float32), np.float32(31.5)
_made = {}


def _scans():
    """Five ragged scans in scan coordinates with coherent labels in [0, 17), both jaws present."""
    if "scans" not in _made:
        from geot_amd.openpoints.dataset import DeviceScanSet
        from geot_amd.synth import make_cloud, region_labels
        units = [make_cloud(m, 700 + i)[0] for i, m in enumerate(SIZES)]
        _made["scans"] = DeviceScanSet([(u * np.float32(1.01) * SCALE + CENTER).astype(np.float32) for u in units],
                                       [(region_labels(u) % 17).astype(np.int32) for u in units], cls=JAWS, device=DEV)
    return _made["scans"]


def _model():
    if "model" not in _made:
        from geot_amd.openpoints.models.segmentation import WholePartSeg
        torch.manual_seed(0)
        _made["model"] = WholePartSeg(segmentor_args=dict(NAME="PointTransformer_seg_T", **SMALL)).to(DEV).eval()
    return _made["model"]


def _seed(seed=11):
    """Every host generator a batcher draws from: numpy's (the vertex samples), python's and torch's (the vote list's views)."""
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)


def _validated(monkeypatch, call, *args, **kw):
    """One validator run from a fixed seed -> (the returned triple, the SegMetrics counts, read()'s dict)."""
    from geot_amd import validation as V
    seen = {}
    read = V.SegMetrics.read

    def spy(self):
        seen["counts"] = self.counts[:self.scans].clone()
        seen["out"] = read(self)
        return seen["out"]
    monkeypatch.setattr(V.SegMetrics, "read", spy)
    _seed()
    triple = getattr(V, call)(_model(), *args, **kw)
    monkeypatch.setattr(V.SegMetrics, "read", read)
    return triple, seen["counts"], seen["out"]


def _same_validation(a, b):
    assert all(type(x) is type(y) and np.array_equal(x, y, equal_nan=True) for x, y in zip(a[0], b[0])), (a[0], b[0])
    assert torch.equal(a[1], b[1])
    assert a[2]["scans"] == b[2]["scans"] >= 3
    for key in ("acc_list", "miou_list", "mdsc_list"):
        assert len(a[2][key]) == len(b[2][key]) == a[2]["scans"]
        for x, y in zip(a[2][key], b[2][key]):
            assert type(x) is type(y) and np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), (key, x, y)


def _kernel_only(wrapper, kinds=("F", "P")):
    assert wrapper.graphs and not wrapper.refused, (list(wrapper.graphs), wrapper.refused)
    assert sorted({name[0] for name in wrapper.graphs}) == sorted(kinds)
    assert set(wrapper.node_types) == set(wrapper.graphs)
    assert all(set(census) == {"kernel"} and census["kernel"] >= 1 for census in wrapper.node_types.values()), wrapper.node_types


# ------------------------------------------------------------------------------------------------ 1. sliced geometry
def test_a_slice_of_the_concatenated_geometry_is_each_passes_own_geometry():
    from geot_amd.graph_eval import tree_tensors
    from geot_amd.openpoints.dataset import ValBatcher
    seg = _model().segmentor
    batcher = ValBatcher(_scans(), N)
    _seed(3)
    positions = [batcher.batch(ids)["pos"] for ids in ([0, 1], [2, 3], [4, 0])]
    with torch.no_grad():
        whole = seg.prefetch_geometry(torch.cat(positions, 0), inline=True)
        assert whole is not None and whole.static
        for k, pos in enumerate(positions):
            alone = dict(tree_tensors(seg.prefetch_geometry(pos, inline=True)))
            cut = dict(tree_tensors(whole.slice(2 * k, 2 * k + 2)))
            assert set(alone) == set(cut) and len(alone) >= 20, sorted(set(alone) ^ set(cut))
            for path, want in alone.items():
                got = cut[path]
                assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), (k, path)


# ------------------------------------------------------------------------------------------------ 2. validate_scans
def test_validate_scans_is_the_same_under_every_switch(monkeypatch):
    from geot_amd.graph_eval import GraphedForward
    base = _validated(monkeypatch, "validate_scans", _scans(), CFG, batch_size=2)
    assert all(np.isfinite(float(v)) for v in base[0])
    _same_validation(base, _validated(monkeypatch, "validate_scans", _scans(), CFG, batch_size=2, lookahead=1))
    _same_validation(base, _validated(monkeypatch, "validate_scans", _scans(), CFG, batch_size=2, lookahead=2))
    for look in (0, 2):
        wrapper = GraphedForward(_model(), warmup=1)
        for epoch in range(3):          # warm-up, capture, replay: every epoch the same values
            _same_validation(base, _validated(monkeypatch, "validate_scans", _scans(), CFG, batch_size=2, graph=wrapper,
                                              lookahead=look))
        assert wrapper.replays >= 4
        _kernel_only(wrapper)
    # graph=True: the model's own wrapper, kept from epoch to epoch
    from geot_amd.graph_eval import graphed_forward
    for epoch in range(2):
        _same_validation(base, _validated(monkeypatch, "validate_scans", _scans(), CFG, batch_size=2, graph=True))
    assert graphed_forward(_model()).replays >= 1


def test_validate_scans_with_the_batches_built_on_a_side_stream(monkeypatch):
    """The batcher's side stream: the batches drawn ahead are joined where their positions are first read."""
    from geot_amd.graph_eval import GraphedForward
    from geot_amd.openpoints.dataset import ValBatcher
    base = _validated(monkeypatch, "validate_scans", _scans(), CFG, batch_size=2)
    batcher = ValBatcher(_scans(), N, stream=torch.cuda.Stream())
    wrapper = GraphedForward(_model(), warmup=1)
    for kw in (dict(), dict(lookahead=1), dict(lookahead=5), dict(graph=wrapper), dict(graph=wrapper, lookahead=2),
               dict(graph=wrapper, lookahead=2)):
        _same_validation(base, _validated(monkeypatch, "validate_scans", batcher, CFG, batch_size=2, indices=None, **kw))
    _same_validation(_validated(monkeypatch, "validate_scans", _scans(), CFG, batch_size=2, indices=[4, 2, 1]),
                     _validated(monkeypatch, "validate_scans", batcher, CFG, batch_size=2, indices=[4, 2, 1], graph=wrapper))
    _kernel_only(wrapper)


# ------------------------------------------------------------------------------------------------ 3. votes
@pytest.mark.parametrize("device_draws", [False, True])
@pytest.mark.parametrize("refine", [0, 10])
def test_voted_labels_and_voted_validation_are_the_same_under_every_switch(monkeypatch, device_draws, refine):
    from geot_amd import validation as V
    from geot_amd.graph_eval import GraphedForward
    from geot_amd.openpoints.dataset import DeviceDraws, VoteBatcher
    batcher = VoteBatcher(_scans(), N)

    def draws():
        return DeviceDraws(5) if device_draws else None

    def voted(**kw):
        _seed()
        return V.vote_scans(_model(), batcher, [3, 1], 3, draws=draws(), refine=refine, **kw)
    base = voted()
    assert [p.shape for p in base] == [(1, SIZES[3]), (1, SIZES[1])]
    wrapper = GraphedForward(_model(), warmup=1)
    for kw in (dict(lookahead=3), dict(lookahead=True), dict(lookahead=2), dict(lookahead=3, graph=wrapper),
               dict(lookahead=3, graph=wrapper), dict(lookahead=True, graph=wrapper)):
        got = voted(**kw)
        assert len(got) == len(base) and all(torch.equal(g, b) for g, b in zip(got, base)), kw
    _kernel_only(wrapper)                                   # one geometry graph for the three passes, one forward graph
    assert len(wrapper.graphs) == 2 and wrapper.replays >= 5
    vbase = _validated(monkeypatch, "validate_scans_voted", batcher, CFG, batch_size=2, draws=draws(), refine=refine)
    for kw in (dict(lookahead=3), dict(lookahead=3, graph=wrapper), dict(lookahead=True, graph=wrapper)):
        _same_validation(vbase, _validated(monkeypatch, "validate_scans_voted", batcher, CFG, batch_size=2, draws=draws(),
                                           refine=refine, **kw))
    _kernel_only(wrapper)


# ------------------------------------------------------------------------------------------------ 4. weights move
def test_a_replay_sees_updated_weights_and_recaptures_for_a_new_tensor():
    from geot_amd.graph_eval import GraphedForward
    from geot_amd.openpoints.dataset import ValBatcher
    from geot_amd.openpoints.models.segmentation import WholePartSeg
    torch.manual_seed(0)
    model = WholePartSeg(segmentor_args=dict(NAME="PointTransformer_seg_T", **SMALL)).to(DEV).eval()      # (edited below)
    head = model.segmentor.seg_head
    _seed(4)
    batch = ValBatcher(_scans(), N).batch([0, 1])
    wrapper = GraphedForward(model, warmup=1)
    with torch.no_grad():
        def replayed():
            geometry = wrapper.lookahead([batch["pos"]])
            wrapper.join()
            return wrapper(batch, geometry.slice(0, 2))[0]
        replayed()
        first = replayed().clone()
        assert torch.equal(first, replayed()) and wrapper.replays >= 3
        graph = wrapper.graphs[("F", wrapper.signature(batch, wrapper.ahead or wrapper.lookahead([batch["pos"]])))][0]
        assert torch.equal(first, model(batch)[0])
        head[3].weight.mul_(1.5)                        # a training step / an EMA update / load_state_dict: in place
        head[1].running_mean.fill_(0.25)
        moved = replayed().clone()
        assert torch.equal(moved, model(batch)[0]) and not torch.equal(moved, first)
        assert [g for name, (g, _) in wrapper.graphs.items() if name[0] == "F"] == [graph]         # no recapture
        head[3].weight = torch.nn.Parameter(head[3].weight.detach().clone() * 0.5)                 # another tensor
        again = replayed().clone()
        assert torch.equal(again, model(batch)[0]) and not torch.equal(again, moved)
        assert [g for name, (g, _) in wrapper.graphs.items() if name[0] == "F"] != [graph]         # captured again
        assert torch.equal(again, replayed())
    _kernel_only(wrapper)


# ------------------------------------------------------------------------------------------------ 5. node census
def test_every_graph_holds_kernel_nodes_only(monkeypatch):
    from geot_amd.graph_eval import GraphedForward
    wrapper = GraphedForward(_model(), warmup=1)
    for epoch in range(2):
        _validated(monkeypatch, "validate_scans", _scans(), CFG, batch_size=2, graph=wrapper, lookahead=1)
    _kernel_only(wrapper)
    assert len(wrapper.graphs) == 2                     # the short last batch runs eagerly: no graph of its own


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_training_mode_and_enabled_grad_are_refused_before_any_capture():
    from geot_amd.graph_eval import GraphedForward
    from geot_amd.openpoints.dataset import ValBatcher
    from geot_amd.openpoints.models.segmentation import WholePartSeg
    model = WholePartSeg(segmentor_args=dict(NAME="PointTransformer_seg_T", **SMALL)).to(DEV)
    batch = ValBatcher(_scans(), N).batch([0, 1])
    wrapper = GraphedForward(model, warmup=0)
    model.train()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="training mode"):
            wrapper.lookahead([batch["pos"]])
        with pytest.raises(RuntimeError, match="training mode"):
            wrapper(batch, None)
    model.eval()
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="grad is enabled"):
            wrapper.lookahead([batch["pos"]])
        with pytest.raises(RuntimeError, match="grad is enabled"):
            wrapper(batch, None)
    assert not wrapper.graphs and not wrapper.inputs and wrapper.replays == 0


# ------------------------------------------------------------------------------------------------ 7. fallback
def test_a_refused_capture_runs_eagerly_and_is_remembered(monkeypatch):
    from geot_amd import graph_eval
    base = _validated(monkeypatch, "validate_scans", _scans(), CFG, batch_size=2)
    asked = []

    def census(graph):
        asked.append(graph)
        return {"kernel": 7, "memset": 1}
    monkeypatch.setattr(graph_eval, "_census", census)
    wrapper = graph_eval.GraphedForward(_model(), warmup=1)
    for epoch in range(3):
        _same_validation(base, _validated(monkeypatch, "validate_scans", _scans(), CFG, batch_size=2, graph=wrapper, lookahead=2))
        assert epoch == 0 or len(asked) == 2            # one refusal per signature (P and F), never tried again
    assert not wrapper.graphs and not wrapper.node_types and wrapper.replays == 0
    assert sorted(name[0] for name in wrapper.refused) == ["F", "P"]
    assert all("memset" in why and "eagerly" in why for why in wrapper.refused.values())
