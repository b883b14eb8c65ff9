"""cfg filter_outlier in the FixMatch+NTM step: iterations with the fused anchors (ntm.filtered_anchors, csrc/ntm_outlier.hip)
equal, bit for bit in every returned loss and in the whole state, the same iterations with the torch composite
ntm._filtered_anchor_rows in its place; the hipGraph replay equals the eager step before and after switch_ep and holds
kernel nodes only; the switch changes ema_t; off, the new path is never entered.

The small model and batches of tests/test_fixmatch_phase2_gpu.py."""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_fixmatch_phase2_gpu import _batch, _new_step, _same, _state  # noqa: E402

pytestmark = pytest.mark.gpu


def _cfg(**kw):
    from geot_amd import train_step as ts
    return dict(ts.NTM_CFG, threed_k=8, **kw)


@functools.lru_cache(maxsize=None)
def _batches():
    return [_batch(3), _batch(400)]


@functools.lru_cache(maxsize=None)
def _run(how):
    """Three eager iterations of a fresh step -> (losses per iteration, state, calls of ntm.filtered_anchors).
    how: "fused" | "composite" (filtered_anchors replaced by _filtered_anchor_rows) | "off" (cfg filter_outlier False)."""
    from geot_amd import ntm
    real, calls = ntm.filtered_anchors, []

    def fused(eta, q=0.97):
        calls.append(tuple(eta.shape))
        return real(eta, q)

    def composite(eta, q=0.97):
        calls.append(tuple(eta.shape))
        return ntm._filtered_anchor_rows(eta, q) + (None,)

    ntm.filtered_anchors = composite if how == "composite" else fused
    try:
        step = _new_step(_cfg(filter_outlier=how != "off"))
        torch.manual_seed(11)
        out = []
        for i in range(3):
            d, u = _batches()[i % 2]
            out.append({k: v.clone() for k, v in step(d, u).items()})
        torch.cuda.synchronize()
    finally:
        ntm.filtered_anchors = real
    return out, _state(step), calls


def test_three_iterations_equal_the_composite_bit_for_bit():
    a, sa, ca = _run("fused")
    b, sb, cb = _run("composite")
    assert ca == cb == [(2, 17, 4096)] * 3, (ca, cb)         # one call per iteration, on the weak view's soft-max
    for i, (x, y) in enumerate(zip(a, b)):
        assert set(x) == set(y) == {"loss", "sup", "unsup", "threed"}
        for k in x:
            assert torch.isfinite(x[k].float()) and torch.equal(x[k], y[k]), (i, k, float(x[k]), float(y[k]))
    _same(sa, sb, "parameters / moments / ema_t")


def test_the_switch_changes_ema_t_and_off_never_enters_the_new_path():
    _, on, _ = _run("fused")
    _, off, calls = _run("off")
    assert not calls
    assert not torch.equal(on["ema_t"], off["ema_t"])


EPOCHS = [1, 1, 1, 51, 51, 51]      # with warmup=1: P / M captured and replayed with the teacher, P@2 / M@2 after switch_ep


def test_graphed_step_equals_eager_and_holds_kernel_nodes_only():
    from geot_amd import graph_step as gs
    cfg = _cfg(filter_outlier=True)
    runs = {}
    for mode in ("eager", "graph"):
        step = _new_step(cfg)
        call = gs.GraphedFixMatchStep(step, warmup=1) if mode == "graph" else step
        torch.manual_seed(11)
        out = []
        for i, epoch in enumerate(EPOCHS):
            call.set_epoch(epoch)
            cur, nxt = _batches()[i % 2], _batches()[(i + 1) % 2]
            out.append({k: v.clone() for k, v in call(cur[0], cur[1], next_batches=nxt).items()})
        torch.cuda.synchronize()
        if mode == "graph":
            assert {"P", "M", "P@2", "M@2"} <= set(call.graphs) and call.captured, sorted(call.graphs)
            assert all(set(call.node_types[k]) == {"kernel"} for k in call.graphs), call.node_types
        runs[mode] = (out, _state(step))
    for i, (a, b) in enumerate(zip(runs["eager"][0], runs["graph"][0])):
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (i, k, float(a[k]), float(b[k]))
    _same(runs["eager"][1], runs["graph"][1], "graph against eager")
