"""train_step.BatchWork -- the typed product of a FixMatch iteration's batch-only work -- under graph_step's tree helpers, and
the step's table of look-ahead keys; plain CPU tensors stand in for the fields, no device and no model are involved."""
import pytest
import torch

from geot_amd import graph_step as gs, train_step as ts
from geot_amd.openpoints.models.backbone.geometry import FpEntry, Geometry, IndexPlan

B, N, C = 2, 16, 17


def _geometry(b, seed):
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(b, N, 3, generator=g)
    idx = torch.randint(0, N, (b * 4 * 3,), generator=g, dtype=torch.int32)
    fp = FpEntry(torch.randint(0, N, (b, N, 3), generator=g, dtype=torch.int32), torch.rand(b, N, 3, generator=g))
    plan = IndexPlan([torch.rand(b, 8, 3, generator=g)], [torch.rand(b, 3, 8, generator=g)], torch.rand(b, 3, 4, generator=g), fp)
    return Geometry(pts, (torch.rand(b, 4, 3, 3, generator=g), torch.rand(b, 4, 3, generator=g), idx), plan, True, "cl", static=True)


def _work(seed, full=True):
    """All fields set (the moving and the frozen teacher's fields at once), or geom_s and knn alone: the product after
    switch_ep with cfg pseudo_refine and use_contrastive off."""
    g = torch.Generator().manual_seed(100 + seed)
    knn = (torch.randint(0, N, (B, N, 8), generator=g, dtype=torch.int32), torch.randperm(B * N, generator=g).to(torch.int32))
    if not full:
        return ts.BatchWork(_geometry(3 * B, seed), knn=knn)
    pred = torch.rand(B, C, N, generator=g)
    return ts.BatchWork(_geometry(3 * B, seed), _geometry(B, seed + 50), (pred,) + tuple(pred.max(1)),
                        torch.rand(B, 128, N, generator=g), knn, torch.randint(0, N, (B, N, 4), generator=g, dtype=torch.int32))


def _tensors(obj):
    if torch.is_tensor(obj):
        return [obj]
    if isinstance(obj, (list, tuple)):
        return [t for v in obj for t in _tensors(v)]
    if hasattr(obj, "tree_fields"):
        return [t for k in obj.tree_fields()[0] for t in _tensors(getattr(obj, k))]
    return []


@pytest.mark.parametrize("full", [True, False])
def test_clone_copy_round_trip(full):
    first, second = _work(1, full), _work(2, full)
    want = [t.clone() for t in _tensors(second)]
    assert len(want) == (23 if full else 10)
    buffers = gs.tree_clone(first)
    assert type(buffers) is ts.BatchWork and [k for k in ts.BatchWork.FIELDS if buffers.made(k)] == \
        (list(ts.BatchWork.FIELDS) if full else ["geom_s", "knn"])
    held = _tensors(buffers)
    for a, b in zip(held, _tensors(first)):
        assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()
    assert buffers.geom_s.pts is None and buffers.geom_s.static and buffers.geom_s.training
    gs.tree_copy_(buffers, second)
    after = _tensors(buffers)
    assert all(a is b for a, b in zip(after, held))                                  # the same buffers, refilled
    assert all(torch.equal(a, b) for a, b in zip(after, want)) and all(torch.equal(a, b) for a, b in zip(_tensors(second), want))


@pytest.mark.parametrize("field", ["feat_t", "refine_nbr", "pseudo", "geom_t"])
def test_copy_refuses_a_field_that_appears_or_disappears(field):
    with_it, without = _work(1), _work(2)
    setattr(without, field, None)
    assert not without.made(field) and getattr(without, field) is None
    with pytest.raises(RuntimeError, match="became"):                                # None in the buffers, there in the product
        gs.tree_copy_(gs.tree_clone(without), with_it)
    with pytest.raises(RuntimeError, match=field):                                   # and the reverse
        gs.tree_copy_(gs.tree_clone(with_it), without)


def test_copy_refuses_a_changed_shape():
    buffers, other = gs.tree_clone(_work(1)), _work(2)
    other.refine_nbr = other.refine_nbr[:, :, :3].contiguous()
    with pytest.raises(RuntimeError, match=r"refine_nbr.*does not fit"):
        gs.tree_copy_(buffers, other)
    other = _work(2)
    other.knn = (other.knn[0], other.knn[1][:-1])
    with pytest.raises(RuntimeError, match=r"knn\[1\].*does not fit"):
        gs.tree_copy_(buffers, other)
    other = _work(2)
    other.geom_s.training = False                                                    # a python scalar of a nested object
    with pytest.raises(RuntimeError, match="became"):
        gs.tree_copy_(buffers, other)


def test_detach_releases_the_autograd_graph():
    w = torch.rand(3, requires_grad=True)
    work = _work(1)
    work.feat_t = work.feat_t * w.sum()
    work.pseudo = (work.pseudo[0] * w[0], work.pseudo[1] * w[1], work.pseudo[2])
    assert work.feat_t.grad_fn is not None and work.pseudo[0].grad_fn is not None and work.pseudo[1].grad_fn is not None
    bare = gs.tree_detach(work)
    assert type(bare) is ts.BatchWork and len(_tensors(bare)) == len(_tensors(work))
    for a, b in zip(_tensors(bare), _tensors(work)):
        assert a.grad_fn is None and not a.requires_grad and a.data_ptr() == b.data_ptr()
    # the split capture's M1 product, as FixMatchNTMStep.forward_backward_head returns it: (losses, rest), rest = (what the cut
    # left of the backward: (outputs, gradients), the next ema_t); the supervised step's rest is (outputs, gradients) alone
    outputs = [torch.rand(2, 4) * w[0] for _ in range(3)]
    grads = [torch.rand(2, 4) * w[1] for _ in range(3)]
    losses = {"loss": (w * w).sum(), "anchors": torch.tensor(3)}
    m1 = (losses, ((outputs, grads), torch.eye(C) * w[2]))
    assert all(t.grad_fn is not None for t in outputs + grads + [m1[1][1], losses["loss"]])
    bare = gs.tree_detach(m1)
    flat = list(bare[0].values()) + bare[1][0][0] + bare[1][0][1] + [bare[1][1]]
    assert len(flat) == 9 and all(t.grad_fn is None and not t.requires_grad for t in flat)
    assert gs.tree_detach((losses, (None, m1[1][1])))[1][0] is None                  # a model that cannot cut


def test_a_read_joins_only_what_was_made_on_a_side_stream(monkeypatch):
    joined = []
    monkeypatch.setattr(ts, "_join", lambda dev, side, *tensors: joined.append((side, tensors)))

    class Side:
        device = "here"
    work, a, b = _work(1), Side(), Side()
    work.made_on(a, "pseudo", "feat_t")
    work.made_on(b, "knn")
    work.made_on(b, "refine_nbr")
    work.made_on(None, "geom_s")
    assert work.made("pseudo") and not joined                                        # asking is not reading
    assert work.geom_s is not None and work.geom_t is not None and not joined        # made in line
    pseudo = work.pseudo
    assert len(joined) == 1 and joined[0][0] is a and len(joined[0][1]) == 4         # the three labels and the feature, together
    assert all(x is y for x, y in zip(joined[0][1], pseudo + (work.feat_t,))) and len(joined) == 1
    assert work.knn is not None and len(joined) == 2 and joined[1][0] is b and len(joined[1][1]) == 2
    assert work.refine_nbr is not None and len(joined) == 3 and joined[2][1][0] is work.refine_nbr
    clone = gs.tree_clone(_work(2))
    assert clone.pseudo is not None and len(joined) == 3                             # a clone has nothing to join


# the table at the commit before this module: graph_step._P_KEYS / _P_KEYS_2 / _p_keys, by phase and cfg use_3d_loss
KEYS = {
    ("", True): (("pos",), ("pos_s", "pos_w", "x_w", "cls_w", "raw_pos")),
    ("@e", True): (("pos",), ("pos_s", "pos_w", "x_w", "cls_w", "raw_pos")),
    ("@2", True): (("pos",), ("pos_s", "pos_w", "raw_pos")),
    ("", False): (("pos",), ("pos_s", "pos_w", "x_w", "cls_w")),
    ("@e", False): (("pos",), ("pos_s", "pos_w", "x_w", "cls_w")),
    ("@2", False): (("pos",), ("pos_s", "pos_w")),
}


@pytest.mark.parametrize("phase,use_3d_loss", sorted(KEYS))
def test_lookahead_keys_are_the_table(phase, use_3d_loss):
    assert phase in ts.PHASES and len(ts.PHASES) == 3
    assert ts.lookahead_keys(phase, dict(ts.NTM_CFG, use_3d_loss=use_3d_loss)) == KEYS[phase, use_3d_loss]
    if use_3d_loss:
        assert ts.lookahead_keys(phase, {}) == KEYS[phase, True]                     # a cfg without the key: on
