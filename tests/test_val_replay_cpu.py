"""The host half of the replayed whole-scan path (geot_amd/validation.py graph= / lookahead=, geot_amd/graph_eval.py): the
keywords' checks, GraphedForward's signature key, and the pass scheduler run on stub batchers -- no device anywhere."""
import itertools

import pytest
import torch


class _NoDevice(torch.nn.Module):
    """A model that fails the test when anything is asked of it: a refused keyword must raise before this."""

    def eval(self):
        raise AssertionError("the model was touched before the keywords were checked")

    def forward(self, data):
        raise AssertionError("the model ran before the keywords were checked")


def _calls(model, **kw):
    from geot_amd import validation as V
    cfg = dict(num_points=64, num_classes=17, num_votes=3)
    return (("validate_scans", lambda: V.validate_scans(model, object(), cfg, **kw)),
            ("validate_scans_voted", lambda: V.validate_scans_voted(model, object(), cfg, **kw)),
            ("vote_scans", lambda: V.vote_scans(model, object(), [0, 1], 3, **kw)))


# ------------------------------------------------------------------------------------------------ 1. the keywords
@pytest.mark.parametrize("kw,error", [
    (dict(graph=1), TypeError), (dict(graph="yes"), TypeError), (dict(graph=None), TypeError), (dict(graph=0), TypeError),
    (dict(lookahead=2.0), TypeError), (dict(lookahead="1"), TypeError), (dict(lookahead=None), TypeError),
    (dict(lookahead=-1), ValueError), (dict(lookahead=65), ValueError), (dict(graph=True, lookahead=-2), ValueError),
    (dict(graph=True, lookahead=1000), ValueError)])
def test_bad_switches_raise_before_any_device_call(kw, error):
    for name, run in _calls(_NoDevice(), **kw):
        with pytest.raises(error, match=name + ": (graph|lookahead|at most)"):
            run()


def test_lookahead_true_is_bounded_by_the_votes_and_a_wrapper_belongs_to_its_model():
    from geot_amd import validation as V
    from geot_amd.graph_eval import MAX_LOOKAHEAD, GraphedForward
    model = _NoDevice()
    with pytest.raises(ValueError, match="at most 64"):
        V.vote_scans(model, object(), [0], MAX_LOOKAHEAD + 1, lookahead=True)
    with pytest.raises(ValueError, match="at most 64"):
        V.validate_scans_voted(model, object(), {}, num_votes=MAX_LOOKAHEAD + 1, lookahead=True)
    with pytest.raises(ValueError, match="num_votes must be >= 1"):         # the existing check comes first
        V.validate_scans_voted(model, object(), {}, num_votes=0, lookahead=True)
    other = GraphedForward(torch.nn.Linear(2, 2))
    for name, run in _calls(model, graph=other):
        with pytest.raises(ValueError, match=name + ": the GraphedForward was built on another model"):
            run()
    for bad, error in ((True, TypeError), (2.0, TypeError), (None, TypeError), (-1, ValueError)):
        with pytest.raises(error, match="warmup"):
            GraphedForward(model, warmup=bad)


def test_what_the_switches_mean():
    from geot_amd.graph_eval import GraphedForward, graphed_forward
    from geot_amd.validation import _replay_switches as sw
    model = torch.nn.Linear(2, 2)
    assert sw(False, 0, 0, model, "x") == (0, None) and sw(False, False, 10, model, "x") == (0, None)
    assert sw(False, True, 10, model, "x") == (10, None) and sw(False, True, 0, model, "x") == (1, None)
    assert sw(False, 3, 10, model, "x") == (3, None) and sw(False, 64, 0, model, "x") == (64, None)
    mine = GraphedForward(model)
    assert sw(mine, 0, 0, model, "x") == (1, mine) and sw(mine, 4, 0, model, "x") == (4, mine)
    g, made = sw(True, 0, 10, model, "x")
    assert g == 1 and isinstance(made, GraphedForward) and made is graphed_forward(model)      # one wrapper per model, kept
    assert sw(True, True, 10, model, "x") == (10, made)


# ------------------------------------------------------------------------------------------------ 2. the signature key
def _batch(b, n, extra=False):
    data = {"pos": torch.zeros(b, n, 3), "x": torch.zeros(b, 3, n), "cls": torch.zeros(b, 1, dtype=torch.int64),
            "sizes": [5] * b, "scans": object()}
    if extra:
        data["pos_search"] = torch.zeros(b, n, 3)
    return data


def test_signature_key():
    from geot_amd.graph_eval import GraphedForward
    from geot_amd.openpoints.models.backbone.geometry import Geometry, IndexPlan
    sig = GraphedForward.signature

    def geometry(b, layout="cl", static=True):
        return Geometry(torch.zeros(b, 8, 3), (torch.zeros(b, 2, 4, 3), torch.zeros(b, 2, 3), None), IndexPlan([], [], None),
                        False, layout, static=static)
    a, b = _batch(2, 64), _batch(2, 64)
    b["pos"] += 1.0                                    # other values, other objects, other host entries: the same graph
    b["sizes"] = [7, 9]
    assert sig(a, geometry(2)) == sig(b, geometry(2)) and hash(sig(a, geometry(2))) == hash(sig(b, geometry(2)))
    assert sig(a) == sig(b)
    others = [sig(_batch(2, 65), geometry(2)), sig(_batch(1, 64), geometry(1)), sig(_batch(2, 64, extra=True), geometry(2)),
              sig(dict(a, cls=a["cls"].to(torch.int32)), geometry(2)), sig(a, geometry(2, layout="cf")), sig(a)]
    assert len(set(others + [sig(a, geometry(2))])) == len(others) + 1
    renamed = {("x2" if k == "x" else k): v for k, v in a.items()}
    assert sig(renamed, geometry(2)) != sig(a, geometry(2))


# ------------------------------------------------------------------------------------------------ 3. the pass scheduler
class _StubBatcher:
    def __init__(self):
        self.drawn, self.joined = [], []

    def batch(self, ids, draws=None):
        self.drawn.append((tuple(ids), draws))
        return {"pos": torch.zeros(len(ids), 4, 3), "call": len(self.drawn) - 1}

    def join(self, batch):
        self.joined.append(batch["call"])


class _StubRunner:
    """Records what _passes asks for: the geometry calls (which batches share one) and every forward pass."""

    def __init__(self, batcher):
        self.batcher, self.geometry, self.forwards = batcher, [], []

    def start(self, batches):
        assert all(b["call"] in self.batcher.joined for b in batches)        # positions are read: the batches were joined
        self.geometry.append(tuple(b["call"] for b in batches))
        return len(self.geometry) - 1

    def forward(self, data, share, next_batches):
        assert data["call"] in self.batcher.joined
        token = self.start(next_batches) if next_batches else None
        self.forwards.append((data["call"], share, len(self.batcher.drawn)))
        return "logits%d" % data["call"], token


def _today(groups, repeats):
    """Today's loop (lookahead = 0) on stubs: the batch() sequence and what it yields."""
    from geot_amd.validation import _passes
    batcher = _StubBatcher()
    out = [(d["call"], first, last) for d, _, first, last in _passes(lambda data: ("l", None, None), batcher, groups, repeats, "D")]
    return batcher.drawn, out


@pytest.mark.parametrize("sizes,repeats", [((2, 2, 1), 1), ((2, 2, 1), 3), ((3,), 4), ((2, 2), 2), ((1,), 1)])
def test_the_scheduler_draws_in_todays_order_and_shares_geometry_among_full_batches(sizes, repeats):
    from geot_amd.validation import _passes, pass_schedule
    ids = itertools.count()
    groups = [[next(ids) for _ in range(s)] for s in sizes]
    drawn_today, out_today = _today(groups, repeats)
    n = len(groups) * repeats
    assert len(drawn_today) == n and [c for c, _, _ in out_today] == list(range(n))
    full = [k for k in range(n) if sizes[k // repeats] == max(sizes)]
    for g in sorted({1, 2, repeats, n + 5}):
        batcher = _StubBatcher()
        runner = _StubRunner(batcher)
        out = []
        for data, logits, first, last in _passes(None, batcher, groups, repeats, "D", lookahead=g, runner=runner):
            assert logits == "logits%d" % data["call"]
            # at most g passes beyond the one in hand are drawn, and never fewer than today's one
            assert data["call"] + 1 <= len(batcher.drawn) <= data["call"] + 1 + g
            out.append((data["call"], first, last))
        assert batcher.drawn == drawn_today                         # the same batch() calls in the same order
        assert out == out_today                                     # the same passes with the same first / last flags
        assert sorted(batcher.joined) == list(range(n))             # every batch joined exactly once
        # which passes share a geometry call: the full batches of each chunk of g passes; the short ones in none
        want = [tuple(k for k in range(s, min(s + g, n)) if k in full) for s in range(0, n, g)]
        assert runner.geometry == [w for w in want if w]
        assert sorted(k for call in runner.geometry for k in call) == full
        # every full pass is handed its own slice of its chunk's call, a short one nothing
        for call, share, _ in runner.forwards:
            if call in full:
                token, index = share
                assert runner.geometry[token][index] == call
            else:
                assert share is None
        # a chunk's geometry starts with the forward pass of the last pass before it (the first: before anything runs)
        for call, _, drawn in runner.forwards:              # drawn: its own chunk, at a chunk's last pass the next one too
            boundary = (call + 1) % g == 0 and call + 1 < n
            assert drawn == min((call // g + 1) * g + (g if boundary else 0), n)
        ops = pass_schedule(sizes, repeats, g)[1]
        assert [a for op, a in ops if op == "draw"] == list(range(n)) == [a for op, a in ops if op == "forward"]
        for members in runner.geometry[1:]:
            at = ops.index(("geometry", members))
            before = [a for op, a in ops[:at] if op == "forward"]
            assert before == list(range(min(members) // g * g - 1))          # ... and that pass has not run yet


def test_the_schedule_names_its_passes():
    from geot_amd.validation import pass_schedule
    passes, ops = pass_schedule((2, 1), 2, 1)
    assert passes == [(0, True, False), (0, False, True), (1, True, False), (1, False, True)]
    assert ops == [("draw", 0), ("geometry", (0,)), ("draw", 1), ("geometry", (1,)), ("forward", 0), ("draw", 2), ("forward", 1),
                   ("draw", 3), ("forward", 2), ("forward", 3)]
    assert pass_schedule((), 3, 2) == ([], [])
    with pytest.raises(RuntimeError, match="lookahead >= 1"):
        pass_schedule((2,), 1, 0)


def test_a_slice_is_handed_over_for_the_concatenated_tensor_alone():
    from geot_amd.validation import _Shared

    class Geo:
        def slice(self, lo, hi):
            return (lo, hi)
    a, b = torch.zeros(2, 4, 3), torch.zeros(2, 4, 3)
    shared = _Shared(Geo(), [a, b])
    assert shared.slice_for(0, a) == (0, 2) and shared.slice_for(1, b) == (2, 4)
    assert shared.slice_for(0, b) is None and shared.slice_for(1, a.clone()) is None         # equal values are not enough
    a.add_(1.0)
    assert shared.slice_for(0, a) is None and shared.slice_for(1, b) == (2, 4)                # edited since
    assert _Shared(None, [a]).slice_for(0, a) is None
