"""The pass driver of geot_amd/validation.py (_passes) with a fake batcher and a fake model, no device: the look-ahead rule
-- join the current batch, queue the next one, then run the model -- over groups of scans run `repeats` times each.  The
host draws happen inside batch(), so this order is what makes seeded runs equal; test_vote_scans_gpu.py checks the same
sequences end to end through validate_scans, validate_scans_voted and vote_scans."""


def look_ahead_events(groups, repeats):
    """The events of the look-ahead loop over every group `repeats` times, written out independently of the driver."""
    passes = [list(g) for g in groups for _ in range(repeats)]
    events = [("batch", passes[0])] if passes else []
    for k, ids in enumerate(passes):
        events.append(("join", ids))
        if k + 1 < len(passes):
            events.append(("batch", passes[k + 1]))
        events.append(("model", ids))
    return events


class _Batcher:
    def __init__(self, events):
        self.events, self.draws = events, []

    def batch(self, ids, draws=None):
        self.events.append(("batch", list(ids)))
        self.draws.append(draws)
        return {"ids": list(ids)}

    def join(self, data):
        self.events.append(("join", data["ids"]))


def _run(groups, repeats, draws=None):
    from geot_amd.validation import _passes
    events = []
    batcher = _Batcher(events)

    def model(data):
        events.append(("model", data["ids"]))
        return ("logits of %s" % data["ids"], None, None)
    out = list(_passes(model, batcher, groups, repeats, draws))
    for data, logits, first, last in out:
        assert logits == "logits of %s" % data["ids"] and isinstance(first, bool) and isinstance(last, bool)
    return events, out, batcher


def test_one_pass_per_group():
    events, out, _ = _run([[0, 1], [2]], 1)
    assert events == [("batch", [0, 1]), ("join", [0, 1]), ("batch", [2]), ("model", [0, 1]), ("join", [2]), ("model", [2])]
    assert events == look_ahead_events([[0, 1], [2]], 1)
    assert [(d["ids"], first, last) for d, _, first, last in out] == [([0, 1], True, True), ([2], True, True)]


def test_every_group_is_repeated_before_the_next_one():
    events, out, _ = _run([[0, 1], [2]], 3)
    assert [d["ids"] for d, _, _, _ in out] == [[0, 1]] * 3 + [[2]] * 3
    assert events == look_ahead_events([[0, 1], [2]], 3)
    assert [e[0] for e in events] == ["batch"] + ["join", "batch", "model"] * 5 + ["join", "model"]
    assert [e[1] for e in events if e[0] == "batch"] == [e[1] for e in events if e[0] == "model"] == [[0, 1]] * 3 + [[2]] * 3
    assert [k for k, p in enumerate(out) if p[2]] == [0, 3] and [k for k, p in enumerate(out) if p[3]] == [2, 5]


def test_one_group_is_the_vote_scans_form():
    events, out, _ = _run([[4]], 2)
    assert events == [("batch", [4]), ("join", [4]), ("batch", [4]), ("model", [4]), ("join", [4]), ("model", [4])]
    assert [(first, last) for _, _, first, last in out] == [(True, False), (False, True)]


def test_no_group_calls_nothing():
    events, out, batcher = _run([], 3)
    assert events == [] and out == [] and batcher.draws == []


def test_draws_reach_every_batch_call_unchanged():
    token = object()
    _, _, batcher = _run([[0, 1], [2]], 2, draws=token)
    assert len(batcher.draws) == 4 and all(d is token for d in batcher.draws)
    _, _, batcher = _run([[0, 1], [2]], 2)
    assert batcher.draws == [None] * 4
