"""Covering passes on the GPU, nothing with a tolerance: geot_sample_draw_cover against the numpy restatement
(tests/_scan_cover_ref.py) bit for bit; geot_scan_cover through the C ABI against torch's index_copy_ / index_add_ of the
owners' soft-max rows (one writer per row and one fp32 addition per round, so the sums are exact), its arg-max against
torch.argmax, its counts against SegMetrics.update, and its refusals; then end to end -- a model that echoes the sampled
labels gets every vertex of every scan right through cover_scans and validate_scans_covered, interpolate= / refine= / graph= /
lookahead= against the calls they are made of."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scan_cover_ref as cref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SET, FINISH = 1, 2
SEED = 0xC0FFEE_0000_0001
C = 17
M = 512
SIZES, JAWS = [300, 700, 1300], [0, 1, 0]           # m = 512: P = 3, one scan with n < m, one whose last pass wraps
_made = {}


def _set(name, sizes, jaws=None, classes=C):
    """Scans of `sizes` vertices in scan coordinates with labels in [0, classes), made once."""
    if name not in _made:
        from geot_amd.openpoints.dataset import DeviceScanSet
        rng = np.random.default_rng(len(sizes) * 1000 + sizes[-1])
        pts = [(rng.standard_normal((n, 3)) * 9.0 + np.array([4.0, -7.0, 2.0])).astype(np.float32) for n in sizes]
        labs = [((np.arange(n) * 7 // 13 + i) % classes).astype(np.int32) for i, n in enumerate(sizes)]
        _made[name] = DeviceScanSet(pts, labs, cls=jaws, device=DEV)
    return _made[name]


def _scans():
    return _set("cover", SIZES, JAWS)


# ------------------------------------------------------------------------------------------------ a. geot_sample_draw_cover
DRAW_SIZES = [1, 2, 5, 16, 17, 1024, 1025, 40001]
# (m, scan ids; 99 lies outside the set): n = 1, n = 2 and n = m; n = m + 1, n < m and a slot outside the set; b = 10, b = 11
# (unbalanced halves) and b = 16; n < m beside the set's largest scan
DRAW_CASES = [(16, [0, 1, 3]), (16, [4, 2, 99]), (512, [5, 6, 7]), (512, [7, 99, 2])]


@pytest.mark.parametrize("m,ids", DRAW_CASES)
def test_sample_draw_cover_is_the_restatement(m, ids):
    from geot_amd.openpoints.dataset import sample_draw, sample_draw_cover
    scans = _set("draw", DRAW_SIZES)
    sizes = [DRAW_SIZES[i] if i < len(DRAW_SIZES) else 0 for i in ids]
    last = max(cref.cover_passes(n, m) for n in sizes if n) - 1
    base = (1 << 63) + 11
    seen = [np.zeros(n, dtype=np.int64) for n in sizes]
    for p in sorted({0, last, last + 1, (1 << 31) - 1}):
        sel, bad = sample_draw_cover(scans, ids, m, SEED, base, p)
        want_sel, want_bad = cref.sample_draw_cover_ref(sizes, m, SEED, base, p)
        assert sel.dtype == torch.int64 and tuple(sel.shape) == (3, m) and bad.dtype == torch.int32
        assert np.array_equal(bad.cpu().numpy(), want_bad) and want_bad.tolist() == [0 if n else 2 for n in sizes]
        assert np.array_equal(sel.cpu().numpy(), want_sel), (p, int((sel.cpu().numpy() != want_sel).sum()))
    for p in range(last + 1):                               # all passes of the cover: every vertex of every slot named once
        sel = sample_draw_cover(scans, ids, m, SEED, base, p)[0].cpu().numpy()
        for s, n in enumerate(sizes):
            if n:
                np.add.at(seen[s], sel[s][cref.owners(n, m, p)], 1)
    assert all((count == 1).all() for count in seen)
    # pass 0 of a scan with n >= m is geot_sample_draw's row for the same id
    plain = sample_draw(scans, ids, m, SEED, base)[0]
    first = sample_draw_cover(scans, ids, m, SEED, base, 0)[0]
    for s, n in enumerate(sizes):
        assert n < m or torch.equal(plain[s], first[s])
    with pytest.raises(RuntimeError, match="pass"):
        sample_draw_cover(scans, ids, m, SEED, base, -1)


# ------------------------------------------------------------------------------------------------ b. geot_scan_cover
def _cover(scans, ids, sel, prob, p, acc, mode, c, pred=None, counts=None, with_labels=True, raw=False, sizes=None, over=()):
    """One geot_scan_cover call through the C ABI; over: arguments replaced by name (the refusals); raw: the error code."""
    from geot_amd import _lib
    from geot_amd.ext._common import call, ptr
    from geot_amd.validation import scan_work_table
    sizes = [scans.sizes[i] for i in ids] if sizes is None else sizes       # (given: the rows of a slot outside the set)
    ids_dev = torch.tensor(ids, dtype=torch.int64, device=DEV)
    work = torch.from_numpy(scan_work_table(sizes)).to(DEV)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(sizes)[:-1]]), dtype=torch.int64, device=DEV)
    args = dict(b=len(ids), c=c, n=sel.shape[1], n_scans=len(scans), total=int(scans.points.shape[0]),
                labels=ptr(scans.labels) if with_labels else None, offsets=ptr(scans.offsets), scan_ids=ptr(ids_dev), sel=ptr(sel),
                prob=ptr(prob), pass_no=p, n_work=int(work.shape[0]), work=ptr(work), out_offsets=ptr(offs), acc=ptr(acc), mode=mode,
                pred=ptr(pred), counts=ptr(counts))
    assert set(dict(over)) <= set(args)
    args.update(over)
    if raw:
        err = _lib.load().geot_scan_cover(*args.values(), torch.cuda.current_stream(DEV).cuda_stream)
    else:
        err = call("geot_scan_cover", DEV, *args.values())
    torch.cuda.synchronize()
    return err


def _probabilities(c, b, m, seed):
    """(b, c, m) soft-max rows; for c >= 2 with a NaN row and a tie planted at samples 3 and 5 of every slot (owners of pass 0)."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    prob = torch.softmax(torch.randn((b, c, m), generator=gen) * 3.0, dim=1)
    if c >= 2:
        prob[:, :, 3] = 0.25 / c
        prob[:, c - 1, 3] = float("nan")                    # a NaN wins, wherever it stands
        prob[:, :, 5] = 0.1 / c
        prob[:, c // 2, 5] = prob[:, c - 1, 5] = 0.45       # a tie: the first maximum
    return prob.contiguous().to(DEV)


def _same(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


@pytest.mark.parametrize("c", [1, 17, 32])
def test_scan_cover_is_index_copy_and_index_add(c):
    from geot_amd.validation import SegMetrics
    scans = _set("cover%d" % c, SIZES, JAWS, classes=c)
    ids, b, slots = [2, 0, 1], 3, c * (c + 1) + 1
    sizes = [scans.sizes[i] for i in ids]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    total, passes = int(starts[-1]), max(cref.cover_passes(n, M) for n in sizes)
    assert passes == 3
    acc = torch.full((total, c), -3.0, device=DEV)           # SET: what is there does not matter, and non-owners leave it
    want = torch.full((total, c), -3.0, device=DEV)
    pred = torch.full((total,), -1, dtype=torch.int64, device=DEV)
    counts = torch.zeros((b, slots), dtype=torch.int64, device=DEV)
    planted = []
    for rnd in range(2):
        for p in range(passes):
            sel_host = cref.sample_draw_cover_ref(sizes, M, SEED, 40 + 3 * rnd, p)[0]
            sel = torch.from_numpy(sel_host).to(DEV)
            prob = _probabilities(c, b, M, 100 * c + 10 * rnd + p)
            rows, values = [], []
            for s, n in enumerate(sizes):
                own = torch.from_numpy(cref.owners(n, M, p)).to(DEV)
                rows.append(int(starts[s]) + sel[s][own])
                values.append(prob[s][:, own].t())
                if rnd == 0 and p == 0:
                    planted.append((int(starts[s]) + int(sel_host[s][3]), int(starts[s]) + int(sel_host[s][5])))
            rows, values = torch.cat(rows), torch.cat(values).contiguous()
            assert rows.unique().numel() == rows.numel()
            if rnd == 0:
                want.index_copy_(0, rows, values)
            else:
                want.index_add_(0, rows, values)             # unique rows: one fp32 addition per element
            last = rnd == 1 and p + 1 == passes
            _cover(scans, ids, sel, prob, p, acc, (SET if rnd == 0 else 0) | (FINISH if last else 0), c,
                   pred=pred if last else None, counts=counts if last else None)
            assert _same(acc, want), (rnd, p, int((acc != want).sum()))
            if rnd == 0 and p == 0:
                assert int((acc == -3.0).all(1).sum()) == total - rows.numel() > 0       # non-owners wrote nothing
    assert not (want == -3.0).any()
    assert torch.equal(pred, torch.argmax(want, dim=1))
    if c >= 2:
        for nan_row, tie_row in planted:                     # (round 1 added finite values to both rows)
            assert int(pred[nan_row]) == c - 1 and torch.isnan(want[nan_row, c - 1])
    # round 0 alone, finished: the planted tie takes the first maximum
    acc0 = torch.empty((total, c), device=DEV)
    pred0 = torch.full((total,), -1, dtype=torch.int64, device=DEV)
    want0 = torch.empty((total, c), device=DEV)
    for p in range(passes):
        sel = torch.from_numpy(cref.sample_draw_cover_ref(sizes, M, SEED, 40, p)[0]).to(DEV)
        prob = _probabilities(c, b, M, 100 * c + p)
        for s, n in enumerate(sizes):
            own = torch.from_numpy(cref.owners(n, M, p)).to(DEV)
            want0.index_copy_(0, int(starts[s]) + sel[s][own], prob[s][:, own].t().contiguous())
        _cover(scans, ids, sel, prob, p, acc0, SET | (FINISH if p + 1 == passes else 0), c, pred=pred0 if p + 1 == passes else None)
    assert _same(acc0, want0) and torch.equal(pred0, torch.argmax(want0, dim=1))
    if c >= 2:
        for nan_row, tie_row in planted:
            assert int(pred0[tie_row]) == c // 2 and int(pred0[nan_row]) == c - 1
    # the counts are SegMetrics.update's on the same labels
    metrics = SegMetrics(c, DEV)
    labels = [scans.labels[int(scans.offsets[i]):int(scans.offsets[i + 1])] for i in ids]
    metrics.update(list(torch.split(pred, sizes)), labels, [0] * b)
    assert torch.equal(counts, metrics.counts[:b]) and int(counts.sum()) == total
    again = counts.clone()                                   # counts are ADDED to; FINISH alone re-reads the sums
    _cover(scans, ids, sel, prob, passes, acc, FINISH, c, counts=again)
    assert torch.equal(again, 2 * counts) and _same(acc, want)


def test_scan_cover_refusals_launch_nothing():
    scans = _scans()
    ids, c = [0, 1, 2], C
    total = sum(SIZES)
    sel = torch.from_numpy(cref.sample_draw_cover_ref(SIZES, M, SEED, 1, 0)[0]).to(DEV)
    prob = _probabilities(c, 3, M, 5)
    acc = torch.full((total, c), -3.0, device=DEV)
    pred = torch.full((total,), -1, dtype=torch.int64, device=DEV)
    counts = torch.zeros((3, c * (c + 1) + 1), dtype=torch.int64, device=DEV)
    from geot_amd.ext._common import ptr
    bad = [dict(pass_no=-1), dict(sel=None), dict(prob=None), dict(acc=None), dict(out_offsets=None), dict(offsets=None),
           dict(scan_ids=None), dict(mode=4), dict(mode=SET | 8), dict(c=0), dict(c=33), dict(n=0), dict(b=-1), dict(b=65536),
           dict(n_scans=0), dict(total=0), dict(n_work=-1), dict(work=None), dict(work=ptr(sel) + 4)]
    for over in bad:
        assert _cover(scans, ids, sel, prob, 0, acc, SET, c, raw=True, over=over) == 1, over
    for mode, kw in ((SET, dict(pred=pred)), (SET, dict(counts=counts)), (0, dict(pred=pred, counts=counts)),
                     (SET | FINISH, dict(counts=counts, with_labels=False))):
        assert _cover(scans, ids, sel, prob, 0, acc, mode, c, raw=True, **kw) == 1, (mode, list(kw))
    with pytest.raises(RuntimeError, match="geot_scan_cover failed.*hipError 1"):
        _cover(scans, ids, sel, prob, -1, acc, SET, c)
    assert bool((acc == -3.0).all()) and bool((pred == -1).all()) and int(counts.sum()) == 0
    for over in (dict(b=0), dict(n_work=0)):                 # nothing to do
        assert _cover(scans, ids, sel, prob, 0, acc, SET, c, raw=True, over=over) == 0
    assert bool((acc == -3.0).all())
    # a slot outside the set is skipped whole: its rows stay, the others are written
    assert _cover(scans, [0, 7, 2], sel, prob, 0, acc, SET, c, raw=True, sizes=SIZES) == 0
    assert bool((acc[:300] != -3.0).all()) and bool((acc[300:1000] == -3.0).all()) and int((acc[1000:] != -3.0).all(1).sum()) == M


# ------------------------------------------------------------------------------------------------ c. the echo test
class Echo(torch.nn.Module):
    """Ten times the one-hot of the sampled points' own labels: a model that is right about every point it is shown."""

    def forward(self, data, geometry=None):
        return 10.0 * torch.nn.functional.one_hot(data["y"], C).permute(0, 2, 1).float().contiguous(), None, None


class Waves(torch.nn.Module):
    """Smooth, sample-dependent logits from the positions alone (deterministic: the same batch gives the same bits)."""

    def forward(self, data, geometry=None):
        k = torch.arange(1, C + 1, device=data["pos"].device, dtype=torch.float32).view(1, C, 1)
        pos = data["pos"].transpose(1, 2)
        return (torch.sin(pos[:, :1] * k) + torch.cos(pos[:, 1:2] * (k * 0.5)) * pos[:, 2:3]).contiguous(), None, None


def _truth(scans, idx):
    return [scans.labels[int(scans.offsets[i]):int(scans.offsets[i + 1])].to(torch.int64).view(1, -1) for i in idx]


@pytest.mark.parametrize("kind", ["val", "vote"])
def test_an_echo_model_labels_every_vertex_right(kind):
    from geot_amd.openpoints.dataset import DeviceDraws, ValBatcher, VoteBatcher
    from geot_amd.validation import ScanCover, cover_scans, validate_scans_covered
    scans = _scans()
    batcher = (ValBatcher if kind == "val" else VoteBatcher)(scans, M, C, draws=DeviceDraws(3, views=kind == "vote"))
    idx = [1, 2, 0]
    preds = cover_scans(Echo(), batcher, idx)
    assert batcher.draws.counter == 3
    want = _truth(scans, idx)
    assert len(preds) == 3 and all(p.dtype == torch.int64 and p.shape == w.shape and torch.equal(p, w) for p, w in zip(preds, want))
    preds = cover_scans(Echo(), batcher, [0], rounds=2)      # one scan below m: one pass per round
    assert torch.equal(preds[0], _truth(scans, [0])[0]) and batcher.draws.counter == 5
    cfg = dict(num_points=M, num_classes=C, epoch=1, epochs=1)
    out = validate_scans_covered(Echo(), batcher, cfg, rounds=2, batch_size=2)
    assert all(float(v) == 1.0 for v in out), out
    if kind == "val":                                         # from the set itself: a ValBatcher is built on it
        out = validate_scans_covered(Echo(), scans, cfg, draws=DeviceDraws(8), batch_size=3)
        assert all(float(v) == 1.0 for v in out), out
        # the batches by hand: ScanCover's mean probabilities are the one-hot soft-max rows
        cover, model = None, Echo()
        for data in batcher.cover(idx, rounds=2):
            cover = ScanCover(data, C) if cover is None else cover
            p, passes, rnd = data["cover"]
            got = cover.add(model(data)[0], data, last=(rnd, p) == (1, passes - 1), want_pred=(rnd, p) == (1, passes - 1))
        assert all(torch.equal(g, w) for g, w in zip(got, want))
        for prob, w in zip(cover.probabilities(), want):
            assert torch.equal(prob.argmax(1), w[0]) and bool((prob.max(1).values > 0.99).all())
        with pytest.raises(RuntimeError, match="last pass has been added"):
            cover.add(model(data)[0], data)


# ------------------------------------------------------------------------------------------------ d. further end to end
def test_interpolate_refine_and_repeatability():
    from geot_amd.openpoints.dataset import DeviceDraws, ValBatcher
    from geot_amd.validation import ScanVotes, cover_scans, refine_scans
    scans, model, idx = _scans(), Waves(), [2, 1]
    batcher = ValBatcher(scans, M, C)
    with pytest.raises(ValueError, match="DeviceDraws"):
        cover_scans(model, batcher, idx)
    base = cover_scans(model, batcher, idx, draws=DeviceDraws(21, counter=5))
    again = cover_scans(model, batcher, idx, draws=DeviceDraws(21, counter=5))
    other = cover_scans(model, batcher, idx, draws=DeviceDraws(22, counter=5))
    assert all(torch.equal(a, b) for a, b in zip(base, again))           # the same seed and counter: the same labels
    assert any(not torch.equal(a, b) for a, b in zip(base, other))
    assert len({int(v) for p in base for v in p.unique()}) >= 3
    # refine=10 is refine_scans on the un-refined result
    refined = cover_scans(model, batcher, idx, draws=DeviceDraws(21, counter=5), refine=10)
    data = batcher.batch(idx, draws=DeviceDraws(0))
    want = refine_scans([p.clone() for p in base], data, 10, num_classes=C)
    assert all(torch.equal(a, b) for a, b in zip(refined, want))
    # interpolate=True is ScanVotes.add fed the same batches by hand
    got = cover_scans(model, batcher, idx, rounds=2, interpolate=True, draws=DeviceDraws(21, counter=5))
    votes = None
    batches = list(batcher.cover(idx, rounds=2, draws=DeviceDraws(21, counter=5)))
    assert len(batches) == 6
    with torch.no_grad():
        for k, data in enumerate(batches):
            votes = ScanVotes(data, C) if votes is None else votes
            by_hand = votes.add(model(data)[0], data, last=k == 5, want_pred=k == 5)
    assert all(torch.equal(a, b) for a, b in zip(got, by_hand))


def test_graph_and_lookahead_give_the_eager_bits():
    from test_val_replay_gpu import CFG, N, _model, _scans as replay_scans
    from geot_amd.graph_eval import GraphedForward
    from geot_amd.openpoints.dataset import DeviceDraws, ValBatcher
    from geot_amd.validation import cover_scans, validate_scans_covered
    scans, model, idx = replay_scans(), _model(), [0, 1]                  # 5003 and 9001 vertices, N = 4096: P = 3
    batcher = ValBatcher(scans, N)

    def run(**kw):
        return cover_scans(model, batcher, idx, draws=DeviceDraws(17), **kw)
    base = run()
    assert [tuple(p.shape) for p in base] == [(1, 5003), (1, 9001)]
    for got in (run(lookahead=True), run(lookahead=2)):
        assert all(torch.equal(a, b) for a, b in zip(base, got))
    wrapper = GraphedForward(model, warmup=1)
    for _ in range(2):                                                   # warm-up and capture, then replays alone
        got = run(graph=wrapper, lookahead=True)
        assert all(torch.equal(a, b) for a, b in zip(base, got))
    assert wrapper.replays >= 3 and not wrapper.refused
    eager = validate_scans_covered(model, scans, CFG, draws=DeviceDraws(4), indices=[0, 1, 2])
    replayed = validate_scans_covered(model, scans, CFG, draws=DeviceDraws(4), indices=[0, 1, 2], graph=wrapper, lookahead=True)
    assert all(type(x) is type(y) and np.array_equal(x, y, equal_nan=True) for x, y in zip(eager, replayed)), (eager, replayed)
