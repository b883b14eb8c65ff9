"""VoteBatcher (geot_amd/openpoints/dataset/vote_batch.py): the validation batch with the `vote` transform list on top of the
`val` list -- against ValBatcher (exact), the vote transform restated in torch (exact), the host draws in the reference's
per-item order, device draws, a side stream."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_val_scans_gpu import DEV, _same, _set  # noqa: E402  (_same: torch.equal with NaN == NaN; a 1-vertex scan normalises to NaN)

pytestmark = pytest.mark.gpu
SIZES, JAWS = [5000, 1, 700, 2600, 65], [0, 1, 1, 0, 1]
M, IDS = 2048, [3, 0, 4, 1, 1, 2]                              # N < m for three scans, a 1-vertex scan, a scan twice
TENSORS = ("pos", "x", "y", "cls", "center", "scale", "scan_ids")
_cache = {}


def _dset():
    if "set" not in _cache:
        _cache["set"] = _set(SIZES, 700, cls=JAWS)
    return _cache["set"]


def _sel(seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.choice(SIZES[i], M, replace=SIZES[i] < M) for i in IDS]).astype(np.int64)


def _same_batches(a, b, keys=TENSORS + ("pos_search",)):
    for key in keys:
        assert _same(a[key], b[key]), key
    assert a["sizes"] == b["sizes"] and a["mandible"] == b["mandible"] and a["scans"] is b["scans"]
    for key in ("points", "labels"):
        assert all(p.data_ptr() == q.data_ptr() and p.shape == q.shape for p, q in zip(a[key], b[key])), key


def test_an_empty_vote_list_gives_the_val_batch():
    from geot_amd.openpoints.dataset import ValBatcher, VoteBatcher
    dset, sel = _dset(), _sel(1)
    want = ValBatcher(dset, M).batch(IDS, sel=sel, check=True)
    got = VoteBatcher(dset, M, vote=[]).batch(IDS, sel=sel, check=True)
    torch.cuda.synchronize()
    assert set(got) == set(want) | {"pos_search"}
    _same_batches(got, want, TENSORS)
    assert _same(got["pos_search"], got["pos"])
    assert got["pos"].is_contiguous() and got["x"].is_contiguous() and got["pos_search"].is_contiguous()


def test_the_configured_vote_scales_pos_and_leaves_x_and_the_search_points():
    from geot_amd.openpoints.dataset import ValBatcher, VoteBatcher
    dset, sel = _dset(), _sel(2)
    batcher = VoteBatcher(dset, M)                             # vote = [PointCloudScaling], the yaml's kwargs: scale in [0.9, 1.1]
    assert batcher.vote == ["PointCloudScaling"] and batcher.program.names[-1] == "PointCloudScaling"
    rng = np.random.default_rng(3)
    scales = (0.9 + 0.2 * rng.random((len(IDS), 3))).astype(np.float32)
    params = [[{}, {}, {"scale": s}] for s in scales]
    got = batcher.batch(IDS, sel=sel, params=params)
    want = ValBatcher(dset, M).batch(IDS, sel=sel)
    torch.cuda.synchronize()
    assert _same(got["pos"], got["pos_search"] * torch.from_numpy(scales).to(DEV)[:, None, :])
    assert not torch.equal(got["pos"], got["pos_search"])
    for key, other in (("x", "x"), ("pos_search", "pos"), ("y", "y"), ("cls", "cls"), ("center", "center"), ("scale", "scale"),
                       ("scan_ids", "scan_ids")):
        assert _same(got[key], want[other]), key
    with pytest.raises(RuntimeError, match="one entry per slot"):
        batcher.batch(IDS, sel=sel, params=params[:2])
    with pytest.raises(RuntimeError, match="idx must lie|at least one scan"):
        batcher.batch([len(SIZES)])
    with pytest.raises(IndexError, match="outside the scan"):
        batcher.batch([4], sel=np.full((1, M), 65, dtype=np.int64), check=True)


def test_host_draws_follow_the_reference_order_per_item():
    """Per item np.random.choice, then the vote list's draw (PointCloudScaling: torch.rand(3) * (hi - lo) + lo)."""
    from geot_amd.openpoints.dataset import TOOTH_VIEW_KWARGS, VoteBatcher
    dset = _dset()
    batcher = VoteBatcher(dset, M)
    np.random.seed(8)
    torch.manual_seed(8)
    got = batcher.batch(IDS)
    np.random.seed(8)
    torch.manual_seed(8)
    lo, hi = np.array(TOOTH_VIEW_KWARGS["scale"]).astype(np.float32)
    sel, params = [], []
    for i in IDS:
        sel.append(np.random.choice(SIZES[i], M, replace=SIZES[i] < M))
        params.append([{}, {}, {"scale": (torch.rand(3, dtype=torch.float32) * (hi - lo) + lo).numpy()}])
    want = batcher.batch(IDS, sel=np.stack(sel), params=params)
    torch.cuda.synchronize()
    _same_batches(got, want)
    other = batcher.batch(IDS)                                 # the next vote: another sample, another scale
    assert not torch.equal(other["pos_search"], got["pos_search"]) and not torch.equal(other["pos"], got["pos"])


def test_device_draws_are_reproducible_and_fresh_per_call():
    from geot_amd.openpoints.dataset import DeviceDraws, VoteBatcher
    dset = _dset()
    one = VoteBatcher(dset, M, draws=DeviceDraws(5, views=True))
    two = VoteBatcher(dset, M, draws=DeviceDraws(5, views=True))
    state = (np.random.get_state()[1].copy(), torch.get_rng_state().clone())
    a1, a2 = one.batch(IDS), one.batch(IDS)
    b1, b2 = two.batch(IDS), two.batch(IDS)
    torch.cuda.synchronize()
    assert np.array_equal(np.random.get_state()[1], state[0]) and torch.equal(torch.get_rng_state(), state[1])   # no host draw
    _same_batches(a1, b1)
    _same_batches(a2, b2)
    assert not torch.equal(a1["pos_search"], a2["pos_search"])
    ratio = a1["pos"] / a1["pos_search"]                       # one scale per slot and axis, within the configured bounds
    ok = torch.isfinite(ratio)
    assert float(ratio[ok].min()) >= 0.9 - 1e-5 and float(ratio[ok].max()) <= 1.1 + 1e-5 and not torch.equal(a1["pos"], a1["pos_search"])
    samples = VoteBatcher(dset, M, draws=DeviceDraws(5))       # the samples alone on the device: the same samples
    torch.manual_seed(1)
    c1 = samples.batch(IDS)
    assert _same(c1["pos_search"], a1["pos_search"]) and _same(c1["x"], a1["x"])


def test_a_side_stream_batch_equals_the_current_stream_batch():
    from geot_amd.openpoints.dataset import VoteBatcher
    dset, sel = _dset(), _sel(4)
    params = [[{}, {}, {"scale": np.array([0.95, 1.0, 1.05], np.float32)}]] * len(IDS)
    want = VoteBatcher(dset, M).batch(IDS, sel=sel, params=params)
    side = VoteBatcher(dset, M, stream=torch.cuda.Stream(DEV))
    got = side.batch(IDS, sel=sel, params=params)
    side.join(got)
    torch.cuda.synchronize()
    _same_batches(got, want)
