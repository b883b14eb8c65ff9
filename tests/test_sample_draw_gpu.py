"""GPU suite of geot_sample_draw (geot_amd/csrc/sample_draw.hip; geot_amd/openpoints/dataset/sample_draw.py) and of the three
batchers' `draws=` mode, against the numpy restatement of the contract (tests/_sample_draw_ref.py).  The kernel is integer
arithmetic: every element of every output is compared for equality, nothing is sampled and there is no tolerance."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sample_draw_ref as sd  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEED = 0x1234567
# each side of the width changes at 2^9 (the 10-bit floor), 2^10 and 2^16, the toy sizes, and one scan of real size
SCAN_SIZES = (1, 2, 5, 7, 511, 512, 513, 1000, 1024, 1025, 65536, 65537, 200003)
# both branches in one grid; n == m at 1, 2, 5, 513; n == m - 1 at 2 and 513; 257: no multiple of the block
M_VALUES = (1, 2, 5, 200, 257, 513, 24000)
INVALID = 1            # hipErrorInvalidValue


def _scan_set(sizes, seed=0):
    from geot_amd.openpoints.dataset import DeviceScanSet
    rng = np.random.default_rng(seed)
    return DeviceScanSet([rng.standard_normal((n, 3)).astype(np.float32) for n in sizes],
                         [rng.integers(0, 17, n).astype(np.int32) for n in sizes], cls=[i % 2 for i in range(len(sizes))], device=DEV)


@functools.lru_cache(maxsize=None)
def _mixed_set():
    return _scan_set(SCAN_SIZES)


@functools.lru_cache(maxsize=None)
def _mixed_slots():
    """Every scan twice and some a third time, in shuffled order (fixed)."""
    rng = np.random.default_rng(11)
    slots = list(range(len(SCAN_SIZES))) * 2 + [0, 4, 7, 10, 12]
    rng.shuffle(slots)
    return tuple(int(s) for s in slots)


@pytest.mark.parametrize("m", M_VALUES)
def test_mixed_sizes_in_one_launch_equal_the_restatement(m):
    from geot_amd.openpoints.dataset import sample_draw
    scans, slots = _mixed_set(), _mixed_slots()
    want_sel, want_bad = sd.sample_draw_ref([SCAN_SIZES[s] for s in slots], m, SEED, 1000)
    sel, bad = sample_draw(scans, slots, m, SEED, 1000)
    assert sel.dtype == torch.int64 and bad.dtype == torch.int32 and tuple(sel.shape) == (len(slots), m) and sel.is_cuda
    got = sel.cpu().numpy()
    wrong = np.flatnonzero((got != want_sel).any(1))
    assert wrong.size == 0, "m = %d: slots %s (sizes %s) differ" % (m, wrong.tolist(), [SCAN_SIZES[slots[i]] for i in wrong])
    assert np.array_equal(bad.cpu().numpy(), want_bad) and not want_bad.any()
    for i, s in enumerate(slots):               # what the rows are for: m distinct vertices of the scan where it has them
        n = SCAN_SIZES[s]
        assert got[i].min() >= 0 and got[i].max() < n
        if n >= m:
            assert np.unique(got[i]).size == m


def test_null_scan_ids_are_the_scans_in_order():
    from geot_amd.openpoints.dataset import sample_draw
    scans = _mixed_set()
    a_sel, a_bad = sample_draw(scans, None, 257, SEED, 5)
    b_sel, b_bad = sample_draw(scans, list(range(len(SCAN_SIZES))), 257, SEED, 5)
    c_sel, _ = sample_draw(scans, torch.arange(len(SCAN_SIZES), device=DEV), 257, SEED, 5)
    assert torch.equal(a_sel, b_sel) and torch.equal(a_bad, b_bad) and torch.equal(a_sel, c_sel)
    want, _ = sd.sample_draw_ref(SCAN_SIZES, 257, SEED, 5)
    assert np.array_equal(a_sel.cpu().numpy(), want)


def test_a_slot_outside_the_set_is_flagged_and_harms_no_other():
    from geot_amd.openpoints.dataset import sample_draw
    scans = _mixed_set()
    ids = [7, -1, 3, len(SCAN_SIZES), 12, 2 ** 40, 0]
    sizes = [SCAN_SIZES[i] if 0 <= i < len(SCAN_SIZES) else 0 for i in ids]
    want_sel, want_bad = sd.sample_draw_ref(sizes, 300, SEED, 77)
    sel, bad = sample_draw(scans, ids, 300, SEED, 77)
    assert bad.cpu().tolist() == [0, 2, 0, 2, 0, 2, 0] == want_bad.tolist()
    assert np.array_equal(sel.cpu().numpy(), want_sel) and not want_sel[[1, 3, 5]].any()
    # NULL scan_ids with more slots than scans: the slots past the set are unusable, the others are drawn
    from geot_amd import _lib
    lib, s, m = _lib.load(), len(SCAN_SIZES) + 2, 64
    out = torch.full((s, m), -7, dtype=torch.int64, device=DEV)
    flags = torch.full((s,), -7, dtype=torch.int32, device=DEV)
    err = lib.geot_sample_draw(s, m, len(scans), int(scans.points.shape[0]), scans.offsets.data_ptr(), None, SEED, 0,
                               out.data_ptr(), flags.data_ptr(), torch.cuda.current_stream(DEV).cuda_stream)
    assert err == 0
    want_sel, want_bad = sd.sample_draw_ref(list(SCAN_SIZES) + [0, 0], m, SEED, 0)
    assert np.array_equal(out.cpu().numpy(), want_sel) and np.array_equal(flags.cpu().numpy(), want_bad)
    # a table entry that is unusable for another reason: an empty scan, offsets that run backwards or past the total
    offsets = torch.tensor([0, 10, 10, 30, 20, 50, 70], dtype=torch.int64, device=DEV)       # total = 60 below
    out = torch.full((6, 8), -7, dtype=torch.int64, device=DEV)
    flags = torch.full((6,), -7, dtype=torch.int32, device=DEV)
    assert lib.geot_sample_draw(6, 8, 6, 60, offsets.data_ptr(), None, SEED, 3, out.data_ptr(), flags.data_ptr(),
                                torch.cuda.current_stream(DEV).cuda_stream) == 0
    want_sel, want_bad = sd.sample_draw_ref([10, 0, 20, 0, 30, 0], 8, SEED, 3)
    assert np.array_equal(out.cpu().numpy(), want_sel) and flags.cpu().tolist() == [0, 2, 0, 2, 0, 2] == want_bad.tolist()


def test_bad_arguments_return_the_error_without_a_launch():
    from geot_amd import _lib
    scans = _mixed_set()
    lib = _lib.load()
    out = torch.full((4, 16), -7, dtype=torch.int64, device=DEV)
    flags = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    good = [4, 16, len(scans), int(scans.points.shape[0]), scans.offsets.data_ptr(), None, SEED, 0, out.data_ptr(), flags.data_ptr()]
    for at, value in ((0, 0), (0, -1), (0, 65536), (1, 0), (1, -3), (2, 0), (3, 0), (4, None), (8, None), (9, None)):
        args = list(good)
        args[at] = value
        assert lib.geot_sample_draw(*args, stream) == INVALID, (at, value)
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((flags == -7).all())
    assert lib.geot_sample_draw(*good, stream) == 0
    torch.cuda.synchronize()
    assert bool((flags == 0).all()) and int(out.min()) >= 0


@pytest.mark.parametrize("base", [2 ** 32 - 3, 2 ** 64 - 2])
def test_the_draw_counter_crosses_its_word_boundaries(base):
    """draw_base + slot runs over 2^32 - 1 into the high counter word, and wraps at 2^64."""
    from geot_amd.openpoints.dataset import sample_draw
    scans = _mixed_set()
    ids = [7, 7, 7, 7, 1, 7]                     # n = 1000 five times (rows must differ) and one with replacement
    sel, bad = sample_draw(scans, ids, 200, SEED, base)
    want, _ = sd.sample_draw_ref([SCAN_SIZES[i] for i in ids], 200, SEED, base)
    assert np.array_equal(sel.cpu().numpy(), want) and not bad.any()
    assert len({want[i].tobytes() for i in (0, 1, 2, 3, 5)}) == 5
    high = 2 ** 64 + SEED                        # the seed is taken modulo 2^64, and its high word is part of the key
    again, _ = sample_draw(scans, ids, 200, high, base)
    assert torch.equal(again, sel)
    other, _ = sample_draw(scans, ids, 200, SEED + (1 << 32), base)
    want_other, _ = sd.sample_draw_ref([SCAN_SIZES[i] for i in ids], 200, SEED + (1 << 32), base)
    assert np.array_equal(other.cpu().numpy(), want_other) and not np.array_equal(want_other, want)


def test_ctypes_and_the_compiled_binding_return_the_same_tensors():
    from geot_amd.ext import _common
    from geot_amd.openpoints.dataset import sample_draw
    scans, slots = _mixed_set(), _mixed_slots()
    assert _common.dispatcher() is not None and hasattr(_common.dispatcher(), "geot_sample_draw")
    saved = _common._dispatch
    out = {}
    try:
        for name, disp in (("dispatcher", saved), ("ctypes", False)):
            _common._dispatch = disp
            out[name] = sample_draw(scans, slots, 257, 2 ** 64 - 5, 2 ** 64 - 9)      # values past 2^63 cross both bindings
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                on_side = sample_draw(scans, slots, 257, 2 ** 64 - 5, 2 ** 64 - 9)
            side.synchronize()
            assert torch.equal(on_side[0], out[name][0]) and torch.equal(on_side[1], out[name][1])
    finally:
        _common._dispatch = saved
    assert torch.equal(out["dispatcher"][0], out["ctypes"][0]) and torch.equal(out["dispatcher"][1], out["ctypes"][1])
    want, _ = sd.sample_draw_ref([SCAN_SIZES[s] for s in slots], 257, 2 ** 64 - 5, 2 ** 64 - 9)
    assert np.array_equal(out["ctypes"][0].cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ the batchers
BATCH_SIZES = (3000, 700, 1500, 1024)       # m = 1024: without replacement, with (700), and n == m
M_BATCH = 1024


def _same(a, b, key=""):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape, key
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b), key
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), key
        for x, y in zip(a, b):
            _same(x, y, key)
    elif key == "scans":
        assert a is b
    else:
        assert a == b, key


def _same_batch(a, b):
    assert set(a) == set(b)
    for k in a:
        _same(a[k], b[k], k)


def _choice_state(sizes, m, seed):
    """numpy's global state after seeding and one np.random.choice per item, the reference's statement."""
    np.random.seed(seed)
    for n in sizes:
        np.random.choice(n, m, replace=n < m)
    return np.random.get_state()


def _state_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and tuple(a[2:]) == tuple(b[2:])


@pytest.fixture()
def no_choice(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("np.random.choice was called in the device-draw mode")
    yield lambda: monkeypatch.setattr(np.random, "choice", refuse)


def test_fixmatch_batcher_draws_on_the_device(no_choice):
    from geot_amd.openpoints.dataset import DeviceDraws, FixMatchBatcher, draw_view_params
    lab, unl = _scan_set(BATCH_SIZES, 1), _scan_set(BATCH_SIZES[::-1], 2)
    batcher = FixMatchBatcher(lab, unl, M_BATCH)
    idx_l, idx_u = [1, 3, 0], [0, 2, 3, 1]
    torch.manual_seed(3)
    np.random.seed(3)
    params = [draw_view_params("train") for _ in idx_l] + [(draw_view_params("train_w"), draw_view_params("train_s")) for _ in idx_u]
    sizes = [BATCH_SIZES[i] for i in idx_l] + [BATCH_SIZES[::-1][i] for i in idx_u]
    # draws=None: numpy's global stream is consumed exactly as before
    np.random.seed(9)
    host = batcher.batch(idx_l, idx_u, params=params, check=True)
    assert _state_equal(np.random.get_state(), _choice_state(sizes, M_BATCH, 9))
    # DeviceDraws: the restatement's rows, labelled slots first, one id per slot; numpy is not touched
    rows, _ = sd.sample_draw_ref(sizes, M_BATCH, SEED, 40)
    want = batcher.batch(idx_l, idx_u, sel_l=rows[:3], sel_u=rows[3:], params=params, check=True)
    before = np.random.get_state()
    no_choice()
    draws = DeviceDraws(SEED, 40)
    got = batcher.batch(idx_l, idx_u, params=params, check=True, draws=draws)
    assert draws.counter == 47 and _state_equal(np.random.get_state(), before)
    _same_batch(got[0], want[0])
    _same_batch(got[1], want[1])
    assert not torch.equal(got[0]["y"], host[0]["y"])
    # two fresh objects give equal batches; the next batch of one continues with the next ids
    again = batcher.batch(idx_l, idx_u, params=params, draws=DeviceDraws(SEED, 40))
    _same_batch(again[0], want[0])
    _same_batch(again[1], want[1])
    nxt = batcher.batch(idx_l, idx_u, params=params, draws=draws)
    rows2, _ = sd.sample_draw_ref(sizes, M_BATCH, SEED, 47)
    want2 = batcher.batch(idx_l, idx_u, sel_l=rows2[:3], sel_u=rows2[3:], params=params)
    _same_batch(nxt[1], want2[1])
    # draw() hands out the device tensor; an explicit sel_l wins for its rows, both given take no id
    resumed = DeviceDraws(0)
    resumed.set_state({"seed": SEED, "counter": 40})
    assert resumed.state() == {"seed": SEED, "counter": 40}
    sel, _ = batcher.draw(idx_l, idx_u, params=params, draws=resumed)
    assert torch.is_tensor(sel) and sel.is_cuda and np.array_equal(sel.cpu().numpy(), rows)
    given = np.zeros((3, M_BATCH), dtype=np.int64)
    sel, _ = batcher.draw(idx_l, idx_u, sel_l=given, params=params, draws=DeviceDraws(SEED, 40))
    assert np.array_equal(sel.cpu().numpy(), np.concatenate([given, rows[3:]]))
    sel, _ = batcher.draw(idx_l, idx_u, sel_l=given, sel_u=rows[3:], params=params, draws=resumed)
    assert isinstance(sel, np.ndarray) and resumed.counter == 47
    # on a side stream, with the DeviceDraws given to the constructor
    side = FixMatchBatcher(lab, unl, M_BATCH, stream=torch.cuda.Stream(), draws=DeviceDraws(SEED, 40))
    data, data_u = side.batch(idx_l, idx_u, params=params)
    side.join(data, data_u)
    torch.cuda.synchronize()
    _same_batch(data, want[0])
    _same_batch(data_u, want[1])


def test_supervised_batcher_draws_on_the_device(no_choice):
    from geot_amd.openpoints.dataset import DeviceDraws, SupervisedBatcher
    scans = _scan_set(BATCH_SIZES, 3)
    batcher = SupervisedBatcher(scans, M_BATCH)
    idx = [3, 1, 0, 2, 1]
    sizes = [BATCH_SIZES[i] for i in idx]
    torch.manual_seed(4)
    np.random.seed(4)
    params = [batcher.program.draw(M_BATCH) for _ in idx]
    np.random.seed(9)
    host = batcher.batch(idx, params=params, check=True)
    assert _state_equal(np.random.get_state(), _choice_state(sizes, M_BATCH, 9))
    rows, _ = sd.sample_draw_ref(sizes, M_BATCH, SEED, 2 ** 32 - 2)
    want = batcher.batch(idx, sel=rows, params=params, check=True)
    before = np.random.get_state()
    no_choice()
    draws = DeviceDraws(SEED, 2 ** 32 - 2)
    got = batcher.batch(idx, params=params, check=True, draws=draws)
    assert draws.counter == 2 ** 32 + 3 and _state_equal(np.random.get_state(), before)
    _same_batch(got, want)
    assert not torch.equal(got["y"], host["y"])
    _same_batch(batcher.batch(idx, params=params, draws=DeviceDraws(SEED, 2 ** 32 - 2)), want)
    sel, _ = batcher.draw(idx, params=params, draws=DeviceDraws(SEED, 2 ** 32 - 2))
    assert torch.is_tensor(sel) and np.array_equal(sel.cpu().numpy(), rows)
    side = SupervisedBatcher(scans, M_BATCH, stream=torch.cuda.Stream(), draws=DeviceDraws(SEED, 2 ** 32 - 2))
    data = side.batch(idx, params=params)
    side.join(data)
    torch.cuda.synchronize()
    _same_batch(data, want)


def test_val_batcher_draws_on_the_device(no_choice):
    from geot_amd.openpoints.dataset import DeviceDraws, ValBatcher
    scans = _scan_set(BATCH_SIZES, 4)
    batcher = ValBatcher(scans, M_BATCH)
    idx = [0, 1, 2, 3]
    np.random.seed(9)
    host = batcher.batch(idx, check=True)
    assert _state_equal(np.random.get_state(), _choice_state(BATCH_SIZES, M_BATCH, 9))
    rows, _ = sd.sample_draw_ref(BATCH_SIZES, M_BATCH, SEED, 0)
    want = batcher.batch(idx, sel=rows, check=True)
    before = np.random.get_state()
    no_choice()
    draws = DeviceDraws(SEED)
    got = batcher.batch(idx, check=True, draws=draws)
    assert draws.counter == 4 and _state_equal(np.random.get_state(), before)
    _same_batch(got, want)
    assert not torch.equal(got["y"], host["y"])
    _same_batch(batcher.batch(idx, draws=DeviceDraws(SEED)), want)
    side = ValBatcher(scans, M_BATCH, stream=torch.cuda.Stream(), draws=DeviceDraws(SEED))
    data = side.batch(idx)
    side.join(data)
    torch.cuda.synchronize()
    _same_batch(data, want)


def test_the_names_are_exported():
    import geot_amd.openpoints.dataset as ds
    assert callable(ds.sample_draw) and ds.DeviceDraws(5).take(3) == 0
    d = ds.DeviceDraws(2 ** 64 + 5, 2 ** 64 - 1)
    assert d.seed == 5 and d.take(2) == 2 ** 64 - 1 and d.counter == 1
