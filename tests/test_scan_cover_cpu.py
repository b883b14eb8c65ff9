"""Covering passes without a GPU: the numpy restatement of geot_sample_draw_cover (tests/_scan_cover_ref.py) has the properties
the contract promises -- the passes partition the scan, one owner per vertex, pass 0 is geot_sample_draw's row, the position is
64-bit -- the build declares and exports both entry points at ABI >= 30, and ScanBatcher.cover() refuses host draws before any
device call and takes len(idx) draw ids per round."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sample_draw_ref as sref  # noqa: E402
import _scan_cover_ref as cref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, DRAW = 0x1234_5678_9ABC_DEF0, (1 << 40) + 3
SIZES = (1, 2, 5, 511, 512, 1000, 1024, 1025, 40001)
MS = (1, 7, 512, 1024)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", SIZES)
def test_the_passes_partition_the_scan(n, m):
    passes = cref.cover_passes(n, m)
    assert passes == -(-n // m) and (passes - 1) * m < n <= passes * m
    rows = cref.cover_rows(n, m, SEED, DRAW, range(passes + 1))
    assert rows.shape == (passes + 1, m) and rows.min() >= 0 and rows.max() < n
    own = np.stack([cref.owners(n, m, p) for p in range(passes + 1)])
    assert own[:passes].sum() == n and not own[passes].any()            # P passes own n vertices; the pass after them none
    assert all(own[p].all() for p in range(passes - 1))                 # only the last pass has fill
    seen = np.bincount(rows[own], minlength=n)
    assert seen.shape == (n,) and (seen == 1).all()                     # exactly one owner per vertex: a partition of [0, n)
    # the fill re-uses the start of the permutation: position q and position q - n agree
    flat = rows[:passes].reshape(-1)
    assert np.array_equal(flat[n:], np.resize(flat[:n], flat.size)[n:])
    if n >= m:
        assert np.array_equal(rows[0], sref.draw_rows(n, m, SEED, [DRAW])[0])       # pass 0 is geot_sample_draw's row
    if n >= 512:
        assert not np.array_equal(rows[0], np.arange(m) % n)            # (a permutation that moves something)


def test_the_position_is_64_bit():
    n, m, p = 5, 7, (1 << 31) - 1
    table = cref.sigma(n, SEED, DRAW)
    assert sorted(table.tolist()) == list(range(n))
    want = [int(table[(p * m + j) % n]) for j in range(m)]
    assert cref.cover_rows(n, m, SEED, DRAW, [p])[0].tolist() == want
    wrapped = [int(table[((p * m + j) & 0xFFFFFFFF) % n]) for j in range(m)]     # what a 32-bit position would give
    assert wrapped != want
    assert not cref.owners(n, m, p).any()
    sel, bad = cref.sample_draw_cover_ref([n, 0, 2], m, SEED, DRAW, p)
    assert bad.tolist() == [0, 2, 0] and sel[0].tolist() == want and not sel[1].any()
    assert sel[2].tolist() == cref.cover_rows(2, m, SEED, DRAW + 2, [p])[0].tolist()


def test_another_draw_id_is_another_permutation():
    a, b = cref.sigma(1000, SEED, DRAW), cref.sigma(1000, SEED, DRAW + 1)
    assert sorted(a.tolist()) == sorted(b.tolist()) == list(range(1000)) and (a != b).sum() > 900


# ------------------------------------------------------------------------------------------------ the build
def test_header_library_and_binding_carry_both_entry_points():
    from geot_amd import _header, _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    assert int(re.search(r"GEOT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 30
    entries = {e.name: e for e in _header.parse()[0]}
    lib = _lib.load()
    assert lib.geot_abi_version() == _lib.ABI_VERSION
    for name, params in (("geot_sample_draw_cover", 12), ("geot_scan_cover", 19)):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in entries and entries[name].streamed and len(entries[name].params) == params
        assert name in _lib.PROTOTYPES and name in _lib.exported_symbols() and callable(getattr(lib, name))
    # geot_sample_draw's arguments plus `int pass` after draw_base
    draw = [kind for kind, _ in entries["geot_sample_draw"].params]
    cover = [kind for kind, _ in entries["geot_sample_draw_cover"].params]
    assert cover == draw[:8] + ["int"] + draw[8:] and entries["geot_sample_draw_cover"].params[8][1] == "int pass"
    # the refusals that need no device: checked before any launch
    import ctypes
    one = ctypes.c_void_p(16)
    assert lib.geot_sample_draw_cover(1, 8, 1, 8, one, None, 1, 0, -1, one, one, None) == 1
    assert lib.geot_scan_cover(1, 17, 8, 1, 8, None, one, one, one, one, -1, 1, one, one, one, 0, None, None, None) == 1
    assert lib.geot_scan_cover(1, 17, 8, 1, 8, None, one, one, None, one, 0, 1, one, one, one, 0, None, None, None) == 1
    assert lib.geot_scan_cover(0, 17, 8, 1, 8, None, one, one, one, one, 0, 1, one, one, one, 0, None, None, None) == 0   # b = 0


def test_cover_passes():
    from geot_amd.openpoints.dataset.sample_draw import cover_passes
    assert cover_passes([100000], 16000) == 7 and cover_passes([300, 700, 1300], 512) == 3
    assert cover_passes([5], 16) == 1 and cover_passes([512], 512) == 1 and cover_passes([513, 2], 512) == 2
    assert abs(0.84 ** 10 - 0.175) < 5e-4           # the share of vertices ten independent passes of 16 % never show
    with pytest.raises(RuntimeError):
        cover_passes([], 4)
    with pytest.raises(RuntimeError):
        cover_passes([4], 0)


# ------------------------------------------------------------------------------------------------ cover() on the host
class _Set:
    sizes = [300, 700, 1300]

    def __len__(self):
        return len(self.sizes)


def _batcher(monkeypatch, draws=None, device_calls=None):
    """A ValBatcher that never saw a device: its draw and its batch recorded in place of the launches."""
    from geot_amd.openpoints.dataset import val_batch
    from geot_amd.openpoints.dataset.fixmatch_batch import TOOTH_VIEW_KWARGS
    b = object.__new__(val_batch.ValBatcher)
    b.scans, b.m, b.c, b.stream, b.draws, b.kwargs, b.device = _Set(), 512, 17, None, draws, TOOTH_VIEW_KWARGS, torch.device("cpu")
    calls = [] if device_calls is None else device_calls

    def draw(scans, ids, m, seed, base, p):
        calls.append(("draw", ids.tolist(), m, seed, base, p))
        return torch.zeros((len(ids), m), dtype=torch.int64), None

    def batch(self, ids, shape, sel, params, ids_dev, check):
        calls.append(("batch", list(ids), shape, len(params), check))
        return {"scan_ids": ids_dev}
    monkeypatch.setattr(val_batch, "sample_draw_cover", draw)
    monkeypatch.setattr(val_batch.ValBatcher, "_batch", batch)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    return b, calls


def test_cover_without_device_draws_raises_before_any_device_call(monkeypatch):
    b, calls = _batcher(monkeypatch)
    with pytest.raises(ValueError, match="DeviceDraws"):
        b.cover([0, 1])
    with pytest.raises(ValueError, match="DeviceDraws"):
        b.cover([0, 1], draws=np.random.default_rng(0))
    from geot_amd.openpoints.dataset import DeviceDraws
    with pytest.raises(ValueError, match="rounds"):
        b.cover([0, 1], rounds=0, draws=DeviceDraws(1))
    with pytest.raises(RuntimeError, match="idx"):
        b.cover([3], draws=DeviceDraws(1))
    assert calls == []


def test_cover_takes_one_id_per_slot_and_round(monkeypatch):
    from geot_amd.openpoints.dataset import DeviceDraws
    draws = DeviceDraws(5, counter=100)
    b, calls = _batcher(monkeypatch, draws=draws)
    gen = b.cover([2, 0, 1], rounds=3)                  # the constructor's draws
    assert draws.counter == 100 and calls == []         # nothing is taken or queued before the first batch is asked for
    first = next(gen)
    assert draws.counter == 103 and first["cover"] == (0, 3, 0) and tuple(first["sel"].shape) == (3, 512)
    rest = list(gen)
    assert draws.counter == 100 + 3 * 3                 # len(idx) * rounds
    assert [x["cover"] for x in [first] + rest] == [(p, 3, r) for r in range(3) for p in range(3)]
    drawn = [c for c in calls if c[0] == "draw"]
    assert drawn == [("draw", [2, 0, 1], 512, 5, 100 + 3 * r, p) for r in range(3) for p in range(3)]    # a slot keeps its id
    assert [c for c in calls if c[0] == "batch"] == [("batch", [2, 0, 1], (3,), 3, False)] * 9
    # draws= of the call wins; one scan of 300 < m vertices is one pass
    other = DeviceDraws(9, counter=7)
    assert [x["cover"] for x in b.cover([0], rounds=2, draws=other)] == [(0, 1, 0), (0, 1, 1)]
    assert other.counter == 9 and draws.counter == 109
