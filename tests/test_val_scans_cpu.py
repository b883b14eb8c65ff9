"""The host halves of validating whole scans from a device-resident scan set (no GPU): the validation loader's draws
(geot_amd/openpoints/dataset/val_batch.py draw_val_sel) against the restated dataset statements and the reference-made
fixture, geot_scan_predict's work table (geot_amd/validation.py scan_work_table), the refusals that need no device and the
binding of the new entry points."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "val_batches_ref.npz")


def _restated_draws(sizes, m):
    """tooth_dataset.py:134-135 per item, in item order."""
    out = []
    for n in sizes:
        points_norm = np.zeros((n, 3), np.float32)
        replace = False if len(points_norm) >= m else True
        out.append(np.random.choice(len(points_norm), m, replace=replace))
    return np.stack(out)


@pytest.mark.parametrize("sizes,m", [((1500, 500, 2000, 1201), 768), ((5, 1, 9), 8), ((8, 8), 8), ((3,), 1)])
def test_draws_equal_the_dataset_statements_and_draw_nothing_else(sizes, m):
    from geot_amd.openpoints.dataset import draw_val_sel
    np.random.seed(77)
    torch.manual_seed(77)
    want, want_next, want_torch = _restated_draws(sizes, m), np.random.random_sample(3), torch.rand(3)
    np.random.seed(77)
    torch.manual_seed(77)
    got, got_next, got_torch = draw_val_sel(sizes, m), np.random.random_sample(3), torch.rand(3)
    assert got.dtype == np.int64 and got.shape == (len(sizes), m)
    assert np.array_equal(got, want) and np.array_equal(got_next, want_next) and torch.equal(got_torch, want_torch)
    for row, n in zip(got, sizes):
        assert row.min() >= 0 and row.max() < n
        if n >= m:
            assert len(set(row.tolist())) == m             # replace=False: no vertex twice
        else:
            assert len(set(row.tolist())) < m              # replace=True exactly when N_i < m: a repeat is certain


def test_draws_equal_the_reference_fixture():
    from geot_amd.openpoints.dataset import draw_val_sel
    fx = np.load(FIXTURE, allow_pickle=False)
    assert int(fx["n_torch_rand"]) == 0
    np.random.seed(int(fx["seed"]))
    torch.manual_seed(int(fx["seed"]))
    for k in range(int(fx["batches"])):
        sizes = [len(fx["scan%d" % i]) for i in fx["b%d_ids" % k]]
        assert np.array_equal(draw_val_sel(sizes, int(fx["num_points"])), fx["b%d_sel" % k])
    assert np.array_equal(np.random.random_sample(4), fx["next_np"])
    assert np.array_equal(torch.rand(4).numpy(), fx["next_torch"])
    assert any(len(fx["scan%d" % i]) < int(fx["num_points"]) for i in range(4))


def _check_cover(table, sizes):
    """Every vertex of every slot in exactly one entry, by interval arithmetic (no per-vertex array)."""
    assert table.dtype == np.int32 and table.ndim == 2 and table.shape[1] == 4 and table.flags["C_CONTIGUOUS"]
    t = table.astype(np.int64)
    assert (t[:, 3] == 0).all() and (t[:, 2] >= 1).all() and (t[:, 1] >= 0).all()
    for slot, m in enumerate(sizes):
        rows = t[t[:, 0] == slot]
        rows = rows[np.argsort(rows[:, 1])]
        assert rows[0, 1] == 0
        assert np.array_equal(rows[1:, 1], rows[:-1, 1] + rows[:-1, 2])          # no gap, no overlap
        assert rows[-1, 1] + rows[-1, 2] == m
    assert set(t[:, 0].tolist()) == set(range(len(sizes)))


@pytest.mark.parametrize("sizes", [(1,), (255,), (256,), (257,), (1, 255, 256, 257), (257, 1, 100003, 63, 64, 65),
                                   (100003, 98765), ((1 << 31) - 1,), ((1 << 31) - 1, 1, (1 << 31) - 1)])
def test_work_table_covers_every_vertex_once(sizes):
    from geot_amd.validation import SCAN_CHUNK_MIN, SCAN_GROUPS, scan_work_table
    table = scan_work_table(sizes)
    _check_cover(table, sizes)
    assert len(table) <= SCAN_GROUPS + len(sizes)
    chunk = int(table[:, 2].max())
    assert chunk % 4 == 0 or len(table) == len(sizes)
    assert chunk <= max(SCAN_CHUNK_MIN, -(-sum(sizes) // SCAN_GROUPS) + 3)


def test_work_table_small_groups_and_refusals():
    from geot_amd.validation import scan_work_table
    for groups, min_chunk in ((1, 1), (3, 4), (7, 64), (100000, 1)):
        _check_cover(scan_work_table((1, 255, 256, 257), groups, min_chunk), (1, 255, 256, 257))
    assert scan_work_table(()).shape == (0, 4)
    for bad in ((0,), (5, -1), (1 << 31,)):
        with pytest.raises(RuntimeError, match="vertices per scan"):
            scan_work_table(bad)


def test_cpu_sets_and_tensors_are_refused():
    from geot_amd.openpoints.dataset import DeviceScanSet, ValBatcher
    from geot_amd.validation import predict_scans
    with pytest.raises(RuntimeError, match="CPU not supported"):
        DeviceScanSet([np.zeros((4, 3), np.float32)], [np.zeros(4, np.int32)], device="cpu")
    cpu_set = DeviceScanSet.__new__(DeviceScanSet)          # what a caller could assemble by hand
    cpu_set.device, cpu_set.sizes = torch.device("cpu"), [4]
    cpu_set.points, cpu_set.labels = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32)
    cpu_set.offsets, cpu_set.cls = torch.tensor([0, 4]), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ValBatcher(cpu_set, 8)
    with pytest.raises(RuntimeError, match="DeviceScanSet"):
        ValBatcher([np.zeros((4, 3), np.float32)], 8)
    batch = {"pos": torch.zeros(1, 8, 3), "center": torch.zeros(1, 3), "scale": torch.ones(1), "scan_ids": torch.zeros(1, dtype=torch.int64),
             "scans": cpu_set, "sizes": [4]}
    with pytest.raises(RuntimeError, match="CPU not supported"):
        predict_scans(torch.zeros(1, 17, 8), batch)


def test_the_new_entry_points_are_declared_bound_and_planned():
    from geot_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    assert int(re.search(r"GEOT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 15
    for name in ("geot_scan_predict", "geot_scan_predict_ws_bytes"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.exported_symbols()
    proto = re.search(r"int geot_scan_predict\((.*?)\);", hdr, flags=re.S).group(1)
    assert len(proto.split(",")) == len(_lib.PROTOTYPES["geot_scan_predict"])
    lib = _lib.load()
    assert lib.geot_scan_predict_ws_bytes(2, 16000) == lib.geot_knn_grid_ws_bytes(2, 16000) and lib.geot_scan_predict_ws_bytes(1, 1) % 16 == 0
    for b, n in ((0, 8), (-1, 8), (65536, 8), (1, 0)):
        assert lib.geot_scan_predict_ws_bytes(b, n) == -1
