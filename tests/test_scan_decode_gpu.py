"""Whole scans decoded at full resolution from one backbone pass, kernel level (csrc/scan_decode.hip), through the C ABI:
geot_scan_decode_front's q against the numpy float32 restatement bit for bit, its idx and weight against geot_three_nn_ws +
geot_fp_weights on the same q bit for bit, its rows within the operation-count bound of the fp64 restatement
(tests/_scan_decode_ref.py); geot_scan_decode_finish against the arg-max rule and geot_seg_confusion; both bit-reproducible.
The shapes are the smallest at which the kernels change path: records of 1 / 63 / 64 / 65 / 1000 vertices (one lane per vertex,
256 per round: a partial round, exact rounds, four rounds), m below, at and over one LDS tile's first steps, c_out through both
store forms.  (Model level: tests/test_scan_decode_model_gpu.py; fit(): tests/test_fit_val_whole_gpu.py.)"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scan_decode_ref as dref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = [1, 63, 64, 65, 1000]
SLOTS = [4, 0, 2, 4, 1, 3]              # permuted, scan 4 in two slots
NAN_VERTEX = 517                        # of scan 4
SENTINEL = -12345.0
_cache = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _kernel_set():
    """Five scans in scan coordinates with one NaN vertex; made once, never changed."""
    if "set" not in _cache:
        from geot_amd.openpoints.dataset import DeviceScanSet
        rng = np.random.default_rng(11)
        pts = [(rng.normal(size=(m, 3)) * 8.0 + np.array([14.0, -37.0, 61.0])).astype(np.float32) for m in SIZES]
        pts[4][NAN_VERTEX, 1] = np.nan
        labels = [rng.integers(0, 40, size=m).astype(np.int32) - 3 for m in SIZES]         # some outside [0, c)
        _cache["set"] = (DeviceScanSet(pts, labels, device=DEV), pts, labels)
    return _cache["set"]


def _front_inputs(m, c_out, seed):
    """Seeded inputs of one front call over SLOTS, host arrays: the slots' affines, centres with duplicates, the stage."""
    rng = np.random.default_rng(seed)
    b = len(SLOTS)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    center = (np.array([14.0, -37.0, 61.0]) + rng.normal(size=(b, 3))).astype(np.float32)
    scale = (rng.random(b) * 4 + 20).astype(np.float32)
    vcenter, vscale = (f(b, 3) * 0.05).astype(np.float32), (rng.random(b) * 0.5 + 0.8).astype(np.float32)
    known = (f(b, m, 3) * 0.4).astype(np.float32)
    known[:, m - 1] = known[:, 0]                           # duplicate centres: the index tie rule
    if m >= 5:
        known[:, 3] = known[:, 0]
    return dict(center=center, scale=scale, view_center=vcenter, view_scale=vscale, known=known, a=f(b, m, c_out),
                skip_const=f(b, c_out), w_xyz=f(c_out, 3), ch_scale=(f(c_out) * 0.5 + 1).astype(np.float32), ch_shift=f(c_out))


def _front(dset, host, relu, table, chunks, skip_record=None, debug=True):
    """geot_scan_decode_front per chunk through the C ABI -> per chunk (z, q, idx, weight) on the host; every buffer starts
    as SENTINEL (idx: -7).  skip_record: that record's slot is made unusable on the device copy."""
    from geot_amd.ext._common import call, ptr
    dv = {k: _dev(v) for k, v in host.items()}
    b, m, c_out = host["known"].shape[0], host["known"].shape[1], host["a"].shape[2]
    table = table.copy()
    if skip_record is not None:
        table[skip_record, 0] = -1
    work, ids = _dev(table), _dev(np.asarray(SLOTS, np.int64))
    out = []
    for first, count, rows in chunks:
        z = torch.full((rows, c_out), SENTINEL, dtype=torch.float32, device=DEV)
        q, w = (torch.full((rows, 3), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(2))
        idx = torch.full((rows, 3), -7, dtype=torch.int32, device=DEV)
        call("geot_scan_decode_front", DEV, b, m, c_out, int(relu), len(dset), int(dset.points.shape[0]), ptr(dset.points),
             ptr(dset.offsets), ptr(ids), ptr(dv["center"]), ptr(dv["scale"]), ptr(dv["view_center"]), ptr(dv["view_scale"]),
             ptr(dv["known"]), ptr(dv["a"]), ptr(dv["skip_const"]), ptr(dv["w_xyz"]), ptr(dv["ch_scale"]), ptr(dv["ch_shift"]), count,
             ptr(work) + 16 * first, rows, ptr(z), *((ptr(q), ptr(idx), ptr(w)) if debug else (None, None, None)))
        out.append(tuple(t.cpu().numpy() for t in (z, q, idx, w)))
    torch.cuda.synchronize()
    return out


def _chain(q, known):
    """geot_three_nn_ws + geot_fp_weights on the same q (one slot's rows): (idx, weight) as the existing kernels give them."""
    from geot_amd.ext._common import call, knn_workspace, ptr
    qd, kd = _dev(q[None]), _dev(known[None])
    n, m = q.shape[0], known.shape[0]
    d2 = torch.empty((1, n, 3), dtype=torch.float32, device=DEV)
    idx = torch.empty((1, n, 3), dtype=torch.int32, device=DEV)
    wp, wb, _keep = knn_workspace(DEV, 1, n, m, 3)
    call("geot_three_nn_ws", DEV, 1, n, m, ptr(qd), ptr(kd), ptr(d2), ptr(idx), wp, wb)
    w = torch.empty_like(d2)
    call("geot_fp_weights", DEV, 1, n, ptr(d2), ptr(w))
    torch.cuda.synchronize()
    return idx[0].cpu().numpy(), w[0].cpu().numpy()


def _same_bits(a, b):
    """Equal bit for bit; a NaN equals a NaN (IEEE leaves its sign and payload open: 0 / 0 is -NaN on x86)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return np.array_equal(a, b)
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


CHUNK = 700         # 1000 + 1 + 64 + 1000 + 63 + 65 rows: boundaries inside both copies of the 1000-vertex scan


@pytest.mark.parametrize("c_out", [1, 3, 4, 5, 260, 1536])
@pytest.mark.parametrize("m", [3, 5, 64, 65, 300])
def test_front_against_the_chain_and_the_fp64_rows(m, c_out):
    from geot_amd.validation import decode_work_table
    dset, pts, _ = _kernel_set()
    sizes = [SIZES[i] for i in SLOTS]
    relu = (m + c_out) % 2 == 0
    host = _front_inputs(m, c_out, 1000 * m + c_out)
    table, chunks = decode_work_table(sizes, CHUNK)
    assert len(chunks) == 4 and any(r[1] > 0 and r[0] in (0, 3) for r in table)           # a record starting inside a scan
    skip = int(np.flatnonzero((table[:, 0] == 3) & (table[:, 2] == 256))[0])               # a full record of the second copy
    got = _front(dset, host, relu, table, chunks, skip_record=skip)
    again = _front(dset, host, relu, table, chunks, skip_record=skip)
    for (z, q, idx, w), (z2, q2, idx2, w2) in zip(got, again):                             # the same call, the same bits
        assert _same_bits(z, z2) and _same_bits(q, q2) and _same_bits(idx, idx2) and _same_bits(w, w2)
    worst = 0.0
    for k, (first, count, rows) in enumerate(chunks):
        z, q, idx, w = got[k]
        touched = np.zeros(rows, bool)
        for r, (slot, v0, cnt, r0) in enumerate(table[first:first + count]):
            rr = slice(r0, r0 + cnt)
            if first + r == skip:                           # a skipped record: its rows are untouched
                assert (z[rr] == SENTINEL).all() and (q[rr] == SENTINEL).all() and (idx[rr] == -7).all() and (w[rr] == SENTINEL).all()
                continue
            touched[rr] = True
            p = pts[SLOTS[slot]][v0:v0 + cnt]
            want_q = dref.query_positions(p, host["center"][slot], host["scale"][slot], host["view_center"][slot], host["view_scale"][slot])
            assert _same_bits(q[rr], want_q), (m, c_out, slot, v0)
            want_idx, want_w = _chain(q[rr], host["known"][slot])
            assert _same_bits(idx[rr], want_idx) and _same_bits(w[rr], want_w), (m, c_out, slot, v0)
            ref_d2, ref_idx = dref.three_nn(q[rr], host["known"][slot])
            assert np.array_equal(ref_idx, idx[rr]) and _same_bits(dref.fp_weights(ref_d2), w[rr])
            nan = np.isnan(q[rr]).any(1)
            if SLOTS[slot] == 4 and v0 <= NAN_VERTEX < v0 + cnt:
                assert nan.sum() == 1 and nan[NAN_VERTEX - v0] and (idx[rr][nan] == 0).all() and np.isnan(z[rr][nan]).all()
            else:
                assert not nan.any()
            want, bound = dref.front_rows(q[rr][~nan], idx[rr][~nan], w[rr][~nan], host["a"][slot], host["skip_const"][slot],
                                          host["w_xyz"], host["ch_scale"], host["ch_shift"], relu)
            err = np.abs(z[rr][~nan] - want)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (m, c_out, slot, v0, float((err / bound).max()))
            if relu:
                assert (z[rr][~nan] >= 0).all()
        skipped = table[skip]
        assert touched.sum() == rows - (skipped[2] if first <= skip < first + count else 0)
    print("front m=%d c_out=%d relu=%d: worst error / bound = %.3f" % (m, c_out, relu, worst))
    assert 0 < worst <= 1
    # the duplicate centres: wherever centre 0 comes first, its twin of the next index follows
    z, q, idx, w = got[0]
    hit = idx[(idx[:, 0] == 0) & (q[:, 0] != SENTINEL) & ~np.isnan(q).any(1)]
    assert (hit[:, 1] == (3 if m >= 5 else m - 1)).all()


def test_front_without_the_optional_outputs_writes_the_same_rows():
    from geot_amd.validation import decode_work_table
    dset, _, _ = _kernel_set()
    host = _front_inputs(65, 260, 9)
    table, chunks = decode_work_table([SIZES[i] for i in SLOTS], CHUNK)
    for relu in (False, True):
        a, b = _front(dset, host, relu, table, chunks), _front(dset, host, relu, table, chunks, debug=False)
        assert all(_same_bits(x[0], y[0]) and (y[1] == SENTINEL).all() for x, y in zip(a, b))
    off, on = _front(dset, host, False, table, chunks), _front(dset, host, True, table, chunks)
    for (z0, *_), (z1, *_) in zip(off, on):
        ok = ~np.isnan(z0)
        assert (z0[ok] < 0).any() and _same_bits(np.maximum(z0[ok], 0), z1[ok]) and np.isnan(z1[~ok]).all()


@pytest.mark.parametrize("c", [1, 5, 17, 32])
def test_finish_is_the_argmax_rule_and_seg_confusion(c):
    from geot_amd.ext._common import call, ptr
    from geot_amd.validation import decode_work_table
    dset, _, labels = _kernel_set()
    sizes = [SIZES[i] for i in SLOTS]
    table, chunks = decode_work_table(sizes, CHUNK)
    skip = 2
    dev_table = table.copy()
    dev_table[skip, 3] = CHUNK                              # rows out of range: skipped
    work, ids = _dev(dev_table), _dev(np.asarray(SLOTS, np.int64))
    starts = np.concatenate([[0], np.cumsum(sizes)])
    out_offs = _dev(starts[:-1].astype(np.int64))
    rng = np.random.default_rng(40 + c)
    runs = []
    for _ in range(2):
        pred = torch.full((sum(sizes),), -1, dtype=torch.int64, device=DEV)
        counts = torch.zeros((len(SLOTS), c * (c + 1) + 1), dtype=torch.int64, device=DEV)
        rng = np.random.default_rng(40 + c)
        want = np.full(sum(sizes), -1, np.int64)
        for first, count, rows in chunks:
            logits = np.round(rng.normal(size=(c, rows)) * 2).astype(np.float32)          # rounded: many exact ties
            logits[rng.integers(0, c, size=rows // 50), rng.integers(0, rows, size=rows // 50)] = np.nan
            lg = _dev(logits)
            call("geot_scan_decode_finish", DEV, len(SLOTS), c, len(dset), int(dset.points.shape[0]), ptr(dset.labels),
                 ptr(dset.offsets), ptr(ids), count, ptr(work) + 16 * first, rows, ptr(lg), ptr(out_offs), ptr(pred), ptr(counts))
            cls = dref.argmax_rule(logits.T)
            for r, (slot, v0, cnt, r0) in enumerate(table[first:first + count]):
                if first + r != skip:
                    want[starts[slot] + v0:starts[slot] + v0 + cnt] = cls[r0:r0 + cnt]
        torch.cuda.synchronize()
        runs.append((pred.cpu().numpy(), counts.cpu().numpy()))
    pred, counts = runs[0]
    assert np.array_equal(pred, want) and (pred == -1).sum() == table[skip, 2]
    assert np.array_equal(runs[1][0], pred) and np.array_equal(runs[1][1], counts)
    # geot_seg_confusion on the same labels (the skipped record's vertices left out of both)
    keep = pred >= 0
    sub_sizes = [int(keep[starts[s]:starts[s + 1]].sum()) for s in range(len(SLOTS))]
    lab = np.concatenate([labels[SLOTS[s]].astype(np.int64)[keep[starts[s]:starts[s + 1]]] for s in range(len(SLOTS))])
    offs = _dev(np.concatenate([[0], np.cumsum(sub_sizes)]).astype(np.int64))
    conf = torch.zeros_like(_dev(counts))
    pred_dev, lab_dev = _dev(pred[keep]), _dev(lab)
    call("geot_seg_confusion", DEV, len(SLOTS), c, ptr(offs), ptr(pred_dev), ptr(lab_dev), ptr(conf))
    torch.cuda.synchronize()
    assert np.array_equal(conf.cpu().numpy(), counts) and counts.sum() == keep.sum()
    at = 0
    for s, n in enumerate(sub_sizes):
        assert np.array_equal(counts[s], dref.confusion_counts(pred[keep][at:at + n], lab[at:at + n], c))
        at += n
