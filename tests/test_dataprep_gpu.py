"""GPU suite of the data-preparation kernels (geot_amd/csrc/dataprep.hip) over the case tables of tests/_dataprep_ref.py:
geot_grid_subsampling, geot_pc_norm_stats, geot_cloud_sample and geot_cloud_sample_batch at every launch branch, through
the package's wrappers and through the C ABI itself.  tests/test_dataprep_cases_cpu.py holds the tables to the branches
they name, without a GPU.

What is asserted
  grid subsampling   every output bit for bit against oracle.np_data, nothing excluded; against the reference's compiled
                     rows (tests/golden/grid_subsampling_edges_ref.npz) where a cell index is -1 and where keys are 40
                     bits wide.  NaN and infinite coordinates are outside the contract: no case has them.
  pc_norm / sample   the centroid within ulp32(mean64) / 2 + n 2^-53 mean|x| of the fp64 mean, positions within B_POS =
                     1e-5 of the fp64 pipeline and bit-equal to numpy's fp32 statements fed the kernel's centroid, labels
                     and class weights bit-equal to numpy's.
  batch              every slot bit-identical to the single-scan calls on that scan alone; unusable slots flagged 2 and
                     zero-filled, class weights included.

What the first runs on an MI355X showed
  The voxel key.  With the key kernel's conversion as it was, (u64)floorf(x), an index of -1 became 2^32 - 1 (the device's
  float -> unsigned conversion saturates per 32-bit half) where the reference's x86-64 build and np_data wrap to 2^64 - 1:
    neg:0:0         66 rows on both sides; the minimum point's row (1.9499999, -0.975, 2.325) is row 41 of np_data's and came
                    out last: 25 of 66 rows displaced
    neg:1:1         92 rows on both sides; the row (0.3325, -3.2110002, 2.2325) is row 39 and came out last: 53 of 92 displaced
                    (the fixture test failed with it: its tie mask is laid out in np_data's order)
    neg:0:3:merge   99 rows where np_data and the compiled reference have 98: the minimum point was not merged into cell
                    (NX - 1, iy - 1, iz)
    neg:2:2         passed: 2^32 - 1 and 2^64 - 1 in the z term both sort the point last, the rows are the same
  The kernel now converts through a signed 64-bit integer (gs_index) and all four agree.
  m == 0 left class_weights unwritten, and a flag-2 slot of geot_cloud_sample_batch had NaN class weights (0 / 0) beside
  its zero-filled outputs; both are fixed in dataprep.hip and pinned here (none-sampled; the unusable-slots test).
  One case of the issue is built otherwise than one might read it: a voxel holding x = (1e8, 1, -1e8, 1) exists only because
  the cell is 1e17 wide, so that 1e8 vanishes in the fp32 distance to the origin -- 0 is otherwise always a cell boundary.

Worst measured share of each derived bound (printed by the scan-case test; run with -s)
  centroid    1.000 of ulp32(mean64) / 2 + n 2^-53 mean|x|  (two-points, n255: the mean of two floats lies half-way between
              two neighbours; the next cases 0.985, 0.93)
  scale       0.123 of 1e-5 relative      (shifted; 0.013 elsewhere)
  positions   0.305 of B_POS = 1e-5       (shifted: the fp32 centroid of a cloud at 1e4 is half an ulp of 1e4 away from the
              exact one; 0.007 elsewhere)

Planted faults (scratch builds of dataprep.hip, value-only, never committed) and the tests that failed with each
  the key's iy term cut to 32 bits                     bit_exact[flat], [neg:1:1]; compiled_reference[neg:1:1]
  gs_index reverted to (u64)floorf                     bit_exact[neg:0:0], [neg:1:1], [neg:0:3:merge]; compiled_reference[neg:1:1]
  gs_reduce_kernel summing from e - 1 down to s        21 tests: bit_exact[order], [n:255..] .. [big], every fixture case, the ABI test
  the vote's run > best_run as >=                      bit_exact[labels], [two:one-voxel] and 7 more; the ABI test
  pn_sum_kernel's stride one block short               scan_case[n65535 .. n262145, shifted]; 6 batch cases (the batch kept its own)
  pnb_sum_kernel's stride one block short              6 batch cases
  pn_weights_kernel without its stride                 scan_case[n256, n257, n65535, n65536, n65537]; 4 batch cases; unusable slots
  pnb_centroid_kernel dividing by the next slot's n    all 7 batch cases; unusable slots
  gs_bbox_kernel without its second trip               bit_exact[big]
  pn_max_kernel without its second trip                scan_case[n262145]
  pnb_max_kernel without its second trip               6 batch cases
  pn_sample_kernel without its second trip             scan_case[n65537], [n262145]
  the label key's voxel id cut to 8 bits               bit_exact[wide:1], [wide:2], [n:4095..], [n:4096..]; compiled_reference[wide:1]; the ABI test
  m == 0 returning before pn_weights_kernel            scan_case[none-sampled]
  pnb_weights_kernel without its flag-2 zero fill      unusable slots
  (The first drafts of three cases let a fault through and were sharpened: the 50-bit-key cloud did not notice the cut iy
  term -- its rows are ordered by iz alone -- and became [flat]; [big] and the plain scan clouds now end in their extreme
  point, the one a grid-stride loop's last trip reads.)

Left unverified: s = 65535 slots (400 MB of workspace; the refusal at 65536 is in tests/test_views_cpu.py); NaN and infinite
coordinates (outside the contract); a scan of more than 2^31 - 1 vertices.
"""
import numpy as np
import pytest
import torch

import _dataprep_ref as R
from oracle import np_data

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F_SENTINEL, I_SENTINEL, MARGIN = -12345.0, -77, 64
WORST = {}            # the worst measured share of each derived bound, printed by every test that adds to it


def _share(key, value, bound):
    share = float(np.max(np.asarray(value, dtype=np.float64) / np.asarray(bound, dtype=np.float64))) if np.size(value) else 0.0
    WORST[key] = max(WORST.get(key, 0.0), share)
    return share


def _lib():
    from geot_amd import _lib
    return _lib.load()


def _up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


class Guarded:
    """An output buffer with sentinel margins on both sides and a sentinel (or garbage) fill."""

    def __init__(self, shape, dtype, fill=None):
        self.fill = fill if fill is not None else (F_SENTINEL if dtype.is_floating_point else I_SENTINEL)
        count = int(np.prod(shape))
        self.whole = torch.full((count + 2 * MARGIN,), self.fill, dtype=dtype, device=DEV)
        self.inner = self.whole[MARGIN:MARGIN + count].view(*shape)

    def ptr(self):
        return self.whole[MARGIN:].data_ptr()

    def intact(self):
        return bool((self.whole[:MARGIN] == self.fill).all()) and bool((self.whole[self.whole.numel() - MARGIN:] == self.fill).all())

    def numpy(self):
        return self.inner.cpu().numpy()


def _garbage(nbytes):
    return torch.full((max(int(nbytes), 1),), 0xFF, dtype=torch.uint8, device=DEV)


# ---- grid subsampling ---------------------------------------------------------------------------------------------------------
def _grid(p, f, lab, dl):
    from geot_amd.openpoints.dataset import grid_subsampling
    res = grid_subsampling(_up(p), _up(f), _up(lab), sampleDl=dl)
    out = [r.cpu().numpy() for r in ((res,) if isinstance(res, torch.Tensor) else res)]
    return {"points": out.pop(0), "features": out.pop(0) if f is not None else None, "labels": out.pop(0) if lab is not None else None}


def _assert_grid(got, want, what):
    rows = "%s: %d rows, np_data has %d" % (what, len(got["points"]), len(want["points"]))
    for part in ("points", "features", "labels"):
        if want[part] is None:
            assert got[part] is None
            continue
        assert R.same_bits(got[part], want[part]), "%s; %s: %s" % (rows, part, R.first_difference(got[part], want[part]))


@pytest.mark.parametrize("name", R.GS_NAMES)
def test_grid_subsampling_bit_exact_at_every_branch(name):
    c = R.gs_case(name)
    _assert_grid(_grid(c["p"], c["f"], c["lab"], c["dl"]), c["want"], name)


@pytest.mark.parametrize("name", R.FIXTURE_CASES)
def test_grid_subsampling_matches_the_compiled_reference_at_the_edges(name):
    """Against the rows the reference's own compiled code returned (in its hash map's order): an index of -1 on each axis,
    40-bit keys.  Labels are compared where the vote is not tied."""
    z, key = np.load(R.EDGES), R.fixture_key(name)
    got = _grid(z[key + "_points"], z[key + "_features"], z[key + "_labels"], float(z[key + "_dl"]))
    ref_p, ref_f, ref_l = z[key + "_ref_points"], z[key + "_ref_features"], z[key + "_ref_labels"]
    assert got["points"].shape == ref_p.shape, "%s: %d rows, the reference has %d" % (name, len(got["points"]), len(ref_p))
    a, b = np_data.row_order(got["points"]), np_data.row_order(ref_p)
    assert R.same_bits(got["points"][a], ref_p[b]), R.first_difference(got["points"][a], ref_p[b])
    assert R.same_bits(got["features"][a], ref_f[b]), R.first_difference(got["features"][a], ref_f[b])
    tied = R.gs_case(name)["want"]["tied"]
    assert tied.any(axis=1).mean() <= R.TIED_SHARE
    free = ~tied[a]
    assert np.array_equal(got["labels"][a][free], ref_l[b][free])


def _grid_abi(c, stream=None):
    """geot_grid_subsampling itself: outputs pre-filled with a sentinel between sentinel margins, the workspace with 0xFF."""
    lib = _lib()
    p, f, lab = _up(c["p"]), _up(c["f"]), _up(c["lab"])
    n, fdim, ldim = len(c["p"]), c["f"].shape[1], c["lab"].shape[1]
    nbytes = int(lib.geot_grid_subsampling_ws_bytes(n))
    assert nbytes > 0
    ws = _garbage(nbytes)
    out_p, out_f = Guarded((n, 3), torch.float32), Guarded((n, fdim), torch.float32)
    out_l, count = Guarded((n, ldim), torch.int32), Guarded((1,), torch.int32)
    torch.cuda.synchronize()
    err = lib.geot_grid_subsampling(n, fdim, ldim, c["dl"], _ptr(p), _ptr(f), _ptr(lab), out_p.ptr(), out_f.ptr(), out_l.ptr(),
                                    count.ptr(), ws.data_ptr(), nbytes, _stream() if stream is None else stream.cuda_stream)
    assert err == 0
    (stream.synchronize if stream is not None else torch.cuda.synchronize)()
    assert all(g.intact() for g in (out_p, out_f, out_l, count))
    return {"points": out_p.numpy(), "features": out_f.numpy(), "labels": out_l.numpy(), "count": int(count.numpy()[0])}


def test_grid_subsampling_abi_keeps_the_rows_past_the_count_and_does_not_depend_on_the_workspace():
    c = R.gs_case("n:4095:5:1:0.05")
    want = c["want"]
    m = len(want["points"])
    first, second = _grid_abi(c), _grid_abi(c)
    other = _grid_abi(c, stream=torch.cuda.Stream(DEV))                  # a stream that is not the default one
    for run in (first, second, other):
        assert run["count"] == m and 0 < m < len(c["p"])
        _assert_grid({k: run[k][:m] for k in ("points", "features", "labels")}, want, "abi")
        assert (run["points"][m:] == F_SENTINEL).all() and (run["features"][m:] == F_SENTINEL).all()
        assert (run["labels"][m:] == I_SENTINEL).all()
    for k in ("points", "features", "labels"):
        assert R.same_bits(first[k], second[k]) and R.same_bits(first[k], other[k])


# ---- pc_norm, sample, class weights: one scan -----------------------------------------------------------------------------------
def _sample_abi(pc, labels, sel, classes, m):
    """geot_pc_norm_stats + geot_cloud_sample themselves on device tensors: garbage in both workspaces, guarded outputs.
    sel None: the identity form (selected == NULL).  -> dict of numpy arrays and the out-of-range flag."""
    lib = _lib()
    n = pc.shape[0]
    stats = Guarded((4,), torch.float32)
    ws = _garbage(lib.geot_pc_norm_ws_bytes())
    assert lib.geot_pc_norm_stats(n, pc.data_ptr(), stats.ptr(), ws.data_ptr(), ws.numel(), _stream()) == 0
    pos, y = Guarded((m, 3), torch.float32), Guarded((m,), torch.int64)
    w, hist = Guarded((classes,), torch.float32), Guarded((classes + 1,), torch.int32, fill=0x7f7f7f7f)
    assert lib.geot_cloud_sample(n, m, classes, pc.data_ptr(), labels.data_ptr(), _ptr(sel), stats.ptr(), pos.ptr(), y.ptr(),
                                 w.ptr(), hist.ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert all(g.intact() for g in (stats, pos, y, w, hist))
    st = stats.numpy()
    return {"pos": pos.numpy(), "y": y.numpy(), "class_weights": w.numpy(), "center": st[:3].copy(), "scale": st[3],
            "flag": int(hist.numpy()[classes])}


@pytest.mark.parametrize("name", R.PN_NAMES)
def test_scan_case_against_numpy_at_every_branch(name):
    from geot_amd.openpoints.dataset import pc_norm, prepare_sample
    c = R.pn_case(name)
    n, m, classes, pc, idx = c["n"], c["m"], c["classes"], c["pc"], c["idx"]
    pc_d, lab_d = _up(pc), _up(c["labels"])
    out = prepare_sample(pc_d, lab_d, _up(idx.astype(np.int64)), num_classes=classes)
    center, scale = out["center"].cpu().numpy(), np.float32(out["scale"].item())
    pos = out["pos"].cpu().numpy()
    # the centroid against the fp64 mean, by the bound derived in _dataprep_ref.centroid_bound
    mean, bound = R.centroid_bound(pc)
    err = np.abs(center.astype(np.float64) - mean)
    print("%s: centroid at %.3f of its bound" % (name, _share("centroid", err, bound)), end="")
    assert (err <= bound).all(), (err, bound)
    # numpy's fp32 statements from OUR centroid: the bits
    q, s = R.norm_given_centroid(pc, center)
    assert s == scale and R.same_bits(pos, q[idx]), R.first_difference(pos, q[idx])
    if n > 1:                                    # (a one-point cloud has scale 0: the positions are 0 / 0, as numpy's)
        print(", scale at %.3f, positions at %.3f; worst so far %s" % (
            _share("scale", abs(float(scale) - c["m64"]), 1e-5 * c["m64"]),
            _share("positions", np.abs(pos - c["q64"][idx]), R.B_POS), {k: round(v, 3) for k, v in WORST.items()}))
        assert abs(float(scale) - c["m64"]) <= 1e-5 * c["m64"]
        assert pos.size == 0 or np.abs(pos - c["q64"][idx]).max() <= R.B_POS
    else:
        assert scale == 0 and np.isnan(pos).all() and np.array_equal(center, pc[0])
    y = out["y"].cpu().numpy()
    assert y.dtype == np.int64 and np.array_equal(y, c["labels"][idx])           # labels outside [0, C) are carried
    assert R.same_bits(out["class_weights"].cpu().numpy(), c["weights"]), (out["class_weights"], c["weights"])
    if m == 0:
        assert pos.shape == (0, 3) and y.shape == (0,) and np.isnan(c["weights"]).all()
    # the C ABI itself, with selected == NULL where the case is the identity: the same bits
    abi = _sample_abi(pc_d, lab_d, _up(c["sel"]), classes, m)
    assert abi["flag"] == 0
    for k in ("pos", "y", "class_weights", "center"):
        assert R.same_bits(abi[k], out[k].cpu().numpy()), k
    assert abi["scale"] == scale
    full, cen, sc = pc_norm(pc_d)                # pc_norm: the identity form without labels
    assert R.same_bits(full.cpu().numpy(), q) and R.same_bits(cen.cpu().numpy(), center) and np.float32(sc.item()) == scale


def test_bad_indices_are_flagged_and_read_point_zero():
    from geot_amd.openpoints.dataset import prepare_sample
    c = R.pn_case("n257")
    n, classes = c["n"], c["classes"]
    pc_d, lab_d = _up(c["pc"]), _up(c["labels"])
    good = np.arange(40, dtype=np.int64) * 3
    for bad in (-1, n, 2 ** 40):
        sel = good.copy()
        sel[[7, 33]] = bad
        zero = good.copy()
        zero[[7, 33]] = 0
        got = _sample_abi(pc_d, lab_d, _up(sel), classes, len(sel))
        want = _sample_abi(pc_d, lab_d, _up(zero), classes, len(sel))
        assert got["flag"] != 0 and want["flag"] == 0
        for k in ("pos", "y", "class_weights"):
            assert R.same_bits(got[k], want[k]), (bad, k)
        with pytest.raises(IndexError):
            prepare_sample(pc_d, lab_d, _up(sel), num_classes=classes)
        quiet = prepare_sample(pc_d, lab_d, _up(sel), num_classes=classes, check=False)
        assert R.same_bits(quiet["pos"].cpu().numpy(), want["pos"])


# ---- the batch ------------------------------------------------------------------------------------------------------------------
def _batch_abi(points, labels, offsets, ids, sel, classes, n_scans, total):
    """geot_cloud_sample_batch itself: ws, bad and every output pre-filled with garbage between sentinel margins.
    points / labels / offsets / sel: device tensors (or views into larger ones); ids: device tensor or None."""
    lib = _lib()
    s, m = sel.shape
    nbytes = int(lib.geot_cloud_sample_batch_ws_bytes(s, classes))
    ws = _garbage(nbytes)
    out = {"raw": Guarded((s, m, 3), torch.float32), "y": Guarded((s, m), torch.int64), "class_weights": Guarded((s, classes), torch.float32),
           "center": Guarded((s, 3), torch.float32), "scale": Guarded((s,), torch.float32), "bad": Guarded((s,), torch.int32)}
    err = lib.geot_cloud_sample_batch(s, m, classes, n_scans, total, points.data_ptr(), labels.data_ptr(), offsets.data_ptr(),
                                      _ptr(ids), sel.data_ptr(), out["raw"].ptr(), out["y"].ptr(), out["class_weights"].ptr(),
                                      out["center"].ptr(), out["scale"].ptr(), out["bad"].ptr(), ws.data_ptr(), nbytes, _stream())
    assert err == 0
    torch.cuda.synchronize()
    assert all(g.intact() for g in out.values())
    return {k: g.numpy() for k, g in out.items()}


def _assert_slot(got, slot, single, what):
    assert R.same_bits(got["raw"][slot], single["pos"]), (what, slot, R.first_difference(got["raw"][slot], single["pos"]))
    assert np.array_equal(got["y"][slot], single["y"]), (what, slot)
    assert R.same_bits(got["class_weights"][slot], single["class_weights"]), (what, slot)
    assert R.same_bits(got["center"][slot], single["center"]) and got["scale"][slot] == single["scale"], (what, slot)


@pytest.mark.parametrize("name", R.BATCH_NAMES)
def test_batch_slots_carry_the_bits_of_the_single_scan_calls(name):
    c = R.batch_case(name)
    classes, m, ids = c["classes"], c["m"], c["ids"]
    sizes = [len(p) for p in c["scans"]]
    points, labels = _up(np.concatenate(c["scans"])), _up(np.concatenate(c["labels"]))
    offsets = _up(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    sel = _up(c["sel"])
    ids_d = None if c["null_ids"] else _up(np.asarray(ids, dtype=np.int64))
    got = _batch_abi(points, labels, offsets, ids_d, sel, classes, len(sizes), sum(sizes))
    assert not got["bad"].any()
    for slot, i in enumerate(ids):
        single = _sample_abi(_up(c["scans"][i]), _up(c["labels"][i]), sel[slot].contiguous(), classes, m)
        _assert_slot(got, slot, single, name)
        assert R.same_bits(single["class_weights"], R.class_weights(c["labels"][i][c["sel"][slot]], classes))
    if not c["null_ids"]:                        # the wrapper on a DeviceScanSet: the same call
        from geot_amd.openpoints.dataset.scan_set import DeviceScanSet, cloud_sample_batch
        out = cloud_sample_batch(DeviceScanSet(c["scans"], c["labels"], device=DEV), ids, c["sel"], num_classes=classes)
        for k in ("raw", "y", "class_weights", "center", "scale", "bad"):
            assert R.same_bits(out[k].cpu().numpy(), got[k]), k


def test_unusable_slots_are_flagged_two_and_zero_filled_beside_untouched_neighbours():
    """Every kind of unusable table entry in one call, between usable slots, one of which has an entry of sel outside its
    scan (flag 1).  The arrays start MARGIN rows inside a larger allocation that also extends past `total`: an entry that
    is refused would, if followed, still be read inside the allocation."""
    t = R.unusable_table()
    total, margin, classes, m = t["total"], t["margin"], 65, 257
    rng = np.random.default_rng(7800)
    pts = torch.from_numpy(rng.standard_normal((total + 2 * margin, 3)).astype(np.float32) * 20).to(DEV)
    lab = torch.from_numpy(rng.integers(0, classes, total + 2 * margin).astype(np.int32)).to(DEV)
    points, labels = pts[margin:], lab[margin:]
    offsets = _up(t["offsets"])
    sizes = np.diff(t["offsets"])

    def sel_for(ids):
        rows, seen = [], 0
        for i in ids:
            n = int(sizes[i]) if 0 <= i < t["n_scans"] and sizes[i] > 0 else 50
            row = np.random.default_rng(7900 + i).integers(0, n, m).astype(np.int64)
            if i == 2:
                seen += 1
                if seen == 1:
                    row[100] = n                 # outside its scan: flag 1, the row is read from vertex 0
            rows.append(row)
        return _up(np.stack(rows))

    ids, clean_ids = t["ids"], t["clean_ids"]
    runs = [_batch_abi(points, labels, offsets, _up(np.asarray(ids, dtype=np.int64)), sel_for(ids), classes, t["n_scans"], total)
            for _ in range(2)]
    clean = _batch_abi(points, labels, offsets, _up(np.asarray(clean_ids, dtype=np.int64)), sel_for(clean_ids), classes,
                       t["n_scans"], total)
    for k in runs[0]:
        assert R.same_bits(runs[0][k], runs[1][k]), k               # two calls, garbage in every buffer: the same bits
    got = runs[0]
    assert clean["bad"].tolist() == [0, 1, 0]
    assert got["bad"].tolist() == [2 if why else {0: 0, 2: 1, 7: 0}[slot] for slot, why in enumerate(t["why"])]
    usable = [slot for slot, why in enumerate(t["why"]) if why is None]
    for slot, why in enumerate(t["why"]):
        if why is None:
            at = usable.index(slot)
            for k in ("raw", "y", "class_weights", "center", "scale"):
                assert R.same_bits(got[k][slot], clean[k][at]), (slot, k)
        else:
            for k in ("raw", "y", "class_weights", "center", "scale"):
                assert not got[k][slot].any() and not np.isnan(got[k][slot]).any(), (why, k, got[k][slot])
    single = _sample_abi(points[300:650].contiguous(), labels[300:650].contiguous(), sel_for([2])[0].contiguous(), classes, m)
    assert single["flag"] != 0
    _assert_slot(got, 2, single, "flag 1")
