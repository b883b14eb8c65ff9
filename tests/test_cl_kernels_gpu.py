"""GPU suite: the point-major FP stage kernels of csrc/channels_last.hip through their C entry points, per launch branch,
against float64.

tests/_cl_ref.py restates the launch geometry (a classifier only: which workgroup takes which rows, through which branch),
holds the case tables (tests/test_cl_plan_cpu.py holds their census) and the float64 referees.  In every test here
GEOT_CL_TILES pins the tile count, so that the geometry does not depend on the device and a few hundred rows reach every
branch; GEOT_CL_TILES_MULT is removed; outputs are pre-filled with NaN; results are compared class by class, and a failure
names the entry point, the case, the class and the first row and channel that differ.

Bounds (u = 2^-24), none of them fitted to what the kernels give:
* fp_front_cl, per element: (4 + CS) u sum |terms| -- one rounding per multiply and add of ((p0 w0 + p1 w1) + p2 w2), one per
  skip fma
* a statistics record of fp_front_cl: count u sum |d| and count u sum d^2, against float64 sums of d = y - pivot over the
  workgroup's own rows.  d is taken as the kernel forms it, ONE correctly rounded fp32 subtraction of two stored fp32 values
  (reproduced to the bit by NumPy), so that the roundings of the sum and of the stored record are all the bound has to cover;
  with d in float64 a record of 2 rows (s2 = fl(fl(y1 - p)^2): three roundings) could miss a bound of 2 u although nothing is
  wrong
* the reduce kernels, per tile: (per + 3) u sum |terms|; the inputs sit on a dyadic grid (x, shift multiples of 1/64 in
  [-4, 4], scale +-{1/2, 1, 2}), so x scale + shift is exact, exact zeros are planted under the strict `> 0` of the mask, and
  bn_apply_cl must equal the referee
* bn_bwd_apply_cl, per element: 6 u |k0| (|g| + |c1| + |xhat c2|)
* the fp64 sums kernels: integer-valued partials, exact equality
* the whole node: tools/cl_fuzz.py's rule and bounds (ReLU inputs within 1e-5 of zero get no upstream gradient on either
  side; forward 1e-5; gradients 2e-5 / 5e-5 / 1e-4 by longest list)

What the 1e-6 bound on (sum y, sum y^2) behind fp_front_cl found: with fp32 accumulators a workgroup of 56 to 303 rows missed
it by up to 15 % (cases "skip cs=2..6", "deal T=1", "deal T=5", "deal granule=128 / 10000": 1.0e-6 to 1.15e-6), because the
sums are those of d = y - pivot and sum d^2 = sum y^2 + n p^2 - ... grows with a pivot a few sigma off the mean; the kernel
now accumulates d and d^2 in fp64: the worst case of this table is 4.3e-7 ("deal T=1", one workgroup of 303 rows), most are
near 2e-7; what is left is the rounding of d and of the fp32 record, which the recombination 2 p s1 scales by (p / sigma)^2.

Value-only faults planted in scratch builds (arithmetic changed, never an address), and the classes that caught them:
* `cnt < CL_STAGE` -> `<=`: "y is written" in the stage-1 row classes, nx1 and nx8 (deal T=1, granule=10000, stage R=1027 /
  2055, tail R=130 / 131)
* pivot taken from the second row: "pivot is the first dealt row of y" in every workgroup class of every case
* `seen` not counted for the last row of an odd group: "row count" in the "tail 1 of 4" / "tail 3 of 4" workgroup classes
* `> 0.f` -> `>= 0.f` in the masks: "sum g" of bn_bwd_reduce_cl and bn_bwd_reduce_skip_cl in every tile class, "dx" of
  bn_bwd_apply_cl (the planted zeros)
* the n p term dropped in bn_sums_shifted_cl: (sum, sum of squares) behind fp_front_cl and bn_stats_cl and in the exact test,
  and the training-mode cases of the whole node
* 8 ranges cut with R / nx: "y is written" in "nx8 stage 0" / "nx8 stage 1" (R = 300, 303, 1027, 2055: not multiples of 8)
* the unrolled loop of bn_sums_cl one tile too far (read clamped): tiles = 63 alone, the only count of the table with a part
  whose tiles end exactly one short of a group of 4
The classes none of these trips name other code: a template instantiation each (CS = 0..8), a block size (widths), the deal
with several workgroups per range (lx > 1, granules), the tails of the 4-row and 2-row loops of the reduce / apply kernels,
empty trailing tiles, a launch block of the weight gradient, the non-finite values.

Not pinned: the sign of a zero result; the backward mask of a NaN input (torch's ReLU backward passes the gradient on, the
kernels' `> 0` drops it -- under batch statistics the channel's gradient is NaN either way).
"""
import copy
import zlib

import numpy as np
import pytest
import torch

import _cl_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]      # each test under its own limit; each takes a second or so

DEV = torch.device("cuda:0")
NAN = float("nan")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


@pytest.fixture(scope="module")
def lib():
    from geot_amd import _lib
    return _lib.load()


@pytest.fixture()
def pin(monkeypatch):
    """pin(T, granule): GEOT_CL_TILES = T, GEOT_CL_GRANULE = granule (None: unset), no GEOT_CL_TILES_MULT"""
    monkeypatch.delenv("GEOT_CL_TILES_MULT", raising=False)
    monkeypatch.delenv("GEOT_CL_GRANULE", raising=False)

    def set_(tiles, granule=None):
        monkeypatch.setenv("GEOT_CL_TILES", str(tiles))
        if granule is None:
            monkeypatch.delenv("GEOT_CL_GRANULE", raising=False)
        else:
            monkeypatch.setenv("GEOT_CL_GRANULE", str(granule))
    return set_


def call(name, *args):
    from geot_amd.ext._common import call as launch
    launch(name, DEV, *args)


def ptr(t):
    return None if t is None else t.data_ptr()


def check(entry, case, labels, field, got, want, bound=None):
    """got, want (rows, channels); labels (rows,): the class of every row; bound (rows, channels), (channels,) or None for
    equality (of values: -0 == +0; NaN == NaN).  Compared class by class: the message names entry point, case, class and the
    first row and channel that differ."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and got.ndim == 2, (entry, field, got.shape, want.shape)
    both_nan = np.isnan(got) & np.isnan(want)
    if bound is None:
        ok = (got == want) | both_nan
    else:
        ok = (np.abs(got - want) <= np.broadcast_to(np.asarray(bound, np.float64), got.shape)) | both_nan
    if ok.all():
        return
    labels = np.asarray(labels, dtype=object)
    for cls in sorted(set(labels.tolist())):
        rows = np.flatnonzero(labels == cls)
        bad = ~ok[rows]
        if bad.any():
            i, ch = np.argwhere(bad)[0]
            r = int(rows[i])
            lim = "" if bound is None else ", bound %.3e" % float(np.broadcast_to(np.asarray(bound, np.float64), got.shape)[r, ch])
            pytest.fail("%s: case %s, class %s, %s: row %d channel %d (%d of the class's %d elements differ): got %.9g want %.9g%s"
                        % (entry, case, cls, field, r, int(ch), int(bad.sum()), bad.size, got[r, ch], want[r, ch], lim))


def bits_equal(a, b):
    return np.ascontiguousarray(a, np.float32).view(np.int32) == np.ascontiguousarray(b, np.float32).view(np.int32)


# ---- geot_fp_front_cl -----------------------------------------------------------------------------------------------
def _fp_inputs(case):
    rng = rng_of(case["name"])
    b, n, m, c, cs = case["b"], case["n"], case["m"], case["c"], case["cs"]
    a = rng.standard_normal((b, m, c)).astype(np.float32)
    idx = rng.integers(0, m, (b, n, 3)).astype(np.int32)
    w = (rng.random((b, n, 3)) + 0.05).astype(np.float32)
    w = (w / w.sum(-1, keepdims=True)).astype(np.float32)
    skip = rng.standard_normal((b, cs, n)).astype(np.float32) if cs else None
    wb = rng.standard_normal((c, cs)).astype(np.float32) if cs else None
    order = np.stack([rng.permutation(n) for _ in range(b)]).astype(np.int32) if case["ordered"] else None
    return a, idx, w, skip, wb, order


@pytest.mark.parametrize("case", R.FP_FRONT_CASES, ids=[c["name"].replace(" ", "_") for c in R.FP_FRONT_CASES])
def test_fp_front_cl_per_class(lib, pin, case):
    b, n, m, c, cs, T = case["b"], case["n"], case["m"], case["c"], case["cs"], case["T"]
    rows = b * n
    entry, name = "geot_fp_front_cl", case["name"]
    a, idx, w, skip, wb, order = _fp_inputs(case)
    pin(T, case["granule"])
    assert lib.geot_fp_front_cl_tiles(b, c, n, cs) == T
    floats = int(lib.geot_cl_stat_floats(T, c))
    assert floats == T * (3 * c + 1)
    d_in = [None if v is None else dev(v) for v in (a, idx, w, skip, wb, order)]
    y_d, part_d = nans(b, n, c), nans(floats)
    call(entry, b, c, m, n, cs, *[ptr(v) for v in d_in], ptr(y_d), ptr(part_d))
    torch.cuda.synchronize()
    y, part = host(y_d).reshape(rows, c), host(part_d)

    # rows: every element written, each within (4 + CS) u sum |terms| of float64
    wg_cls, seq_cls = R.fp_front_classes(b, n, T, case["granule"])
    wg_rows = R.fp_front_rows(b, n, T, case["granule"], order)
    labels = np.empty(rows, dtype=object)
    seq_rows = R.fp_front_rows(b, n, T, case["granule"], None)
    for out_r, seq_r in zip(wg_rows, seq_rows):
        labels[out_r] = seq_cls[seq_r]
    assert all(v is not None for v in labels)                      # the deal covers every output row
    want, mag = R.fp_front_ref(a, idx, w, skip, wb)
    want, mag = want.reshape(rows, c), mag.reshape(rows, c)
    check(entry, name, labels, "y is written", np.isnan(y), np.zeros_like(y))
    err = np.abs(y - want) / np.maximum(mag, 1e-300)
    print("%s %s: max |y - y64| / sum |terms| = %.3f u (bound %d u)" % (entry, name, float(err.max()) / R.U32, 4 + cs))
    check(entry, name, labels, "y", y, want, (4 + cs) * R.U32 * mag)

    # statistics records: (T, 3, c) = (s1, s2, pivot), then T counts
    rec, counts = part[:T * 3 * c].reshape(T, 3, c), part[T * 3 * c:]
    wg_labels = np.array(["workgroup %d: %s" % (k, ", ".join(sorted(s))) for k, s in enumerate(wg_cls)], dtype=object)
    want_counts = np.array([len(r) for r in wg_rows], np.float64)
    check(entry, name, wg_labels, "row count", counts[:, None], want_counts[:, None])
    assert float(counts.sum()) == rows
    if name in R.FP_FRONT_COUNTS:
        assert counts.tolist() == R.FP_FRONT_COUNTS[name]
    ref = [R.shifted_sums_ref(y, r) for r in wg_rows]
    s1, s2, sabs, piv = (np.stack([v[i] for v in ref]) for i in range(4))
    pivot_ok = bits_equal(rec[:, 2], piv)
    check(entry, name, wg_labels, "pivot is the first dealt row of y, bit for bit", pivot_ok, np.ones_like(pivot_ok))
    worst = [float((np.abs(rec[:, i] - s) / np.maximum(want_counts[:, None] * R.U32 * t, 1e-300)).max())
             for i, s, t in ((0, s1, sabs), (1, s2, s2))]
    print("%s %s: worst s1 / s2 error as a fraction of the bound: %.3f / %.3f" % (entry, name, worst[0], worst[1]))
    check(entry, name, wg_labels, "s1 = sum (y - pivot)", rec[:, 0], s1, want_counts[:, None] * R.U32 * sabs)
    check(entry, name, wg_labels, "s2 = sum (y - pivot)^2", rec[:, 1], s2, want_counts[:, None] * R.U32 * s2)

    # through geot_bn_sums_shifted_cl: sum y, sum y^2 at the bound tests/test_channels_last_gpu.py uses
    sums_d = nans(c, 2, dtype=torch.float64)
    call("geot_bn_sums_shifted_cl", T, c, ptr(part_d), ptr(sums_d))
    torch.cuda.synchronize()
    plain = R.plain_sums_ref(y)
    scale = np.stack([np.abs(y.astype(np.float64)).sum(0), plain[:, 1]], 1)
    print("geot_bn_sums_shifted_cl after %s %s: worst error / (sum |y|, sum y^2) = %.2e (bound 1e-6)"
          % (entry, name, float((np.abs(host(sums_d) - plain) / np.maximum(scale, 1e-300)).max())))
    check("geot_bn_sums_shifted_cl after " + entry, name, np.array(["channel"] * c, dtype=object), "(sum y, sum y^2)",
          host(sums_d), plain, 1e-6 * scale)


# ---- reduce and apply kernels ---------------------------------------------------------------------------------------
def _dyadic(case, with_skip=False):
    """x, shift multiples of 1/64 in [-4, 4], scale in +-{1/2, 1, 2}: x scale + shift is exact in fp32; every third channel of
    every fifth row (and all of row 0) sits at a pre-activation of exactly 0"""
    rng = rng_of("reduce " + case["name"] + str(case.get("cs", "")))
    rows, c = case["b"] * case["n"], case["c"]
    x = (rng.integers(-256, 257, (rows, c)) / 64.0).astype(np.float32)
    scale = rng.choice(np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], np.float32), c)
    steps = rng.integers(-256, 257, c)
    steps = np.where(np.abs(scale) == 2.0, 2 * (steps // 2), np.where(np.abs(scale) == 0.5, steps // 2, steps))
    shift = (steps / 64.0).astype(np.float32)                  # such that the zero of every channel is on x's grid too
    zero = (-shift / scale).astype(np.float32)
    assert np.all(np.abs(zero) <= 4) and np.all(zero * 64 == np.round(zero * 64))
    x[::5, ::3] = zero[None, ::3]
    x[0, :] = zero
    assert np.all(x.astype(np.float64) * scale + shift == (x * scale + shift).astype(np.float64))
    assert np.all((x * scale + shift)[0] == 0)
    d = dict(x=x, shift=shift, scale=scale, dz=rng.standard_normal((rows, c)).astype(np.float32),
             mean=(rng.integers(-64, 65, c) / 64.0).astype(np.float32), rstd=(rng.random(c) + 0.5).astype(np.float32),
             k0=rng.standard_normal(c).astype(np.float32), c1=(0.1 * rng.standard_normal(c)).astype(np.float32),
             c2=(0.1 * rng.standard_normal(c)).astype(np.float32))
    if with_skip and case["cs"]:
        d["skip"] = rng.standard_normal((case["b"], case["cs"], case["n"])).astype(np.float32)
    return d


def _tiles_of(lib, case):
    rows = case["b"] * case["n"]
    tiles, per = R.cl_launch_dims(rows, case["c"], case["T"])
    assert lib.geot_cl_tiles(1, rows, case["c"]) == tiles
    rng_ = R.tile_ranges(rows, tiles, per)
    names = []
    for r0, r1 in rng_:
        ln = r1 - r0
        names.append("empty tile" if ln == 0 else "%s tile, %d %% 4 rows%s" % ("full" if ln == per else "short", ln % 4, ", odd" if ln % 2 else ""))
    return tiles, per, rng_, np.array(names, dtype=object)


def _row_labels(rows, ranges, per):
    labels = np.empty(rows, dtype=object)
    for r0, r1 in ranges:
        ln = r1 - r0
        for r in range(r0, r1):
            j = r - r0
            labels[r] = ("full tile" if ln == per else "short tile") + (", tail of the 4-row loop" if j >= ln - ln % 4 else "")
    return labels


_ids = lambda table: [c["name"].replace(" ", "_") for c in table]      # noqa: E731


@pytest.mark.parametrize("case", R.REDUCE_CASES, ids=_ids(R.REDUCE_CASES))
def test_bn_stats_cl_per_tile(lib, pin, case):
    rows, c = case["b"] * case["n"], case["c"]
    pin(case["T"])
    tiles, per, ranges, tile_names = _tiles_of(lib, case)
    d = _dyadic(case)
    x_d, part_d = dev(d["x"]), nans(int(lib.geot_cl_stat_floats(tiles, c)))
    call("geot_bn_stats_cl", rows, c, ptr(x_d), ptr(part_d))
    torch.cuda.synchronize()
    part = host(part_d)
    rec, counts = part[:tiles * 3 * c].reshape(tiles, 3, c), part[tiles * 3 * c:]
    check("geot_bn_stats_cl", case["name"], tile_names, "row count", counts[:, None],
          np.array([[r1 - r0] for r0, r1 in ranges], np.float64))
    ref = [R.shifted_sums_ref(d["x"], np.arange(r0, r1)) for r0, r1 in ranges]
    s1, s2, sabs, piv = (np.stack([v[i] for v in ref]) for i in range(4))
    ok = bits_equal(rec[:, 2], piv)
    check("geot_bn_stats_cl", case["name"], tile_names, "pivot is the tile's first row (zeros for an empty tile)", ok, np.ones_like(ok))
    check("geot_bn_stats_cl", case["name"], tile_names, "s1", rec[:, 0], s1, (per + 3) * R.U32 * sabs)
    check("geot_bn_stats_cl", case["name"], tile_names, "s2", rec[:, 1], s2, (per + 3) * R.U32 * s2)
    sums_d = nans(c, 2, dtype=torch.float64)
    call("geot_bn_sums_shifted_cl", tiles, c, ptr(part_d), ptr(sums_d))
    torch.cuda.synchronize()
    plain = R.plain_sums_ref(d["x"])
    scale = np.stack([np.abs(d["x"].astype(np.float64)).sum(0), plain[:, 1]], 1)
    check("geot_bn_sums_shifted_cl after geot_bn_stats_cl", case["name"], np.array(["channel"] * c, dtype=object), "(sum x, sum x^2)",
          host(sums_d), plain, (per + 3) * R.U32 * scale)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", R.REDUCE_CASES, ids=_ids(R.REDUCE_CASES))
def test_bn_bwd_reduce_cl_per_tile(lib, pin, case, relu):
    rows, c = case["b"] * case["n"], case["c"]
    pin(case["T"])
    tiles, per, ranges, tile_names = _tiles_of(lib, case)
    d = _dyadic(case)
    t = {k: dev(v) for k, v in d.items()}
    part_d = nans(tiles, 2, c)
    call("geot_bn_bwd_reduce_cl", rows, c, relu, ptr(t["x"]), ptr(t["dz"]), ptr(t["scale"]), ptr(t["shift"]), ptr(t["mean"]),
         ptr(t["rstd"]), ptr(part_d))
    torch.cuda.synchronize()
    part = host(part_d)
    ref = [R.bn_bwd_sums_ref(d["x"][r0:r1], d["dz"][r0:r1], d["scale"], d["shift"], d["mean"], d["rstd"], relu) for r0, r1 in ranges]
    want, mag = np.stack([v[0] for v in ref]), np.stack([v[1] for v in ref])
    for k, field in enumerate(("sum g", "sum g xhat")):
        check("geot_bn_bwd_reduce_cl relu=%d" % relu, case["name"], tile_names, field, part[:, k], want[:, k], (per + 3) * R.U32 * mag[:, k])
    sums_d = nans(c, 2, dtype=torch.float64)
    call("geot_bn_sums_cl", tiles, c, ptr(part_d), ptr(sums_d))
    torch.cuda.synchronize()
    check("geot_bn_sums_cl after geot_bn_bwd_reduce_cl relu=%d" % relu, case["name"], np.array(["channel"] * c, dtype=object),
          "(sum g, sum g xhat)", host(sums_d), want.sum(0).T, (per + 3) * R.U32 * mag.sum(0).T)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", R.REDUCE_CASES, ids=_ids(R.REDUCE_CASES))
def test_bn_apply_cl_and_bn_bwd_apply_cl_per_row_class(lib, pin, case, relu):
    rows, c = case["b"] * case["n"], case["c"]
    pin(case["T"])
    tiles, per, ranges, _ = _tiles_of(lib, case)
    labels = _row_labels(rows, ranges, per)
    d = _dyadic(case)
    t = {k: dev(v) for k, v in d.items()}
    out_d = nans(rows, c)
    call("geot_bn_apply_cl", rows, c, relu, ptr(t["x"]), ptr(t["scale"]), ptr(t["shift"]), ptr(out_d))
    torch.cuda.synchronize()
    out = host(out_d)
    entry = "geot_bn_apply_cl relu=%d" % relu
    check(entry, case["name"], labels, "out is written", np.isnan(out), np.zeros_like(out))
    want = R.bn_apply_ref(d["x"], d["scale"], d["shift"], relu)
    assert np.array_equal(want, want.astype(np.float32).astype(np.float64))          # exact in fp32: equality is the bound
    check(entry, case["name"], labels, "out", out, want)
    dx_d = nans(rows, c)
    call("geot_bn_bwd_apply_cl", rows, c, relu, ptr(t["x"]), ptr(t["dz"]), ptr(t["scale"]), ptr(t["shift"]), ptr(t["mean"]),
         ptr(t["rstd"]), ptr(t["k0"]), ptr(t["c1"]), ptr(t["c2"]), ptr(dx_d))
    torch.cuda.synchronize()
    dx = host(dx_d)
    entry = "geot_bn_bwd_apply_cl relu=%d" % relu
    check(entry, case["name"], labels, "dx is written", np.isnan(dx), np.zeros_like(dx))
    want, mag = R.bn_bwd_apply_ref(d["x"], d["dz"], d["scale"], d["shift"], d["mean"], d["rstd"], d["k0"], d["c1"], d["c2"], relu)
    check(entry, case["name"], labels, "dx", dx, want, 6 * R.U32 * mag)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", R.SKIP_REDUCE_CASES, ids=["%s_%s" % (c["name"].replace(" ", "_"), c["cs"]) for c in R.SKIP_REDUCE_CASES])
def test_bn_bwd_reduce_skip_cl_per_tile(lib, pin, case, relu):
    b, n, c, cs = case["b"], case["n"], case["c"], case["cs"]
    rows, K = b * n, 2 + 2 * case["cs"]
    pin(case["T"])
    tiles, per, ranges, tile_names = _tiles_of(lib, case)
    d = _dyadic(case, with_skip=True)
    t = {k: dev(v) for k, v in d.items()}
    part_d = nans(tiles, K, c)
    call("geot_bn_bwd_reduce_skip_cl", b, n, c, cs, relu, ptr(t["x"]), ptr(t["dz"]), ptr(t["scale"]), ptr(t["shift"]), ptr(t["mean"]),
         ptr(t["rstd"]), ptr(t.get("skip")), ptr(part_d))
    torch.cuda.synchronize()
    part = host(part_d)
    skip_rows = d["skip"].transpose(0, 2, 1).reshape(rows, cs) if cs else None      # row r = (bi, e): skip[bi, :, e]
    ref = [R.bn_bwd_sums_ref(d["x"][r0:r1], d["dz"][r0:r1], d["scale"], d["shift"], d["mean"], d["rstd"], relu,
                             None if skip_rows is None else skip_rows[r0:r1]) for r0, r1 in ranges]
    want, mag = np.stack([v[0] for v in ref]), np.stack([v[1] for v in ref])
    entry = "geot_bn_bwd_reduce_skip_cl relu=%d" % relu
    fields = ["sum g", "sum g xhat"] + ["sum g skip_%d" % k for k in range(cs)] + ["sum xhat skip_%d" % k for k in range(cs)]
    for k, field in enumerate(fields):
        check(entry, case["name"], tile_names, field, part[:, k], want[:, k], (per + 3) * R.U32 * mag[:, k])
    sums_d = nans(c, K, dtype=torch.float64)
    call("geot_bn_sums_k_cl", tiles, c, K, ptr(part_d), ptr(sums_d))
    torch.cuda.synchronize()
    check("geot_bn_sums_k_cl after " + entry, case["name"], np.array(["channel"] * c, dtype=object), "the %d sums" % K,
          host(sums_d), want.sum(0).T, (per + 3) * R.U32 * mag.sum(0).T)


# ---- the fp64 sums kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", R.SUMS_TILES)
def test_sums_kernels_add_exactly(lib, pin, tiles):
    """integer-valued partials below 2^20, integer pivots and counts: every float64 sum is exact in any order, so the result must
    equal NumPy's.  (The tile count is an argument here; the knob is pinned like everywhere in this file.)"""
    pin(8)
    rng = rng_of("sums %d" % tiles)
    for c in R.SUMS_C:
        labels = np.array(["channel block %d%s" % (ch // 64, ", partly filled" if (ch // 64 + 1) * 64 > c else "") for ch in range(c)], dtype=object)
        for K in R.SUMS_K:
            part = rng.integers(-(2 ** 20) + 1, 2 ** 20, (tiles, K, c)).astype(np.float32)
            part_d, sums_d = dev(part), nans(c, K, dtype=torch.float64)
            call("geot_bn_sums_k_cl", tiles, c, K, ptr(part_d), ptr(sums_d))
            torch.cuda.synchronize()
            check("geot_bn_sums_k_cl", "tiles=%d c=%d K=%d" % (tiles, c, K), labels, "sums", host(sums_d), part.astype(np.float64).sum(0).T)
            if K == 2:
                sums_d = nans(c, 2, dtype=torch.float64)
                call("geot_bn_sums_cl", tiles, c, ptr(part_d), ptr(sums_d))
                torch.cuda.synchronize()
                check("geot_bn_sums_cl", "tiles=%d c=%d" % (tiles, c), labels, "sums", host(sums_d), part.astype(np.float64).sum(0).T)
        s1 = rng.integers(-(2 ** 20) + 1, 2 ** 20, (tiles, c)).astype(np.float64)
        s2 = rng.integers(0, 2 ** 20, (tiles, c)).astype(np.float64)
        p = rng.integers(-1000, 1001, (tiles, c)).astype(np.float64)
        cnt = rng.integers(0, 1001, tiles).astype(np.float64)
        cnt[rng.integers(0, tiles)] = 0.0
        rec = np.concatenate([np.stack([s1, s2, p], 1).reshape(-1), cnt]).astype(np.float32)
        sums_d = nans(c, 2, dtype=torch.float64)
        rec_d = dev(rec)
        call("geot_bn_sums_shifted_cl", tiles, c, ptr(rec_d), ptr(sums_d))
        torch.cuda.synchronize()
        want = np.stack([(s1 + cnt[:, None] * p).sum(0), (s2 + 2.0 * p * s1 + cnt[:, None] * p * p).sum(0)], 1)
        assert np.abs(want).max() < 2.0 ** 52
        check("geot_bn_sums_shifted_cl", "tiles=%d c=%d" % (tiles, c), labels, "(sum x, sum x^2)", host(sums_d), want)


def test_sums_k_cl_refuses_k_out_of_range(lib, pin):
    pin(8)
    part_d, sums_d = torch.zeros(4 * 19 * 4, device=DEV), torch.zeros(4 * 19, dtype=torch.float64, device=DEV)
    for K in (0, -1, R.CL_MAX_SUMS + 1):
        assert lib.geot_bn_sums_k_cl(4, 4, K, part_d.data_ptr(), sums_d.data_ptr(), None) == R.INVALID, K
    assert lib.geot_bn_sums_k_cl(-1, 4, 2, part_d.data_ptr(), sums_d.data_ptr(), None) == R.INVALID
    assert lib.geot_bn_sums_cl(4, -4, part_d.data_ptr(), sums_d.data_ptr(), None) == R.INVALID
    assert lib.geot_bn_sums_shifted_cl(-4, 4, part_d.data_ptr(), sums_d.data_ptr(), None) == R.INVALID


# ---- geot_fp_skip_wgrad_cl ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,cs", R.WGRAD_CASES)
def test_fp_skip_wgrad_cl_is_exact_on_dyadic_inputs(lib, pin, c, cs):
    pin(8)
    rng = rng_of("wgrad %d %d" % (c, cs))
    K = 2 + 2 * cs
    sums_k = rng.integers(-1000, 1001, (c, K)).astype(np.float64)
    scale = rng.choice(np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], np.float32), c)
    c1 = (rng.integers(-256, 257, c) / 64.0).astype(np.float32)
    c2 = (rng.integers(-256, 257, c) / 64.0).astype(np.float32)
    s2 = rng.integers(-1000, 1001, cs).astype(np.float64)
    want = R.skip_wgrad_ref(sums_k, scale, c1, c2, s2, cs)
    assert np.array_equal(want, want.astype(np.float32).astype(np.float64))          # exact in fp32
    gwb_d = nans(c, cs)
    args = [dev(v) for v in (sums_k, scale, c1, c2, s2)]
    call("geot_fp_skip_wgrad_cl", c, cs, *[ptr(v) for v in args], ptr(gwb_d))
    torch.cuda.synchronize()
    labels = np.array(["launch block %d" % (ch * cs // 256) for ch in range(c)], dtype=object)
    check("geot_fp_skip_wgrad_cl", "c=%d cs=%d" % (c, cs), labels, "grad wb", host(gwb_d), want)
    # cs = 0: nothing to do, the buffer is left as it is
    keep = torch.full((c,), 7.0, device=DEV)
    call("geot_fp_skip_wgrad_cl", c, 0, ptr(args[0]), ptr(args[1]), ptr(args[2]), ptr(args[3]), None, ptr(keep))
    torch.cuda.synchronize()
    assert bool((keep == 7.0).all())


# ---- the whole node -------------------------------------------------------------------------------------------------
def _rel(got, want):
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("ci", range(len(R.NODE_CASES)), ids=["%(kind)s_n%(n)d_m%(m)d_c%(c)d_cs%(cs)d" % c for c in R.NODE_CASES])
def test_whole_node_against_float64(lib, pin, ci):
    """fp_stage_cl and fp_front_cl + bn_act_cl: forward, gradients w.r.t. the table, the skip weights, gamma and beta, and the
    running variance against the same function in float64; a rebuilt reverse index and a rerun give the same bits."""
    from geot_amd import fused_norm as fn
    from geot_amd.synth import make_batch
    from geot_amd.pointnet2 import pointnet2_utils as pu
    case = R.NODE_CASES[ci]
    b, n, m, c, cs = case["b"], case["n"], case["m"], case["c"], case["cs"]
    relu, training, ordered, kind = case["relu"], case["training"], case["ordered"], case["kind"]
    pin(8 if b * n >= 128 else 3)
    pos = torch.from_numpy(make_batch(b, max(n, m), start_index=ci + 1)[0]).to(DEV)
    unknown, known = pos[:, :n].contiguous(), pos[:, :m].contiguous()
    d2, idx = pu._ext.three_nn(unknown, known)
    w = pu._ext.fp_weights(d2)
    if kind == "hub":
        idx = idx.clone()
        idx[:, ::2, 0] = 0
        if m > 2:
            idx[idx == m - 1] = 1
    elif kind == "one":             # the two farther slots of every point on target 0 (all three would make y constant per channel)
        idx = idx.clone()
        idx[:, :, 1:] = 0
    idx = idx.contiguous()
    torch.manual_seed(ci + 1)
    a_cl = torch.randn(b, m, c, device=DEV)
    skip = torch.randn(b, cs, n, device=DEV) if cs else None
    wb = torch.randn(c, cs, device=DEV) if cs else None
    up = torch.randn(b, n, c, device=DEV)
    bn = torch.nn.BatchNorm1d(c).to(DEV)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-0.2, 0.2)
        bn.running_var.uniform_(0.5, 1.5)
    bn.train(training)
    z64, ga64, gwb64, gg64, gb64, bn64, keep = R.node_ref64(a_cl, idx, w, skip, wb, bn, relu, up)
    up = up * keep.to(DEV)
    order_u = fn.local_spatial_order(unknown) if ordered else None
    order_k = fn.local_spatial_order(known) if ordered else None
    assert (order_u is not None) == ordered
    longest = int(torch.bincount((idx.long() + torch.arange(b, device=DEV).view(b, 1, 1) * m).reshape(-1), minlength=b * m).max())
    tol = R.node_grad_tolerance(longest)
    res = {}
    for form in ("fp_stage_cl", "fp_front_cl + bn_act_cl"):
        bn_f = copy.deepcopy(bn)
        a_r = a_cl.clone().requires_grad_(True)
        wb_r = None if wb is None else wb.clone().requires_grad_(True)
        rix = fn.ReverseIndex(idx, w, m, order_k)
        if form == "fp_stage_cl":
            z = fn.fp_stage_cl(bn_f, a_r, idx, w, skip, wb_r, relu, order_u, rix)
        else:
            y, part = fn.fp_front_cl(a_r, idx, w, skip, wb_r, order_u, rix)
            z = fn.bn_act_cl(bn_f, y, relu=relu, partial=part)
        (z * up).sum().backward()
        res[form] = (z.detach(), a_r.grad)
        errs = {"z": _rel(z, z64), "dA": _rel(a_r.grad, ga64), "dgamma": _rel(bn_f.weight.grad, gg64), "dbeta": _rel(bn_f.bias.grad, gb64)}
        if wb_r is not None:
            errs["dWb"] = _rel(wb_r.grad, gwb64)
        if training:
            errs["running_var"] = _rel(bn_f.running_var, bn64.running_var)
        print("%s %s: %s (gradient bound %.0e)" % (form, case, {k: "%.1e" % v for k, v in errs.items()}, tol))
        bad = {k: v for k, v in errs.items() if v > (R.NODE_FORWARD_TOLERANCE if k == "z" else tol)}
        assert not bad, "%s, case %s: relative error against float64 over the bound (%.0e forward, %.0e gradients): %s" % (
            form, case, R.NODE_FORWARD_TOLERANCE, tol, bad)
    # a rebuilt reverse index, a rerun: the same bits
    a_r = a_cl.clone().requires_grad_(True)
    z2 = fn.fp_stage_cl(copy.deepcopy(bn), a_r, idx, w, skip, None if wb is None else wb.clone().requires_grad_(True), relu, order_u,
                        fn.ReverseIndex(idx, w, m, order_k))
    (z2 * up).sum().backward()
    assert torch.equal(z2, res["fp_stage_cl"][0]) and torch.equal(a_r.grad, res["fp_stage_cl"][1])


# ---- non-finite activations -----------------------------------------------------------------------------------------
SPECIAL = np.array([np.nan, np.inf, -np.inf], np.float32)


def _nonfinite_rows(rows, c, seed, per):
    """dyadic x (rows, c) with NaN, +inf and -inf planted in every column (per = "column": the scale goes by column) or in
    every row (per = "row"); -> (x, the class of every element)"""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-256, 257, (rows, c)) / 64.0).astype(np.float32)
    for si in range(3):
        if per == "column":
            assert rows >= 16
            x[(3 * np.arange(c) + 5 * si + 1) % rows, np.arange(c)] = SPECIAL[si]
        else:
            assert c >= 5
            x[np.arange(rows), (np.arange(rows) + 2 * si) % c] = SPECIAL[si]
    cls = np.where(np.isnan(x), "NaN", np.where(np.isposinf(x), "+inf", np.where(np.isneginf(x), "-inf", "finite")))
    assert all((cls == name).sum() == (c if per == "column" else rows) for name in ("NaN", "+inf", "-inf"))
    return x, cls


def _want_apply(x, scale, shift, relu):
    z = torch.from_numpy(x).double() * torch.from_numpy(scale).double() + torch.from_numpy(shift).double()
    return (torch.relu(z) if relu else z).numpy()


@pytest.mark.parametrize("relu", [0, 1])
def test_bn_apply_cl_propagates_non_finite_values(lib, pin, relu):
    """NaN -> NaN; +-inf follows the sign of the scale; -inf under a positive scale with ReLU -> 0: what torch gives"""
    pin(3)
    for rows, c in ((37, 8), (19, 260)):
        x, cls = _nonfinite_rows(rows, c, rows, "column")
        scale = np.tile(np.array([0.5, -2.0, 1.0, -1.0], np.float32), c // 4)
        shift = (np.random.default_rng(c).integers(-256, 257, c) / 64.0).astype(np.float32)
        want = _want_apply(x, scale[None, :], shift[None, :], relu)
        assert np.isnan(want[cls == "NaN"]).all() and (want[(cls == "-inf") & (scale[None, :] > 0).repeat(rows, 0)] == (0 if relu else -np.inf)).all()
        out_d, x_d, scale_d, shift_d = nans(rows, c), dev(x), dev(scale), dev(shift)
        call("geot_bn_apply_cl", rows, c, relu, ptr(x_d), ptr(scale_d), ptr(shift_d), ptr(out_d))
        torch.cuda.synchronize()
        out = host(out_d)
        for name in ("NaN", "+inf", "-inf", "finite"):
            sel = cls == name
            labels = np.array(["x = %s, scale %s 0" % (name, ">" if s > 0 else "<") for s in np.broadcast_to(scale, x.shape)[sel]], dtype=object)
            check("geot_bn_apply_cl relu=%d" % relu, "%d x %d" % (rows, c), labels, "out", out[sel][:, None], want[sel][:, None])


@pytest.mark.parametrize("relu", [0, 1])
def test_bn_apply_propagates_non_finite_values(lib, pin, relu):
    """the channels-first kernel, through its float4 body, its tail and its unaligned rows (l = 7: rows start at any word)"""
    pin(3)
    for b, c, l in ((2, 4, 16), (2, 3, 7), (1, 5, 9)):
        x, cls = _nonfinite_rows(b * c, l, l, "row")
        rng = np.random.default_rng(l)
        scale = np.array([0.5, -2.0, 1.0, -1.0, 2.0], np.float32)[:c]
        shift = (rng.integers(-256, 257, c) / 64.0).astype(np.float32)
        want = _want_apply(x.reshape(b, c, l), scale[None, :, None], shift[None, :, None], relu).reshape(b * c, l)
        out_d, x_d, scale_d, shift_d = nans(b, c, l), dev(x), dev(scale), dev(shift)
        call("geot_bn_apply", b, c, l, relu, ptr(x_d), ptr(scale_d), ptr(shift_d), ptr(out_d))
        torch.cuda.synchronize()
        out = host(out_d).reshape(b * c, l)
        labels = np.array(["row (b, c) = (%d, %d), scale %s 0, %s" % (r // c, r % c, ">" if scale[r % c] > 0 else "<",
                                                                      "/".join(sorted(set(cls[r].tolist())))) for r in range(b * c)], dtype=object)
        check("geot_bn_apply relu=%d" % relu, "%d x %d x %d" % (b, c, l), labels, "out", out, want)


@pytest.mark.parametrize("layout,relu", [("cl", False), ("cl", True), ("cf", False), ("cf", True), ("pool", True)])
def test_one_nan_in_a_training_batch_makes_its_channel_nan(lib, pin, layout, relu):
    """BatchNorm1d (+ ReLU) in training mode with a single NaN in the batch: mean, scale and shift of its channel are NaN and
    the whole channel comes out NaN, as torch gives in float64 on the CPU -- not zeros (a diverged run must stay visible).
    Through bn_act_cl, bn_act, and the pooled form bn_relu_max (which has a ReLU)."""
    from geot_amd import fused_norm as fn
    pin(3)
    b, l, c, hit = 2, 64, 8, 5
    torch.manual_seed(9)
    x = torch.randn(b, c, l, device=DEV) * 2 + 0.5               # channels-first view of the batch
    x[1, hit, 17] = NAN
    bn = torch.nn.BatchNorm1d(c).to(DEV).train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    ref = copy.deepcopy(bn).double().cpu()
    want = ref(x.double().cpu())
    want = torch.relu(want) if relu else want
    if layout == "cl":
        got = fn.bn_act_cl(bn, x.transpose(1, 2).contiguous(), relu=relu).transpose(1, 2)
    elif layout == "cf":
        got = fn.bn_act(bn, x, relu=relu)
    else:
        got = fn.bn_relu_max(bn, x, 16)
        want = want.view(b, c, l // 16, 16).max(-1)[0]
    torch.cuda.synchronize()
    got, want = got.detach().cpu().double(), want.detach()
    assert bool(torch.isnan(want[:, hit]).all())
    assert bool(torch.isnan(got[:, hit]).all()), "%s relu=%s: the NaN's channel came out as %s" % (layout, relu, got[:, hit].flatten()[:6].tolist())
    others = [ch for ch in range(c) if ch != hit]
    assert bool(torch.isfinite(got[:, others]).all())
    assert float((got[:, others] - want[:, others]).abs().max() / want[:, others].abs().max()) <= 1e-5
