"""Shared by the tests of the point-major FP stage kernels (csrc/channels_last.hip): a NumPy restatement of the launch
geometry, used as a CLASSIFIER only (which workgroup takes which rows, through which branch), the fixed case tables of
tests/test_cl_kernels_gpu.py (tests/test_cl_plan_cpu.py holds their census), and the float64 referees.

Geometry.  Every *_cl launch has T = geot_cl_tiles / geot_fp_front_cl_tiles workgroups: "CUs x workgroups per CU" (or
GEOT_CL_TILES), capped at ceil(rows / 16), at least 1.  The reduce / apply kernels give workgroup t the rows
[t per, min(R, (t + 1) per)), per = ceil(R / T): trailing workgroups can be empty.  fp_front_cl deals rows instead (cl_deal):
with T a multiple of 8 the R rows are cut into 8 ranges [R x / 8, R (x + 1) / 8), one per XCD x = block % 8, else there is one
range; the lx workgroups of a range take its granules of g rows in turn, workgroup l the granules l, l + lx, l + 2 lx ...
The i-th row of a workgroup is a + (l + (i / g) lx) g + i % g, valid while below b; a workgroup stages CL_STAGE = 128 of
them at a time and leaves at the first stage with fewer (a stage of 0 rows when its count is a multiple of 128).

Referees.  Plain float64 NumPy of the same operations; where a kernel forms an intermediate by ONE correctly rounded fp32
operation on stored fp32 values (the shifted sums' d = y - pivot), the referee takes that value to the bit and sums in
float64, so that the bound counts the roundings of the sum alone.  The whole-node referee is torch in float64 on the CPU."""
import numpy as np

U32 = 2.0 ** -24
CL_STAGE = 128
CL_FP_U, CL_FP_STAGES = 2, 2
CL_MAX_SKIP = 8
CL_MAX_THREADS = 1024
CL_MAX_SUMS = 2 + 2 * CL_MAX_SKIP
INVALID = 1                       # hipErrorInvalidValue


# ---- launch geometry ------------------------------------------------------------------------------------------------
def cl_block(c4):
    return (c4 + 63) & ~63


def cl_dims_ok(rows, c):
    return rows > 0 and c >= 4 and c % 4 == 0 and c // 4 <= CL_MAX_THREADS


def cl_tiles_for(rows, c, pinned=None, cus=256, per_cu=None):
    """cl_tiles_for / fp_front_cl_tiles: pinned = GEOT_CL_TILES (None or <= 0: unset); per_cu: workgroups per CU (the
    reduce / apply kernels: 32 / waves; fp_front_cl: what the occupancy query says)"""
    if pinned is not None and pinned > 0:
        t = pinned
    else:
        waves = (c // 4 + 63) // 64
        t = cus * (max(32 // waves, 1) if per_cu is None else per_cu)
    t = min(t, (rows + 15) // 16)
    return max(t, 1)


def cl_launch_dims(rows, c, pinned=None, cus=256):
    """-> (tiles, per) of the reduce / apply launches"""
    tiles = cl_tiles_for(rows, c, pinned, cus)
    return tiles, (rows + tiles - 1) // tiles


def tile_ranges(rows, tiles, per):
    """[r0, r1) of every workgroup of a reduce / apply launch (r0 == r1: an empty trailing tile)"""
    return [(min(rows, t * per), min(rows, (t + 1) * per)) for t in range(tiles)]


def granule_of(setting, R, T):
    """GEOT_CL_GRANULE as geot_fp_front_cl reads it: None = unset -> 8; < 1 -> one contiguous run per workgroup"""
    g = 8 if setting is None else int(setting)
    return g if g >= 1 else (R + T - 1) // T


def cl_deal(R, T, g, block):
    """ClDeal of workgroup `block` of T"""
    nx = 8 if (T >= 8 and T % 8 == 0) else 1
    x = block % nx
    return dict(nx=nx, a=R * x // nx, b=R * (x + 1) // nx, l=block // nx, lx=T // nx, g=g)


def deal_row(d, i):
    return d["a"] + (d["l"] + (i // d["g"]) * d["lx"]) * d["g"] + i % d["g"]


def deal_rows(R, T, g, block):
    """the sequence positions workgroup `block` takes, in the order it takes them: the kernel's loop, stage by stage, the
    stage's count = 1 + the last valid slot, out at the first stage that is not full"""
    d = cl_deal(R, T, g, block)
    out, base, i = [], 0, np.arange(CL_STAGE, dtype=np.int64)
    while True:
        r = deal_row(d, base + i)
        ok = r < d["b"]
        cnt = int(np.flatnonzero(ok)[-1]) + 1 if ok.any() else 0
        out.append(r[ok])
        if cnt < CL_STAGE:
            break
        base += CL_STAGE
    return np.concatenate(out)


def deal_table(R, T, g):
    """the whole launch at once: (rows (T, I) of every workgroup's slots i = 0 .. I - 1, valid (T, I)), I past every range's end"""
    nx = 8 if (T >= 8 and T % 8 == 0) else 1
    blk = np.arange(T, dtype=np.int64)[:, None]
    x, l, lx = blk % nx, blk // nx, T // nx
    a, b = R * x // nx, R * (x + 1) // nx
    i = np.arange(int((b - a).max()) + 1, dtype=np.int64)[None, :]
    r = a + (l + (i // g) * lx) * g + i % g
    return r, r < b


def stage_counts(count):
    """rows of every stage a workgroup with `count` rows runs, the last, short one included (0: the `cnt == 0` exit)"""
    return [CL_STAGE] * (count // CL_STAGE) + [count % CL_STAGE]


def fp_front_rows(b, n, T, granule, order=None):
    """per workgroup: the OUTPUT rows (bi n + e) in the order the workgroup computes them; order (b, n) per-cloud ids"""
    R = b * n
    g = granule_of(granule, R, T)
    out = []
    for blk in range(T):
        r = deal_rows(R, T, g, blk)
        if order is not None:
            bi = r // n
            r = bi * n + np.asarray(order).reshape(-1)[r]
        out.append(r)
    return out


def fp_front_classes(b, n, T, granule):
    """-> (per workgroup class names, per sequence position the class of the row).  A workgroup: its range form, whether it is
    empty, how its stage loop ends, the pipeline tail of its last stage.  A row: stage, and whether it sits in the last,
    partial group of S U = 4 rows / is the odd last row of a pair."""
    R = b * n
    g = granule_of(granule, R, T)
    wg, row_cls = [], np.empty(R, dtype=object)
    su = CL_FP_U * CL_FP_STAGES
    for blk in range(T):
        d = cl_deal(R, T, g, blk)
        rows = deal_rows(R, T, g, blk)
        st = stage_counts(len(rows))
        names = {"nx%d" % d["nx"], "lx1" if d["lx"] == 1 else "lx>1"}
        if len(rows) == 0:
            names.add("empty workgroup")
        else:
            names.add("%s" % ("1 stage" if len(st) == 1 else "2 stages" if len(st) == 2 else "3+ stages"))
            names.add("exit: cnt == 0" if st[-1] == 0 else "exit: short stage")
            if st[-1]:
                names.add("tail %d of 4" % (st[-1] % su))
            if np.any(np.diff(rows) > 1):
                names.add("strided granules")
            if np.any(np.diff(rows // n) > 0):
                names.add("cloud boundary inside the run")
        wg.append(names)
        for i, r in enumerate(rows):
            s, j, cnt = i // CL_STAGE, i % CL_STAGE, st[min(i // CL_STAGE, len(st) - 1)]
            name = "nx%d stage %d" % (d["nx"], min(s, 2))
            if j >= cnt - cnt % su:
                name += ", partial group" + (", odd last row" if (cnt % CL_FP_U and j == cnt - 1) else "")
            row_cls[r] = name
    return wg, row_cls


# ---- case tables of tests/test_cl_kernels_gpu.py -----------------------------------------------------------------
def _fp(name, b, n, m, c, cs, T, granule=None, ordered=False):
    return dict(name=name, b=b, n=n, m=m, c=c, cs=cs, T=T, granule=granule, ordered=ordered)


FP_FRONT_CASES = (
    # width: c4 in {1, 63, 64, 65, 1024} -> blocks of 64, 64, 64, 128, 1024 threads; 8 ranges of one workgroup, counts 37 / 38
    [_fp("width c=%d" % c, 2, 150, 50, c, 2, 8, ordered=bool(i & 1)) for i, c in enumerate((4, 252, 256, 260, 4096))]
    # every skip instantiation; one range of 5 workgroups
    + [_fp("skip cs=%d" % cs, 3, 101, 3, 260, cs, 5, ordered=bool(cs & 1)) for cs in range(9)]
    # the deal: T, granule
    + [_fp("deal T=%d" % T, 3, 101, 50, 68, 1, T, ordered=bool(i & 1)) for i, T in enumerate((1, 5, 8, 12, 16))]
    + [_fp("deal T=24 R=1200", 3, 400, 50, 68, 1, 24, ordered=True)]
    + [_fp("deal granule=%s" % g, 3, 101, 1, 68, 3, 5, granule=g, ordered=bool(i & 1)) for i, g in enumerate((1, 0, 128, 10000))]
    # the stage loop
    + [_fp("stage R=1027", 13, 79, 50, 12, 1, 8, ordered=True), _fp("stage R=2055", 5, 411, 3, 12, 0, 8)]
    + [_fp("tail R=%d" % (b * n), b, n, 3, 8, 2, 1, ordered=(b * n) % 3 == 0)
       for b, n in ((1, 1), (1, 2), (1, 3), (1, 5), (2, 3), (1, 7), (2, 65), (1, 131))]
)

# what the census must find: workgroup classes, and the counts the cases were chosen for
FP_FRONT_WG_CLASSES = ("nx1", "nx8", "lx1", "lx>1", "empty workgroup", "1 stage", "2 stages", "3+ stages", "exit: cnt == 0",
                       "exit: short stage", "tail 0 of 4", "tail 1 of 4", "tail 2 of 4", "tail 3 of 4", "strided granules",
                       "cloud boundary inside the run")
FP_FRONT_COUNTS = {
    "width c=260": [37, 38, 37, 38, 37, 38, 37, 38],
    "deal granule=128": [128, 128, 47, 0, 0],
    "deal granule=10000": [303, 0, 0, 0, 0],
    "deal T=24 R=1200": [54] * 8 + [48] * 16,      # lx = 3: the first workgroup of every range takes 7 granules, the others 6
    "stage R=1027": [128, 128, 129, 128, 128, 129, 128, 129],
    "stage R=2055": [256, 257, 257, 257, 257, 257, 257, 257],
}


def _rd(name, b, n, c, T):
    return dict(name=name, b=b, n=n, c=c, T=T)


ROW_CASES = (
    _rd("R=1", 1, 1, 68, 8), _rd("R=16", 1, 16, 68, 8), _rd("R=17", 1, 17, 68, 8), _rd("R=33", 3, 11, 68, 2),
    _rd("R=70", 2, 35, 68, 4), _rd("R=57", 3, 19, 68, 3), _rd("R=1025", 25, 41, 68, 64),
)
WIDTHS = (4, 252, 256, 260, 4096)
REDUCE_CASES = ROW_CASES + tuple(_rd("width c=%d" % c, 3, 11, c, 2) for c in WIDTHS) + (_rd("width c=260 R=1025", 25, 41, 260, 64),)
SKIP_REDUCE_CASES = (tuple(dict(_rd("cs=%d" % cs, 3, 11, 260, 2), cs=cs) for cs in range(9))
                     + tuple(dict(r, cs=cs) for r, cs in zip(ROW_CASES, (0, 3, 8, 1, 2, 5, 8)))
                     + tuple(dict(_rd("width c=%d" % c, 3, 11, c, 2), cs=cs) for c, cs in zip(WIDTHS, (1, 2, 8, 3, 4))))
REDUCE_CLASSES = ("one tile", "per % 4 == 0", "per % 4 == 1", "per % 4 == 2", "per % 4 == 3", "odd per", "short last tile",
                  "empty trailing tiles", "cloud boundary inside a tile")


def reduce_classes(case):
    R = case["b"] * case["n"]
    tiles, per = cl_launch_dims(R, case["c"], case["T"])
    rng_ = tile_ranges(R, tiles, per)
    names = {"per %% 4 == %d" % (per % 4)}
    if tiles == 1:
        names.add("one tile")
    if per % 2:
        names.add("odd per")
    lens = [r1 - r0 for r0, r1 in rng_]
    if any(0 < v < per for v in lens):
        names.add("short last tile")
    if any(v == 0 for v in lens):
        names.add("empty trailing tiles")
    if any(r1 > r0 and (r1 - 1) // case["n"] > r0 // case["n"] for r0, r1 in rng_):
        names.add("cloud boundary inside a tile")
    return names


SUMS_TILES = (1, 15, 16, 17, 63, 64, 65, 200)
SUMS_C = (4, 60, 64, 68, 260)
SUMS_K = (2, 4, 18)
WGRAD_CASES = tuple((32, cs) for cs in range(1, 9)) + ((36, 8), (64, 4), (68, 4), (260, 1), (260, 5))

# whole node: cl_fuzz.py's axes at their smallest sizes, every value of every axis, both forms per case
NODE_CASES = tuple(dict(zip(("b", "n", "m", "c", "cs", "relu", "training", "ordered", "kind"), v)) for v in (
    (2, 33, 3, 252, 0, True, True, False, "nn"),
    (2, 33, 17, 260, 1, False, True, True, "hub"),
    (3, 257, 3, 260, 8, True, True, True, "one"),
    (1, 257, 17, 252, 1, True, False, False, "nn"),
    (2, 257, 17, 260, 0, False, False, True, "one"),
    (3, 33, 3, 252, 8, False, True, False, "hub"),
    (2, 257, 3, 252, 8, True, False, True, "hub"),
    (1, 33, 17, 260, 0, True, True, True, "nn"),
    (2, 257, 17, 252, 1, False, True, False, "one"),
    (3, 257, 17, 260, 8, True, True, False, "nn"),
))


# ---- float64 referees -----------------------------------------------------------------------------------------------
def fp_front_ref(a, idx, w, skip, wb):
    """a (b, m, c), idx / w (b, n, 3), skip (b, cs, n) or None, wb (c, cs) -> (y (b, n, c), sum of |terms| (b, n, c)) in float64"""
    a64, w64 = a.astype(np.float64), w.astype(np.float64)
    b, n = idx.shape[:2]
    g = a64[np.arange(b)[:, None, None], idx]                      # (b, n, 3, c)
    y = (g * w64[..., None]).sum(2)
    mag = (np.abs(g) * np.abs(w64)[..., None]).sum(2)
    if skip is not None and skip.shape[1]:
        s64, wb64 = skip.astype(np.float64).transpose(0, 2, 1), wb.astype(np.float64)
        y = y + s64 @ wb64.T
        mag = mag + np.abs(s64) @ np.abs(wb64).T
    return y, mag


def shifted_sums_ref(y32, rows):
    """The statistics record of one workgroup over its rows of y32 (R, c) fp32, in the order it takes them: pivot = its
    first row; d = y - pivot as the kernel forms it, one correctly rounded fp32 subtraction; -> (s1, s2, sum |d|, pivot) with
    the sums in float64.  No rows: zeros."""
    c = y32.shape[1]
    if len(rows) == 0:
        z = np.zeros(c)
        return z, z, z, np.zeros(c, np.float32)
    piv = y32[rows[0]]
    d = (y32[rows] - piv[None, :]).astype(np.float64)               # fp32 - fp32 in fp32, then widened
    return d.sum(0), (d * d).sum(0), np.abs(d).sum(0), piv


def plain_sums_ref(y):
    """-> (c, 2): sum y, sum y^2 over all leading axes, float64"""
    y64 = y.astype(np.float64).reshape(-1, y.shape[-1])
    return np.stack([y64.sum(0), (y64 * y64).sum(0)], 1)


def bn_apply_ref(x, scale, shift, relu):
    """max(x scale + shift, 0 or -inf) in float64 (NaN propagates: np.maximum)"""
    z = x.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)
    return np.maximum(z, 0.0) if relu else z


def bn_mask_g(x, dz, scale, shift, relu):
    """g = dz [x scale + shift > 0] (strictly), float64"""
    g = dz.astype(np.float64)
    if relu:
        g = g * (x.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64) > 0)
    return g


def bn_bwd_sums_ref(x, dz, scale, shift, mean, rstd, relu, skip_rows=None):
    """x, dz (rows, c); skip_rows (rows, cs) or None -> (sums (K, c), sums of |terms| (K, c)), K = 2 + 2 cs:
    [0] sum g  [1] sum g xhat  [2 + k] sum g skip_k  [2 + cs + k] sum xhat skip_k"""
    g = bn_mask_g(x, dz, scale, shift, relu)
    xh = (x.astype(np.float64) - mean.astype(np.float64)) * rstd.astype(np.float64)
    terms = [g, g * xh]
    if skip_rows is not None:
        s = skip_rows.astype(np.float64)
        terms += [g * s[:, k:k + 1] for k in range(s.shape[1])] + [xh * s[:, k:k + 1] for k in range(s.shape[1])]
    return np.stack([t.sum(0) for t in terms]), np.stack([np.abs(t).sum(0) for t in terms])


def bn_bwd_apply_ref(x, dz, scale, shift, mean, rstd, k0, c1, c2, relu):
    """-> (k0 (g - c1 - xhat c2), |k0| (|g| + |c1| + |xhat c2|)) float64"""
    g = bn_mask_g(x, dz, scale, shift, relu)
    xh = (x.astype(np.float64) - mean.astype(np.float64)) * rstd.astype(np.float64)
    k, a, b = k0.astype(np.float64), c1.astype(np.float64), c2.astype(np.float64)
    return k * (g - a - xh * b), np.abs(k) * (np.abs(g) + np.abs(a) + np.abs(xh * b))


def skip_wgrad_ref(sums_k, scale, c1, c2, s2, cs):
    """grad_wb[c, j] = scale_c (S1[c, j] - c1_c S2[j] - c2_c S3[c, j]), float64"""
    s1, s3 = sums_k[:, 2:2 + cs], sums_k[:, 2 + cs:2 + 2 * cs]
    return scale.astype(np.float64)[:, None] * (s1 - c1.astype(np.float64)[:, None] * s2[None, :] - c2.astype(np.float64)[:, None] * s3)


def node_ref64(a_cl, idx, w, skip, wb, bn, relu, up):
    """The whole FP node -- interpolation + skip GEMV, BatchNorm1d (training or eval mode, as `bn` stands), ReLU -- and its
    gradients, with torch ops in float64 on the CPU.
    -> (z, grad a, grad wb or None, grad gamma, grad beta, the float64 module, keep)

    A ReLU input within fp32 rounding of zero has no defined mask at this precision (any two fp32 evaluations may disagree
    and move a whole gradient element): those elements (|input| <= 1e-5) get no upstream gradient, in the referee and -- the
    caller multiplies `up` by `keep` -- on the GPU alike."""
    import torch
    a64 = a_cl.double().cpu().requires_grad_(True)
    wb64 = None if wb is None else wb.double().cpu().requires_grad_(True)
    b, m, c = a64.shape
    n = idx.shape[1]
    g = torch.gather(a64, 1, idx.cpu().long().reshape(b, n * 3, 1).expand(-1, -1, c)).view(b, n, 3, c)
    y = (g * w.double().cpu().unsqueeze(-1)).sum(2)
    if skip is not None:
        y = y + torch.matmul(skip.double().cpu().transpose(1, 2), wb64.t())
    bn64 = torch.nn.BatchNorm1d(c).double()
    bn64.load_state_dict({k: v.double().cpu() if v.dtype.is_floating_point else v.cpu() for k, v in bn.state_dict().items()})
    bn64.train(bn.training)
    pre = bn64(y.transpose(1, 2)).transpose(1, 2)
    z = torch.relu(pre) if relu else pre
    keep = (pre.detach().abs() > 1e-5) if relu else torch.ones_like(pre, dtype=torch.bool)
    up64 = up.double().cpu() * keep
    (z * up64).sum().backward()
    return z.detach(), a64.grad, None if wb64 is None else wb64.grad, bn64.weight.grad, bn64.bias.grad, bn64, keep


def node_grad_tolerance(longest):
    """a list of N pairs is summed in fp32 in list order: error grows like sqrt(N) eps x (sum |terms| / |result|)"""
    return 1e-4 if longest > 2000 else (5e-5 if longest > 256 else 2e-5)


NODE_FORWARD_TOLERANCE = 1e-5
