"""Shared by the forward-gather tests (csrc/gather_group.hip): the host-only plan query of geot_gather_points /
geot_group_points / geot_three_interpolate[_into] (geot_gather_plan), the planner restated in Python, a classifier that says
which branches of table_gather_lds_kernel and tlds_load_rows a shape reaches, the case table of the GPU tests with its
inputs, and the referees.  The referees use numpy and torch on the CPU only.

Three kinds of referee:
* exact: a copy (table[idx]) or ONE fp32 operation; the kernel must give the same bits
* an fp32 restatement, operation by operation in the kernel's stated order (the library is built with -ffp-contract=off): the
  same bits again; each comes with its fp64 value and a bound gamma(k) * sum |terms| that the restatement itself has to meet
  (tests/test_gather_plan_cpu.py), k being the roundings a term passes through
* float atomics (any order): the fp64 scatter-add with gamma(n + 1) * sum |terms| per element, n the number of
  contributions that land on the element, counted from the indices; plus integer-valued inputs whose partial sums stay
  below 2^24, which must come out exact in any order"""
import ctypes
import zlib

import numpy as np
import torch

from _fused_ref import gamma

NONE, PLAIN, LDS = 0, 1, 2                        # forms, as geot_gather_plan returns them
FORM_NAMES = {NONE: "none", PLAIN: "plain", LDS: "lds"}
PLAN_FIELDS = ("ch", "chunks", "slices", "per", "lds")
TLDS_FLOATS = 36864                               # floats of table rows a workgroup keeps in LDS (144 KB)
TLDS_THREADS = 1024
PASS = 4 * TLDS_THREADS                           # U = 4 elements per thread and pass
F32 = np.float32


def plan(lib, b, c, m, L):
    """(form, {field: value} for the LDS form else None) of one call shape, from the library"""
    out = (ctypes.c_longlong * len(PLAN_FIELDS))(*([-7] * len(PLAN_FIELDS)))
    form = lib.geot_gather_plan(int(b), int(c), int(m), int(L), out, len(PLAN_FIELDS))
    return form, (dict(zip(PLAN_FIELDS, out)) if form == LDS else None)


def plan_ref(b, c, m, L, impl=None):
    """the planner restated: same answer as plan() must give (impl: the value of GEOT_GATHER_IMPL)"""
    if b < 1 or c < 1 or L < 1:
        return NONE, None
    if (impl or "").startswith("p") or m < 1 or m > TLDS_FLOATS or L * c < 65536:
        return PLAIN, None
    ch = min(TLDS_FLOATS // m, 16, c)
    chunks = -(-c // ch)
    want = -(-512 // (chunks * b))
    maxs = max(L // 4096, 1)
    slices = min(64, max(1, min(max(want, 1), maxs)))
    return LDS, {"ch": ch, "chunks": chunks, "slices": slices, "per": -(-L // slices), "lds": ch * m * 4}


def classes(b, c, m, L, table_off=0):
    """the branches of table_gather_lds_kernel / tlds_load_rows an LDS-form launch of this shape reaches, as a set of names
    (table_off: floats between a 16-byte boundary and the table's first element); empty for the plain form"""
    form, p = plan_ref(b, c, m, L)
    if form != LDS:
        return set()
    got = {"ch=%d" % p["ch"], "slices=%d" % p["slices"]}
    for bi in range(b):
        for cy in range(p["chunks"]):
            c0 = cy * p["ch"]
            nch = min(p["ch"], c - c0)
            count = nch * m
            if nch < p["ch"]:
                got.add("partial chunk")
            if (table_off + (bi * c + c0) * m) % 4 == 0:
                got.add("loader 16-byte")
                if count % 4:
                    got.add("loader count % 4 tail")
                if count // 4 > 4 * TLDS_THREADS:
                    got.add("loader second trip")
            else:
                got.add("loader scalar")
                if count > 4 * TLDS_THREADS:
                    got.add("loader second trip")
    for s in range(p["slices"]):
        n = min(L, (s + 1) * p["per"]) - s * p["per"]
        if 0 < n < p["per"]:
            got.add("short last slice")
        if n < PASS:
            got.add("short pass")
        if n > PASS:
            got.add("second pass")
        if n % PASS:
            got.add("pass tail")
    return got


# (name, (b, c, m, L), expected form, expected plan fields): the case table of tests/test_gather_forward_gpu.py
LDS_CASES = [
    ("gate, below", (1, 16, 64, 4095), PLAIN, {}),
    ("gate, above", (1, 16, 64, 4096), LDS, {"slices": 1, "ch": 16}),
    ("LDS budget, largest table", (1, 2, 36864, 32768), LDS, {"ch": 1, "lds": 144 * 1024, "slices": 8}),
    ("LDS budget, one over", (1, 2, 36865, 32768), PLAIN, {}),
    ("ch capped by c, short last slice", (2, 3, 100, 21846), LDS, {"ch": 3, "slices": 5, "per": 4370}),
    ("ch 15", (1, 16, 2305, 4096), LDS, {"ch": 15, "chunks": 2}),
    ("ch 16", (1, 16, 2304, 4096), LDS, {"ch": 16, "chunks": 1}),
    ("partial chunk, odd m", (3, 19, 777, 4001), LDS, {"ch": 16, "chunks": 2, "slices": 1}),
    ("slices, exactly two", (1, 8, 100, 8192), LDS, {"slices": 2, "per": 4096}),
    ("slices, two uneven", (1, 8, 100, 8193), LDS, {"slices": 2, "per": 4097}),
    ("slices, three", (1, 8, 101, 12289), LDS, {"slices": 3, "per": 4097}),
    ("slices, cap of 64", (1, 1, 7, 262149), LDS, {"slices": 64, "per": 4097, "ch": 1}),
    ("want < maxs", (16, 8, 18432, 36864), LDS, {"ch": 2, "slices": 8, "chunks": 4}),
    ("shorter than one pass", (1, 4096, 8, 16), LDS, {"chunks": 256, "slices": 1}),
    ("second pass of one element", (1, 16, 33, 4097), LDS, {"slices": 1, "per": 4097}),
    ("row loader's second trip", (1, 1, 20000, 65536), LDS, {"ch": 1, "slices": 16}),
    ("one-element table", (2, 32, 1, 2048), LDS, {"ch": 16, "chunks": 2, "slices": 1}),
]
LDS_CASE = {name: shape for name, shape, _, _ in LDS_CASES}
# the plain kernels' own edges: L around a block of 256, c around GG_CCHUNK = 8, three batches
PLAIN_CASES = [(3, c, 50, L) for L in (255, 256, 257) for c in (1, 8, 9)]
# storage offsets: the odd-m case and one aligned case, table / index / weight 1, 2, 3 floats past fresh storage
OFFSET_CASES = ("partial chunk, odd m", "ch 16")
# every class the case table has to reach (the census of tests/test_gather_plan_cpu.py)
REQUIRED_CLASSES = ("loader 16-byte", "loader scalar", "loader count % 4 tail", "loader second trip", "partial chunk",
                    "slices=1", "slices=2", "slices=3", "slices=64", "short last slice", "ch=1", "ch=3", "ch=15", "ch=16",
                    "short pass", "second pass", "pass tail")


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def position_table(b, c, m):
    """table[bi, l, j] = bi c m + l m + j as fp32 (exact below 2^24): a wrong row, chunk or batch offset names itself"""
    assert b * c * m < 2 ** 24
    return np.arange(b * c * m, dtype=F32).reshape(b, c, m)


def indices(rng, m, shape):
    """int32 ids in [0, m) over `shape` (batch first): random with repeats, then per batch a 0, an m - 1 and a run of one
    value across a whole wave of lanes (64 consecutive elements, wherever the row is long enough)"""
    idx = rng.integers(0, m, shape).astype(np.int32)
    flat = idx.reshape(shape[0], -1)
    flat[:, 0] = 0
    flat[:, -1] = m - 1
    n = flat.shape[1]
    if n > 2:
        lo = min(64, n // 2)
        hi = min(lo + 128, n - 1)
        flat[:, lo:hi] = rng.integers(0, m)
        flat[:, 1] = m - 1
        flat[:, n - 2] = 0
    return idx


def weights(rng, shape):
    """interpolation weights: positive, negative, an exact 0 and an exact 1 among them"""
    w = (rng.random(shape) * 2 - 0.5).astype(F32)
    flat = w.reshape(-1)
    flat[::7] = 0.0
    flat[3::11] = 1.0
    return w


# ---- exact ops ---------------------------------------------------------------------------------------------------------

def gather_ref(table, idx):
    """out[b, c, e] = table[b, c, idx[b, e]]; idx (b, ...) is taken flat per batch"""
    b = table.shape[0]
    flat = idx.reshape(b, 1, -1).astype(np.int64)
    return np.take_along_axis(table, np.broadcast_to(flat, (b, table.shape[1], flat.shape[2])), axis=2)


def grouping_cl_ref(inp, idx):
    """out[i, s, :] = inp[idx[i, s], :]"""
    return inp[idx.astype(np.int64)]


def subtraction_cl_ref(in1, in2, idx):
    """out[i, s, :] = fl(in1[i, :] - in2[idx[i, s], :]): one fp32 subtraction"""
    return (in1[: idx.shape[0], None, :] - in2[idx.astype(np.int64)]).astype(F32)


def graph_feature_ref(x_q, x_k, idx):
    """(b, 2c, nq, k): fl(x_k[b, c, idx[b, i, j]] - x_q[b, c, i]) over x_q[b, c, i]"""
    b, c, nq = x_q.shape
    k = idx.shape[2]
    nb = gather_ref(x_k, idx).reshape(b, c, nq, k)
    q = np.broadcast_to(x_q[..., None], (b, c, nq, k))
    return np.concatenate([(nb - q).astype(F32), q], axis=1)


def graph_feature_grad_q_ref(g, old):
    """old + acc with acc += fl(g2[j] - g1[j]) left to right from 0, in fp32; g (b, 2c, nq, k), old (b, c, nq)"""
    c = old.shape[1]
    acc = np.zeros(old.shape, F32)
    for j in range(g.shape[3]):
        acc = (acc + (g[:, c:, :, j] - g[:, :c, :, j]).astype(F32)).astype(F32)
    return (old + acc).astype(F32)


# ---- fp32 restatements with their fp64 values and bounds ------------------------------------------------------------------

def three_interpolate_ref32(table, idx, w):
    """fl(fl(fl(p0 w0) + fl(p1 w1)) + fl(p2 w2)), (b, c, n)"""
    b, c, _ = table.shape
    n = idx.shape[1]
    p = gather_ref(table, idx).reshape(b, c, n, 3)
    t = (p * w[:, None]).astype(F32)
    return ((t[..., 0] + t[..., 1]).astype(F32) + t[..., 2]).astype(F32)


def three_interpolate_ref64(table, idx, w):
    """(fp64 value, bound): gamma(3) sum |p_t w_t| -- a term passes its product and at most two additions"""
    b, c, _ = table.shape
    n = idx.shape[1]
    t = gather_ref(table, idx).reshape(b, c, n, 3).astype(np.float64) * w[:, None].astype(np.float64)
    return t.sum(-1), gamma(3) * np.abs(t).sum(-1)


def interpolation_cl_ref32(inp, idx, w, out0):
    """acc = out0; acc = fl(acc + fl(inp[idx[i, t]] w[i, t])) for t = 0 .. k - 1"""
    acc = out0.astype(F32).copy()
    for t in range(idx.shape[1]):
        acc = (acc + (inp[idx[:, t].astype(np.int64)] * w[:, t, None]).astype(F32)).astype(F32)
    return acc


def interpolation_cl_ref64(inp, idx, w, out0):
    """(fp64 value, bound): gamma(k + 1) (|out0| + sum |terms|)"""
    t = inp[idx.astype(np.int64)].astype(np.float64) * w[..., None].astype(np.float64)      # (n, k, c)
    return out0 + t.sum(1), gamma(idx.shape[1] + 1) * (np.abs(out0.astype(np.float64)) + np.abs(t).sum(1))


def aggregation_cl_ref32(inp, pos, w, idx, out0):
    """acc = out0; acc = fl(acc + fl(fl(inp[idx[i, s], ch] + pos[i, s, ch]) w[i, s, ch % w_c])) for s = 0 .. ns - 1"""
    c, w_c = inp.shape[1], w.shape[2]
    wch = np.arange(c) % w_c
    acc = out0.astype(F32).copy()
    for s in range(idx.shape[1]):
        v = (inp[idx[:, s].astype(np.int64)] + pos[:, s]).astype(F32)
        acc = (acc + (v * w[:, s][:, wch]).astype(F32)).astype(F32)
    return acc


def aggregation_cl_ref64(inp, pos, w, idx, out0):
    """(fp64 value, bound): gamma(ns + 2) (|out0| + sum (|inp| + |pos|) |w|)"""
    c, w_c = inp.shape[1], w.shape[2]
    ww = w[:, :, np.arange(c) % w_c].astype(np.float64)
    a, p = inp[idx.astype(np.int64)].astype(np.float64), pos.astype(np.float64)
    return out0 + ((a + p) * ww).sum(1), gamma(idx.shape[1] + 2) * (np.abs(out0.astype(np.float64)) + ((np.abs(a) + np.abs(p)) * np.abs(ww)).sum(1))


# ---- float atomics: fp64 scatter-add, contributions counted from the indices ----------------------------------------------

def scatter_rows64(rows, terms, n_rows):
    """(sum, bound) of out[rows[e], :] += terms[e, :] in fp64: bound = gamma(count + 1) * sum |terms| with count the number of
    e landing on the row (one rounding for the term's own product, at most count for the additions, in any order)"""
    rows = torch.from_numpy(np.ascontiguousarray(rows.reshape(-1).astype(np.int64)))
    t = torch.from_numpy(np.ascontiguousarray(terms.reshape(rows.numel(), -1).astype(np.float64)))
    out = torch.zeros(n_rows, t.shape[1], dtype=torch.float64).index_add_(0, rows, t)
    mag = torch.zeros(n_rows, t.shape[1], dtype=torch.float64).index_add_(0, rows, t.abs())
    cnt = torch.bincount(rows, minlength=n_rows).double()
    g = (cnt + 1) * 2.0 ** -24
    return out.numpy(), ((g / (1 - g))[:, None] * mag).numpy()


def scatter_cf64(g, idx, w, m):
    """channels-first (the plain geot_*_grad kernels): out[b, c, idx[b, e, t]] += w[b, e, t] g[b, c, e], with the bound as
    above; g (b, c, L), idx (b, L, nt), w (b, L, nt) or None"""
    b, c, L = g.shape
    nt = idx.shape[-1]
    rows = idx.reshape(b, L * nt).astype(np.int64) + (np.arange(b) * m)[:, None]
    terms = np.repeat(g.transpose(0, 2, 1).astype(np.float64), nt, axis=1)                  # (b, L nt, c)
    if w is not None:
        terms = terms * w.reshape(b, L * nt, 1).astype(np.float64)
    out, bound = scatter_rows64(rows, terms, b * m)
    return out.reshape(b, m, c).transpose(0, 2, 1), bound.reshape(b, m, c).transpose(0, 2, 1)


def interpolation_cl_grad_terms(g, idx, w):
    """(rows, terms) of grad_in[idx[i, t], :] += g[i, :] w[i, t]"""
    return idx, g[:, None, :].astype(np.float64) * w[..., None].astype(np.float64)


def aggregation_cl_grad_ref(inp, pos, w, idx, g):
    """grad_position (fp32, one product: exact), and (rows, terms) of grad_input and of grad_weight.  The fp32 sum
    fl(inp + pos) is taken as the kernel forms it (one correctly rounded addition), so that a grad_weight term passes one
    more rounding, its product, like every other term here"""
    n, ns = idx.shape
    c, w_c = inp.shape[1], w.shape[2]
    wch = np.arange(c) % w_c
    ww = w[:, :, wch]                                                               # (n, ns, c)
    g_pos = (g[:, None, :] * ww).astype(F32)
    t_in = g[:, None, :].astype(np.float64) * ww.astype(np.float64)
    v = (inp[idx.astype(np.int64)] + pos).astype(F32).astype(np.float64)
    t_w = g[:, None, :].astype(np.float64) * v                                      # lands on (i, s, ch % w_c)
    rows_w = (np.arange(n * ns)[:, None] * w_c + wch[None, :]).reshape(n, ns, c)
    return g_pos, (idx, t_in), (rows_w, t_w)


# ---- fp_weights ------------------------------------------------------------------------------------------------------------

EPS32 = F32(1e-8)                                 # the kernel's 1e-8f


def fp_weights_ref32(d2):
    """the kernel's expression in numpy fp32: r = 1 / (sqrt(d2) + 1e-8f), w = r / ((r0 + r1) + r2); (rows, 3)"""
    one = F32(1.0)
    r = (one / (np.sqrt(d2.astype(F32)) + EPS32).astype(F32)).astype(F32)
    norm = ((r[:, 0] + r[:, 1]).astype(F32) + r[:, 2]).astype(F32)
    return (r / norm[:, None]).astype(F32)


def fp_weights_ref64(d2):
    """the same expression in fp64 on the same fp32 inputs (the fp32 constant included).  A weight passes at most 9 fp32
    operations -- sqrt, add, reciprocal for its own r; the same three plus two additions for any term of the norm; one
    division -- all on positive numbers, so its relative error is at most gamma(9) where division and sqrt are correctly
    rounded (hipcc's default for fp32)"""
    r = 1.0 / (np.sqrt(d2.astype(np.float64)) + float(EPS32))
    return r / ((r[:, 0] + r[:, 1]) + r[:, 2])[:, None]


FP_WEIGHTS_BOUND = gamma(9)


def fp_weights_rows(rows):
    """squared distances (rows, 3): random magnitudes over many decades, then one, two and three zero distances, a
    subnormal, 1e30 and equal distances planted in the first rows (as many as there are)"""
    rng = rng_of("fp_weights %d" % rows)
    d2 = (10.0 ** rng.uniform(-12, 4, (rows, 3))).astype(F32)
    special = np.array([[0, 0.25, 1], [0, 0, 1], [0, 0, 0], [1e-40, 1e-3, 1], [1e30, 1, 1e30], [0.5, 0.5, 0.5],
                        [1e30, 1e30, 1e30], [1e-40, 1e-40, 0], [0.04, 0.04, 0.09]], dtype=F32)
    k = min(rows, len(special))
    d2[rows - k:] = special[:k]
    return d2
