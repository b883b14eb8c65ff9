"""Shared by the scatter-gradient tests: the host-only plan query of the *_grad_ws / _grad_out / _grad_from entry points
(geot_scatter_grad_plan), a bisection for the shapes where its answer switches, and the fp64 restatement of the
scatter-add the GPU tests compare against."""
import ctypes

import torch

NONE, TILES, CSR, CL = 0, 1, 2, 3                 # forms, as geot_scatter_grad_plan returns them
FORM_NAMES = {NONE: "none", TILES: "tiles", CSR: "csr", CL: "channels-last"}
PLAN_FIELDS = ("ch", "tl", "q", "ppp", "cap", "lds", "lds_build", "ints")


def plan(lib, b, c, m, L, nt, weighted=None):
    """(form, {field: value} for the tile form else None) of one call shape"""
    weighted = (nt == 3) if weighted is None else weighted
    out = (ctypes.c_longlong * len(PLAN_FIELDS))()
    form = lib.geot_scatter_grad_plan(int(b), int(c), int(m), int(L), int(nt), int(bool(weighted)), out, len(PLAN_FIELDS))
    return form, (dict(zip(PLAN_FIELDS, out)) if form == TILES else None)


TLDS_FLOATS = 36864                               # the list walk holds whole rows of at most this many sources in LDS
SCAN_CHUNK = 4096


def whole_rows(c, m, L, nt):
    """the shape half of the list walk's preference: whole rows in one part (fewer than 4 channels, or 4 rows fit the
    LDS) and lists of 12 pairs or more on average"""
    return 1 <= L <= TLDS_FLOATS and m >= 1 and nt >= 1 and (c < 4 or TLDS_FLOATS // L >= 4) and L * nt >= 12 * m


def ws_floats_ref(b, c, m, L, nt, tile_ints):
    """geot_scatter_grad_ws_floats restated: the largest of the channels-last accumulator, the tile plan's workspace
    (tile_ints: its `ints`, 0 without a tile plan) and, where whole_rows holds, the one-part reverse index (offsets,
    scan scratch, and rank / source / weight / pair id per pair)"""
    if b < 1 or c < 1 or m < 1:
        return 0
    t, pairs = b * m, b * L * nt
    rows = (t + 1) + (t + 1 + SCAN_CHUNK - 1) // SCAN_CHUNK + 4 * pairs + 8 if whole_rows(c, m, L, nt) else 0
    return max(b * m * c, tile_ints, rows)


def switch(pred, lo, hi):
    """x in [lo, hi) with pred(x) != pred(x + 1), by bisection; pred(lo) and pred(hi) must differ"""
    a, z = pred(lo), pred(hi)
    assert a != z, (lo, hi, a)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid) == a:
            lo = mid
        else:
            hi = mid
    return lo


def rel(got, want64):
    """largest error relative to the scale of the element's row (the tolerance rule of tests/test_ref_fixtures_gpu.py)"""
    got, want64 = got.double().cpu(), want64.double().cpu()
    scale = want64.abs().amax(dim=-1, keepdim=True).clamp_min(1e-30)
    return float(((got - want64).abs() / scale).max())


def scatter64(g, idx, w, m):
    """fp64 restatement: out[b, c, idx[b, e, t]] += w[b, e, t] * g[b, c, e]"""
    b, c, L = g.shape
    nt = idx.shape[-1]
    src = g.double().cpu().unsqueeze(-1) * (w.double().cpu().unsqueeze(1) if w is not None else 1.0)
    out = torch.zeros(b, c, m, dtype=torch.float64)
    out.scatter_add_(2, idx.long().cpu().reshape(b, 1, L * nt).expand(-1, c, -1), src.reshape(b, c, L * nt).expand(b, c, L * nt))
    return out
