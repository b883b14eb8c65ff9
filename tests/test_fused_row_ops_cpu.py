"""The host-only sizing exports of the fused row ops, without a GPU: the slice counts and workspaces the wrappers in
geot_amd/fused_norm.py allocate by must stay within what the kernels of csrc/bnrelu.hip and csrc/layernorm.hip assume,
over random and boundary shapes, and invalid sizes must give -1."""
import numpy as np
import pytest

BN_MAX_SLICES = 32          # csrc/bnrelu.hip
ROWDOT_MAX_SLICES = 64      # geot_rowdot_small_slices' cap
COLSUM_MAX_SLICES = 16      # colsum_finish_kernel reads at most 16 partial rows
LN_WIDTHS = (128, 256, 384, 512, 768, 1024)
LN_ROWS_PER_BLOCK = 8       # res_ln_bwd_kernel: 4 waves x LN_ROWS_PER_WAVE = 2 rows


@pytest.fixture(scope="module")
def lib():
    from geot_amd import _lib
    return _lib.load()


def _sizes(rng, hi, count):
    """log-uniform integers in [1, hi], plus 1, 2, 3 and hi"""
    r = np.exp(rng.uniform(0, np.log(hi), count)).astype(np.int64)
    return [1, 2, 3, hi] + [int(v) for v in np.clip(r, 1, hi)]


def _around(points):
    return sorted({p + d for p in points for d in (-1, 0, 1) if p + d >= 1})


def test_rowdot_small_slices_cover_every_element(lib):
    """1 <= S <= 64, and the slices of ceil(l / S) rounded up to 4 elements cover [0, l) with none empty (the kernel's
    empty-slice branch is never taken through this sizing) and none past 65535 rows of grid"""
    rng = np.random.default_rng(1)
    rows = _around([1, 8, 16, 17, 128, 1024, 65535]) + _sizes(rng, 65535, 60)
    ls = _around([4, 2048, 2049, 63 * 2048, 64 * 2048, 1 << 20]) + _sizes(rng, 1 << 26, 60)
    for c in rows:
        for l in ls:
            s = lib.geot_rowdot_small_slices(c, l)
            assert 1 <= s <= ROWDOT_MAX_SLICES, (c, l, s)
            per = ((l + s - 1) // s + 3) & ~3
            assert s * per >= l and (s - 1) * per < l, (c, l, s)
    assert lib.geot_rowdot_small_slices(8, 63 * 2048 + 1) == ROWDOT_MAX_SLICES       # the shape the GPU test takes to the cap
    for c, l in ((0, 5), (5, 0), (-1, 5), (5, -1)):
        assert lib.geot_rowdot_small_slices(c, l) == -1


def test_colsum_workspace_holds_every_slice(lib):
    """workspace = S * cols floats with 1 <= S <= 16: colsum_kernel writes partial[slice * cols + col] for slice < S"""
    rng = np.random.default_rng(2)
    rows = _around([1, 32, 33, 481, 512, 4101, 1 << 20]) + _sizes(rng, 1 << 24, 60)
    cols = _around([1, 64, 65, 1024, 1025, 1536]) + _sizes(rng, 1 << 16, 40)
    for r in rows:
        for c in cols:
            ws = lib.geot_colsum_ws_floats(r, c)
            assert ws % c == 0 and 1 <= ws // c <= COLSUM_MAX_SLICES, (r, c, ws)
            assert ws // c <= -(-r // 32) or ws // c == 1, (r, c, ws)              # slices of >= 32 rows
    assert lib.geot_colsum_ws_floats(4101, 64) == COLSUM_MAX_SLICES * 64
    for r, c in ((0, 5), (5, 0), (-3, 5), (5, -3)):
        assert lib.geot_colsum_ws_floats(r, c) == -1


def test_res_ln_workspace_holds_every_block(lib):
    """workspace >= 2 * ceil(rows / 8) * C floats (res_ln_bwd_kernel writes partial[(blk * 2 + {0,1}) * C + col]); only the
    six widths of the templates are supported"""
    assert [c for c in range(0, 4097) if lib.geot_res_ln_supported(c)] == list(LN_WIDTHS)
    rng = np.random.default_rng(3)
    for c in LN_WIDTHS:
        for rows in _around([1, 7, 8, 9, 1024, 1025]) + _sizes(rng, 1 << 22, 60):
            assert lib.geot_res_ln_ws_floats(rows, c) >= 2 * (-(-rows // LN_ROWS_PER_BLOCK)) * c, (rows, c)
    for rows, c in ((0, 384), (-1, 384), (5, 0), (5, 383), (5, 64), (5, 2048)):
        assert lib.geot_res_ln_ws_floats(rows, c) == -1


def test_bn_slices_within_the_statistics_buffer(lib):
    """1 <= S <= BN_MAX_SLICES = 32 statistics slices, each at least 4096 elements when there is more than one (so none is
    empty: ceil(l / S) rounded up to 4 times S - 1 stays below l); b or c past 65535 (grid y / z) or < 1 give -1"""
    rng = np.random.default_rng(4)
    bs = _around([1, 2, 8, 65535]) + _sizes(rng, 65535, 12)
    cs = _around([1, 2, 32, 1024, 65535]) + _sizes(rng, 65535, 12)
    ls = _around([1, 4096, 8192, 131072, 262144]) + _sizes(rng, 1 << 24, 20)
    for b in bs:
        for c in cs:
            if b > 65535 or c > 65535:
                assert lib.geot_bn_slices(b, c, 4096) == -1
                continue
            for l in ls:
                s = lib.geot_bn_slices(b, c, l)
                assert 1 <= s <= BN_MAX_SLICES, (b, c, l, s)
                assert s == 1 or l // s >= 4096, (b, c, l, s)
                per = ((l + s - 1) // s + 3) & ~3
                assert (s - 1) * per < l, (b, c, l, s)
    assert lib.geot_bn_slices(1, 2, 262147) == BN_MAX_SLICES                      # the shape the GPU test takes to the cap
    for b, c, l in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (65536, 1, 1), (1, 65536, 1)):
        assert lib.geot_bn_slices(b, c, l) == -1


def test_model_shapes_stay_on_the_tested_branches(lib):
    """TOOTH_SEG_CFG's shapes against the switches the GPU tests cover: groups of 32 points (8 lanes per row of the
    segment kernels, an n of tests/test_fused_row_ops_gpu.py), width 384 (a res_ln template), 4 heads of d = 96 (a
    multiple of 4: the head-split kernel), 512 tokens (a soft-max gradient width)"""
    from geot_amd.openpoints.models.backbone.transformer import TOOTH_SEG_CFG as cfg
    n, c, heads, g = cfg["group_size"], cfg["trans_dim"], cfg["num_heads"], cfg["num_group"]
    assert n % 4 == 0 and 32 <= n <= 256
    assert lib.geot_res_ln_supported(c)
    assert c % heads == 0 and (c // heads) % 4 == 0
    assert g in (64, 128, 256, 512, 1024)
