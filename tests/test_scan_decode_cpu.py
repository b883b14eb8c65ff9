"""Decoding whole scans without a GPU: the numpy restatement (tests/_scan_decode_ref.py) against a brute-force fp64 search on
inputs without near-ties, the ABI version and both signatures, every refusal of geot_scan_decode_front /
geot_scan_decode_finish through the host-only path (a refusal comes before any launch, so it needs no device), the chunked
work table, and the label cap: on the model-level fixtures the fp64 reference alone leaves at most 2 % of the vertices within
twice its bound of a tie."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scan_decode_ref as dref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from geot_amd import _lib, build
    build.build()
    return _lib.load()


def test_abi_version_and_signatures(lib):
    from geot_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    assert int(re.search(r"GEOT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 31
    assert lib.geot_abi_version() == _lib.ABI_VERSION
    for name, params in (("geot_scan_decode_front", 27), ("geot_scan_decode_finish", 15)):
        proto = re.search(r"int %s\((.*?)\);" % name, hdr, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.PROTOTYPES[name]) == params, name
        assert getattr(lib, name).restype is ctypes.c_int
    # the records are geot_scan_predict's: (slot, first vertex, vertex count, fourth word), four int32, 16-byte aligned
    assert "first output row" in hdr and "accuracy of decoded against interpolated or covered labels on real scans has" in hdr


def _front_args(**over):
    one = 4096                          # any non-NULL, 16-byte aligned address: a refusal never reads it
    args = dict(b=1, m=3, c_out=4, relu=1, n_scans=1, total=8, points=one, offsets=one, scan_ids=one, center=one, scale=one,
                view_center=one, view_scale=one, known=one, a=one, skip_const=one, w_xyz=one, ch_scale=one, ch_shift=one, n_work=1,
                work=one, rows=8, z=one, q=None, idx=None, weight=None, stream=None)
    args.update(over)
    return list(args.values())


def _finish_args(**over):
    one = 4096
    args = dict(b=1, c=17, n_scans=1, total=8, labels=one, offsets=one, scan_ids=one, n_work=1, work=one, rows=8, logits=one,
                out_offsets=one, pred=one, counts=one, stream=None)
    args.update(over)
    return list(args.values())


FRONT_REFUSALS = [dict(b=-1), dict(b=65536), dict(m=2), dict(m=0), dict(c_out=0), dict(relu=2), dict(relu=-1), dict(n_scans=0),
                  dict(total=0), dict(n_work=-1), dict(rows=-1), dict(rows=1 << 31), dict(work=None), dict(work=4100)] + \
                 [{k: None} for k in ("points", "offsets", "scan_ids", "center", "scale", "view_center", "view_scale", "known", "a",
                                      "skip_const", "w_xyz", "ch_scale", "ch_shift", "z")]
FINISH_REFUSALS = [dict(b=-1), dict(b=65536), dict(c=0), dict(c=33), dict(n_scans=0), dict(total=0), dict(n_work=-1), dict(rows=-1),
                   dict(rows=1 << 31), dict(work=None), dict(work=4100), dict(offsets=None), dict(scan_ids=None), dict(logits=None),
                   dict(pred=None, counts=None), dict(labels=None), dict(out_offsets=None)]


@pytest.mark.parametrize("over", FRONT_REFUSALS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_front_refusals_come_before_any_launch(lib, over):
    assert lib.geot_scan_decode_front(*_front_args(**over)) == 1            # hipErrorInvalidValue


@pytest.mark.parametrize("over", FINISH_REFUSALS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_finish_refusals_come_before_any_launch(lib, over):
    assert lib.geot_scan_decode_finish(*_finish_args(**over)) == 1


def test_nothing_to_do_is_success(lib):
    for over in (dict(b=0), dict(n_work=0, work=None), dict(rows=0)):
        assert lib.geot_scan_decode_front(*_front_args(**over)) == 0, over
        assert lib.geot_scan_decode_finish(*_finish_args(**over)) == 0, over


def test_reference_search_equals_brute_force_fp64():
    """On well-separated inputs (no two candidates of a vertex closer in distance than fp32 can tell apart) the float32
    (d2, index) choice is the float64 one; the weights sum to one."""
    rng = np.random.default_rng(5)
    for v, m in ((1, 3), (65, 5), (200, 64), (300, 65), (257, 300)):
        known = rng.normal(size=(m, 3)).astype(np.float32)
        q = rng.normal(size=(v, 3)).astype(np.float32)
        d2, idx = dref.three_nn(q, known)
        idx64, d64 = dref.three_nn_fp64(q, known)
        gaps = np.diff(d64, axis=1) / np.maximum(d64[:, 1:], 1e-30)
        clear = (gaps > 64 * dref.U).all(1)                  # separated by far more than the rounding of d2 (3 roundings + inputs)
        assert clear.mean() > 0.9 and np.array_equal(idx[clear], idx64[clear])
        assert np.allclose(d2[clear], d64[clear][:, :3], rtol=8 * dref.U)
        w = dref.fp_weights(d2)
        assert np.allclose(w.sum(1), 1.0, atol=4 * dref.U) and (w[:, 0] >= w[:, 1]).all() and (w[:, 1] >= w[:, 2]).all()


def test_reference_tie_and_nan_rules():
    known = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0], [5, 5, 5]], np.float32)        # duplicates: 0, 2, 3
    q = np.array([[0, 0, 0], [np.nan, 0, 0]], np.float32)
    d2, idx = dref.three_nn(q, known)
    assert idx[0].tolist() == [0, 2, 3] and d2[0].tolist() == [0, 0, 0]
    assert idx[1].tolist() == [0, 0, 0] and np.isinf(d2[1]).all()
    assert np.isnan(dref.fp_weights(d2)[1]).all()           # 0 / 0
    assert dref.argmax_rule(np.array([[1.0, 3.0, 3.0], [1.0, np.nan, 9.0]])).tolist() == [1, 1]


def test_front_row_bound_covers_a_float32_evaluation():
    """The kernel's statements in numpy float32 lie inside the fp64 row's bound, and the bound is not vacuous."""
    rng = np.random.default_rng(6)
    v, m, c = 120, 40, 37
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    q, a, skip, wx, sc, sh = f(v, 3), f(m, c), f(c), f(c, 3), f(c), f(c)
    d2, idx = dref.three_nn(q, f(m, 3))
    w = dref.fp_weights(d2)
    z, bound = dref.front_rows(q, idx, w, a, skip, wx, sc, sh, relu=True)
    t = (w[:, 0, None] * a[idx[:, 0]]).astype(np.float32)
    t = (t + (w[:, 1, None] * a[idx[:, 1]]).astype(np.float32)).astype(np.float32)
    t = (t + (w[:, 2, None] * a[idx[:, 2]]).astype(np.float32)).astype(np.float32)
    t = (t + skip[None]).astype(np.float32)
    x = (wx[None, :, 0] * q[:, 0, None]).astype(np.float32)
    x = (x + (wx[None, :, 1] * q[:, 1, None]).astype(np.float32)).astype(np.float32)
    x = (x + (wx[None, :, 2] * q[:, 2, None]).astype(np.float32)).astype(np.float32)
    z32 = np.maximum(((sc[None] * (t + x).astype(np.float32)).astype(np.float32) + sh[None]).astype(np.float32), 0)
    assert (np.abs(z32 - z) <= bound).all()
    assert np.median(bound) < 1e-5 and (np.abs(z32 - z) > 0).any()


def test_decode_work_table_covers_every_vertex_once():
    from geot_amd.validation import decode_work_table
    for sizes, chunk in (([1, 63, 64, 65, 1000], 300), ([150, 97], 100), ([150, 97], 32768), ([5], 1), ([700], 256)):
        table, chunks = decode_work_table(sizes, chunk)
        assert table.dtype == np.int32 and table.shape[1] == 4
        seen = [np.zeros(m, int) for m in sizes]
        at = 0
        for k, (first, count, rows) in enumerate(chunks):
            assert first == at and count >= 1 and (rows == chunk or k == len(chunks) - 1)
            taken = np.zeros(rows, int)
            for slot, v0, cnt, r0 in table[first:first + count]:
                assert 1 <= cnt <= 256 and r0 >= 0 and r0 + cnt <= rows
                seen[slot][v0:v0 + cnt] += 1
                taken[r0:r0 + cnt] += 1
            assert (taken == 1).all()
            at += count
        assert at == len(table) and all((s == 1).all() for s in seen)
        assert sum(r for _, _, r in chunks) == sum(sizes)
    with pytest.raises(RuntimeError):
        decode_work_table([10], 0)


def test_label_cap_holds_for_the_fixtures_on_the_reference_alone():
    """The model-level label comparisons (tests/test_scan_decode_model_gpu.py) leave out vertices whose fp64 top-1 / top-2
    margin is within twice the bound; that share may be at most 2 %.  Here, without a device: the same seeded model's last stage
    on the same seeded scans, with seeded features in place of the backbone's (the backbone itself needs the GPU)."""
    model = dref.tiny_model()
    p = dref.stage_params(model)
    rng = np.random.default_rng(31)
    c, m = dref.TINY["trans_dim"], dref.TINY["downsample_targets"][0]
    excluded = total = 0
    for jaw, (pts, _) in enumerate(dref.tiny_scans()):
        center, scale = pts.mean(0).astype(np.float32), np.float32(np.abs(pts - pts.mean(0)).max())
        q = dref.query_positions(pts, center, scale, np.zeros(3, np.float32), np.float32(1.0))
        known = q[rng.choice(len(q), m, replace=False)]
        f_l1 = rng.normal(size=(c, m)).astype(np.float32)
        d2, idx = dref.three_nn(q, known)
        logits, bound = dref.last_stage(p, f_l1, known, jaw, q, idx, dref.fp_weights(d2))
        # the probabilistic bound is about 1e-3 on logits of about 5: far from vacuous
        assert np.isfinite(logits).all() and (bound > 0).all() and bound.max() < 1e-3 * np.abs(logits).max()
        excluded += int(dref.near_ties(logits, bound).sum())
        total += len(q)
    assert total == sum(dref.SCAN_SIZES) and excluded / total <= dref.LABEL_CAP


def test_fit_refuses_an_unknown_val_whole_before_anything_else():
    from geot_amd.fit import VAL_WHOLE, _val_whole
    assert VAL_WHOLE == ("interp", "covered", "decoded")
    assert _val_whole({}, 0, False, 0) == "interp" and _val_whole({"val_whole": "decoded"}, 0, False, 0) == "decoded"
    assert _val_whole({"val_whole": "covered"}, 0, True, 2) == "covered"
    for cfg, votes, graph, ahead in (({"val_whole": "direct"}, 0, False, 0), ({"val_whole": "decoded"}, 3, False, 0),
                                     ({"val_whole": "covered"}, 3, False, 0), ({"val_whole": "decoded"}, 0, True, 0),
                                     ({"val_whole": "decoded"}, 0, False, 2)):
        with pytest.raises(ValueError, match="val_whole"):
            _val_whole(cfg, votes, graph, ahead)
