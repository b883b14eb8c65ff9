"""GPU suite of geot_pseudo_refine (csrc/pseudo_refine.hip): the kernel against the numpy float32 restatement of its
contract (tests/_pseudo_refine_ref.py) on the same neighbour ids -- keep exact, value bit for bit -- at the tail wave, the
widest and narrowest class loops, k = n and a batch offset above 0, in both forms of sharing the classes out
(GEOT_PSEUDO_REFINE_IMPL=point|split); against the reference-executed fixture through both bindings; pseudo_refine_mask
against the composite pseudo_label_refine / _margin / _margin_v1 it replaces; the refusals; an id outside [0, N)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _pseudo_refine_ref as pref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FIXTURE = os.path.join(HERE, "golden", "pseudo_label_refine_ref.npz")
MODE_ID = {"max": 0, "margin": 1, "margin_v1": 2}
# both computed as the reference does, torch.exp(torch.tensor(-1/2)) in fp32, and as the composite does, float(np.exp(-0.5))
# rounded to fp32 by the multiply: the same bits, 0x3f1b4598, so the composite's margins are expected bit for bit
BETA = float(torch.exp(torch.tensor(-1 / 2)))


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def kernel(prob, nbr, k, mode, th, beta=BETA, e=None, want_value=True):
    """geot_pseudo_refine on numpy inputs -> (keep, value) as numpy."""
    from geot_amd.ext._common import call, ptr
    b, c, npts = prob.shape
    p, ids = T(prob), T(nbr, torch.int32)
    ej = T(np.asarray(e, np.float64)[:c].astype(np.float32)) if e is not None else None
    keep = torch.full((b, npts), 7, dtype=torch.uint8, device=DEV)
    value = torch.full((b, npts), -5.0, device=DEV) if want_value else None
    call("geot_pseudo_refine", DEV, b, c, npts, nbr.shape[2], k, MODE_ID[mode], float(th), float(beta), ptr(p), ptr(ids),
         ptr(ej), ptr(keep), ptr(value))
    torch.cuda.synchronize()
    return keep.cpu().numpy(), (value.cpu().numpy() if want_value else None)


def draw(b, c, npts, n, seed, scale=3.0):
    rng = np.random.default_rng(seed)
    z = torch.from_numpy((rng.normal(size=(b, c, npts)) * scale).astype(np.float32))
    prob = torch.softmax(z, dim=1).numpy() if c > 1 else rng.uniform(0.05, 0.95, size=(b, c, npts)).astype(np.float32)
    nbr = rng.integers(0, npts, size=(b, npts, n)).astype(np.int32)      # repeated ids: equal values among the n
    e = rng.uniform(0.95, 0.98, size=c)
    return prob, nbr, e


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("form", ["point", "split"])
@pytest.mark.parametrize("n,k", [(1, 1), (4, 1), (4, 4), (16, 3), (32, 32)])
@pytest.mark.parametrize("mode", pref.MODES)
def test_kernel_equals_the_restatement(mode, n, k, form, monkeypatch):
    monkeypatch.setenv("GEOT_PSEUDO_REFINE_IMPL", form)        # read by the library at every call
    # margin_v1 applied more than once runs away to -inf - -inf where a point and its neighbours disagree strongly; a NaN's
    # payload is not part of the contract, so those cases take near-uniform probabilities, on which every value is finite
    scale = 0.3 if mode == "margin_v1" and k > 1 else 3.0
    seen = 0
    for npts in (63, 64, 65, 257):
        for c in (1, 2, 5, 17, 32):
            if c == 1 and mode != "max":
                continue
            for b in (1, 3):
                prob, nbr, e = draw(b, c, npts, n, seed=1000 * npts + 10 * c + b, scale=scale)
                _, v0 = pref.refine(prob, nbr, k, mode, 0.0, np.float32(BETA), e)
                th = float(np.median(v0))                    # both mask values occur
                want_keep, want_value = pref.refine(prob, nbr, k, mode, th, np.float32(BETA), e)
                assert set(np.unique(want_keep)) == {0, 1}, (npts, c, b)
                keep, value = kernel(prob, nbr, k, mode, th, e=e)
                what = (mode, n, k, form, npts, c, b)
                assert np.isfinite(want_value).all(), what
                assert same_bits(value, want_value), (what, int((value != want_value).sum()))
                assert np.array_equal(keep, want_keep), (what, int((keep != want_keep).sum()))
                seen += 1
    assert seen == (40 if mode == "max" else 32)


def test_value_is_optional_and_two_calls_give_the_same_bits():
    prob, nbr, e = draw(3, 17, 257, 4, seed=5)
    a = kernel(prob, nbr, 2, "margin", 0.3)
    b = kernel(prob, nbr, 2, "margin", 0.3)
    only_keep, none = kernel(prob, nbr, 2, "margin", 0.3, want_value=False)
    assert none is None and np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]) and np.array_equal(only_keep, a[0])


def test_kernel_equals_the_reference_fixture_through_both_bindings():
    from geot_amd.ext import _common
    from geot_amd.utils.pseudo_mask import E_JOINT
    z = np.load(FIXTURE)
    assert int(z["beta_bits"]) == int(np.float32(BETA).view(np.uint32)) == 0x3f1b4598
    assert _common.dispatcher() is not None and hasattr(_common.dispatcher(), "geot_pseudo_refine")
    saved = _common._dispatch
    try:
        for name, disp in (("dispatcher", saved), ("ctypes", False)):
            _common._dispatch = disp
            for case, th in zip([str(c) for c in z["cases"]], z["th"]):
                mode, n, k = re.match(r"(\w+)_n(\d+)_k(\d+)", case).groups()
                keep, value = kernel(z["prob"], z["nbr_n" + n].astype(np.int32), int(k), mode, th, e=E_JOINT)
                assert np.array_equal(keep, z["mask_" + case]), (name, case, int((keep != z["mask_" + case]).sum()))
                if mode != "max":
                    assert same_bits(value, z["margin_" + case]), (name, case)
    finally:
        _common._dispatch = saved


@pytest.fixture(scope="module")
def cloud():
    """Two clouds of 2 000 points, confident regions with noisy borders: (pred_t (B, C, N), pos (B, N, 3)) on the device."""
    rng = np.random.default_rng(11)
    pos = (rng.normal(size=(2, 2000, 3)) * np.array([1.0, 0.7, 0.4])).astype(np.float32)
    centres = pos[:, :6]
    d = np.sqrt(((pos[:, :, None, :] - centres[:, None, :, :]) ** 2).sum(-1))
    near = np.sort(d, axis=2)
    scale = 1.0 + 14.0 * np.clip((near[..., 1] - near[..., 0]) / 0.5, 0.0, 1.0)
    z = rng.normal(size=(2, 2000, 17)) * 1.5
    np.put_along_axis(z, d.argmin(2)[..., None], np.take_along_axis(z, d.argmin(2)[..., None], 2) + scale[..., None], 2)
    pred = torch.softmax(T(z.transpose(0, 2, 1).astype(np.float32)), dim=1).contiguous()
    return pred, T(pos)


@pytest.mark.parametrize("size,k", [(4, 1), (6, 3)])
def test_fused_entry_point_equals_the_composite(size, k, cloud):
    from geot_amd.utils import pseudo_mask as pm
    pred, pos = cloud
    nbr = pm.neighbours(pos, size)
    idx, _ = pm.pointops.knn(pos, pos, size + 1)
    assert nbr.dtype == torch.int32 and tuple(nbr.shape) == (2, 2000, size) and torch.equal(nbr.long(), idx[:, :, 1:])
    assert not (nbr == torch.arange(2000, device=DEV)[None, :, None]).any()            # slot 0, the point itself, is gone
    keep = pm.pseudo_refine_mask(pred, 0.9, pos, size, k)
    want = pm.pseudo_label_refine(pred, 0.9, pos, size, k)
    assert keep.dtype == torch.uint8 and torch.equal(keep.bool(), want)
    assert 0 < int(want.sum()) < want.numel() and not torch.equal(want, pred.max(1)[0].ge(0.9))
    assert torch.equal(pm.pseudo_refine_mask(pred, 0.9, None, size, k, nbr=nbr), keep)     # neighbours handed over
    keep, value = pm.pseudo_refine_mask(pred, 0.5, pos, size, k, mode="margin", return_value=True)
    want, margin = pm.pseudo_label_refine_margin(pred, 0.5, pos, size, k)
    print("margin: %d of %d kept, %d margins differ" % (int(want.sum()), want.numel(), int((value != margin).sum())))
    assert torch.equal(keep.bool(), want) and torch.equal(value.view(torch.int32), margin.view(torch.int32))
    assert 0 < int(want.sum()) < want.numel()
    keep, value = pm.pseudo_refine_mask(pred, 0.5, pos, size, k, mode="margin_v1", return_value=True)
    want, margin, _ = pm.pseudo_label_refine_margin_v1(pred, 0.5, 0, pos, size, k)
    print("margin_v1: %d of %d kept, %d margins differ" % (int(want.sum()), want.numel(), int((value != margin).sum())))
    assert torch.equal(keep.bool(), want) and torch.equal(value.view(torch.int32), margin.view(torch.int32))


def test_invalid_arguments_are_refused_before_the_launch():
    prob, nbr, e = draw(2, 17, 64, 4, seed=3)
    with pytest.raises(RuntimeError, match="invalid"):          # k > n
        kernel(prob, nbr, 5, "max", 0.5)
    with pytest.raises(RuntimeError, match="invalid"):          # n > 32
        kernel(prob, np.zeros((2, 64, 33), np.int32), 1, "max", 0.5)
    with pytest.raises(RuntimeError, match="invalid"):          # N < n + 1
        kernel(prob[:, :, :4], nbr[:, :4], 1, "max", 0.5)
    with pytest.raises(RuntimeError, match="invalid"):          # one class has no margin
        kernel(prob[:, :1], nbr, 1, "margin", 0.5)
    with pytest.raises(RuntimeError, match="invalid"):          # margin_v1 without E_joint
        kernel(prob, nbr, 1, "margin_v1", 0.5)
    from geot_amd.ext._common import call, ptr
    p, ids = T(prob), T(nbr)
    with pytest.raises(RuntimeError, match="invalid"):          # a NULL output
        call("geot_pseudo_refine", DEV, 2, 17, 64, 4, 1, 0, 0.5, BETA, ptr(p), ptr(ids), None, None, None)
    torch.cuda.synchronize()


@pytest.mark.parametrize("form", ["point", "split"])
def test_an_id_outside_the_cloud_drops_its_point_only(form, monkeypatch):
    """The header: such an id is never followed, the point's keep is 0 and its value NaN.  The table is built by hand and
    every buffer is of the size the call states: nothing is read out of bounds."""
    monkeypatch.setenv("GEOT_PSEUDO_REFINE_IMPL", form)
    prob, nbr, e = draw(2, 17, 65, 4, seed=9)
    clean_keep, clean_value = kernel(prob, nbr, 2, "max", 0.0)
    assert clean_keep.all()
    nbr[0, 3, 2], nbr[0, 10, 0], nbr[1, 64, 3], nbr[1, 0, 1] = 65, -1, 2 ** 31 - 1, -2 ** 31
    keep, value = kernel(prob, nbr, 2, "max", 0.0)
    bad = np.zeros((2, 65), bool)
    bad[0, 3] = bad[0, 10] = bad[1, 64] = bad[1, 0] = True
    assert (keep[bad] == 0).all() and np.isnan(value[bad]).all()
    assert (keep[~bad] == 1).all() and same_bits(value[~bad], clean_value[~bad])
    want_keep, want_value = pref.refine(prob, nbr, 2, "max", 0.0, np.float32(BETA))
    assert np.array_equal(keep, want_keep) and np.array_equal(np.isnan(value), np.isnan(want_value))
