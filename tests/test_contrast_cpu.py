"""The teacher-student contrastive loss, the part that needs no GPU: the ABI and the binding of the geot_contrast_* entry
points, their refusals before any launch, the cfg keys, and the fp64 restatement the GPU tests compare against
(tests/_contrast_ref.py) against the reference-executed fixture (tests/golden/contrast_loss_ref.npz): on every one of the
six calls the reference's own fp32 loss, gradient and bank lie within the derived bounds -- the condition that the bounds
are ones a correct fp32 implementation meets -- and the pointer sequence is the fixture's."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _contrast_ref as cref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "contrast_loss_ref.npz")

SIGNATURES = {
    "geot_contrast_select": ["int b", "int p", "int s", "float th", "const float *score", "const long long *perm",
                             "const long long *perm_q", "unsigned long long seed", "unsigned long long *counter", "int *ws",
                             "int *anchors", "int *count", "int *enqueue_rows", "int *inv", "void *stream"],
    "geot_contrast_loss": ["int b", "int p", "int d", "int s", "int channels_first", "const float *feat_s",
                           "const float *feat_t", "const int *anchors", "const int *count", "const float *bank", "float tau",
                           "float tau_b", "float *xhat", "float *that", "float *norm", "float *ws", "float *ell",
                           "float *grad_dir", "float *loss", "void *stream"],
    "geot_contrast_loss_grad": ["int b", "int p", "int d", "int s", "int channels_first", "const int *count", "const int *inv",
                                "const float *xhat", "const float *norm", "const float *grad_dir", "const float *upstream",
                                "float tau_b", "float *rows", "float *grad", "void *stream"],
    "geot_contrast_enqueue": ["int b", "int d", "int s", "const int *count", "const int *enqueue_rows", "const float *that",
                              "float *bank", "long long *ptr", "void *stream"],
}


def test_abi_version_and_signatures():
    from geot_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    assert int(re.search(r"GEOT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 24
    lib = _lib.load()
    assert lib.geot_abi_version() == _lib.ABI_VERSION
    for name, want_args in SIGNATURES.items():
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
        assert [" ".join(a.split()) for a in decl.split(",")] == want_args, name
        proto = _lib.PROTOTYPES[name]
        assert len(proto) == len(want_args)
        for a, t in zip(want_args, proto):
            want = (ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float")
                    else ctypes.c_ulonglong if a.startswith("unsigned long long") else ctypes.c_int)
            assert t is want, (name, a, t)
        assert getattr(lib, name).argtypes == proto
    for key, value in (("B", 64), ("D", 256), ("S", 1024)):
        assert _lib.CONSTANTS["GEOT_CONTRAST_MAX_" + key] == value
    assert lib.geot_contrast_select_ws_ints(2, 96) == 2 * 96 + 2 + 2
    assert lib.geot_contrast_ws_floats(2, 1024, 128) == (2 + 4) * 2048 * 130      # chunks of 1024 keys: 2 of anchors, 4 of bank
    assert lib.geot_contrast_ws_floats(2, 16, 37) == 2 * 32 * 39
    assert "contrast.hip" in build.SOURCES


def test_entry_point_refusals_need_no_device():
    from geot_amd import _lib
    lib = _lib.load()
    fake = 1 << 20          # hipErrorInvalidValue (1) before any launch: the pointers are never followed
    good = dict(b=2, p=96, s=16, th=0.9, score=fake, perm=None, perm_q=None, seed=1, counter=fake, ws=fake, anchors=fake,
                count=fake, rows=fake, inv=fake)
    for change in (dict(b=0), dict(b=65), dict(p=0), dict(s=0), dict(s=1025), dict(b=64, p=1 << 26), dict(score=None),
                   dict(counter=None), dict(perm=fake), dict(perm_q=fake), dict(ws=None), dict(anchors=None), dict(count=None),
                   dict(rows=None), dict(inv=None)):
        assert lib.geot_contrast_select(*dict(good, **change).values(), None) == 1, change
    good = dict(b=2, p=96, d=128, s=16, cf=0, fs=fake, ft=fake, anchors=fake, count=fake, bank=fake, tau=0.1, tau_b=1.0,
                xhat=fake, that=fake, norm=fake, ws=fake, ell=fake, gdir=fake, loss=fake)
    for change in (dict(d=0), dict(d=257), dict(s=1025), dict(b=65), dict(p=0), dict(tau=0.0), dict(tau_b=-1.0),
                   dict(tau=float("nan")), dict(fs=None), dict(ft=None), dict(bank=None), dict(ws=None), dict(loss=None),
                   dict(gdir=None), dict(anchors=None), dict(count=None)):
        assert lib.geot_contrast_loss(*dict(good, **change).values(), None) == 1, change
    good = dict(b=2, p=96, d=128, s=16, cf=1, count=fake, inv=fake, xhat=fake, norm=fake, gdir=fake, up=fake, tau_b=1.0,
                rows=fake, grad=fake)
    for change in (dict(d=257), dict(b=0), dict(tau_b=0.0), dict(up=None), dict(grad=None), dict(rows=None), dict(inv=None)):
        assert lib.geot_contrast_loss_grad(*dict(good, **change).values(), None) == 1, change
    good = dict(b=2, d=128, s=16, count=fake, rows=fake, that=fake, bank=fake, ptr=fake)
    for change in (dict(d=0), dict(s=0), dict(b=65), dict(count=None), dict(rows=None), dict(that=None), dict(bank=None),
                   dict(ptr=None)):
        assert lib.geot_contrast_enqueue(*dict(good, **change).values(), None) == 1, change


def test_check_cfg_accepts_and_rejects():
    from geot_amd import train_step as ts
    assert ts.NTM_CFG["use_contrastive"] is False and ts.NTM_CFG["contrastive_loss_weight"] == 1.0
    assert ts.NTM_CFG["cur_threshold"] == 0.9 and ts.NTM_CFG["contrast_samples"] == 1024 and ts.NTM_CFG["contrast_seed"] == 0
    ts.check_cfg(dict(ts.NTM_CFG))
    ts.check_cfg(dict(ts.NTM_CFG, use_contrastive=True, contrastive_loss_weight=0.5, cur_threshold=1.0, contrast_samples=1))
    for bad in (None, 1, 0, "True"):
        with pytest.raises(TypeError, match="use_contrastive"):
            ts.check_cfg(dict(ts.NTM_CFG, use_contrastive=bad))
    for bad in (0, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="contrastive_loss_weight"):
            ts.check_cfg(dict(ts.NTM_CFG, use_contrastive=True, contrastive_loss_weight=bad))
    for bad in (0.0, -0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError, match="cur_threshold"):
            ts.check_cfg(dict(ts.NTM_CFG, use_contrastive=True, cur_threshold=bad))
    for bad in (0, 1025, -1):
        with pytest.raises(ValueError, match="contrast_samples"):
            ts.check_cfg(dict(ts.NTM_CFG, use_contrastive=True, contrast_samples=bad))
    for key in ("contrast_samples", "contrast_seed"):
        for bad in (16.0, "16", True, None):
            with pytest.raises(TypeError, match=key):
                ts.check_cfg(dict(ts.NTM_CFG, use_contrastive=True, **{key: bad}))
    for key in ("contrastive_loss_weight", "cur_threshold"):
        for bad in ("1", None, True):
            with pytest.raises(TypeError, match=key):
                ts.check_cfg(dict(ts.NTM_CFG, use_contrastive=True, **{key: bad}))


def test_python_refusals_come_before_any_device_call():
    import torch
    from geot_amd.utils.cluster_contrastloss import nativeContrastLoss_t
    from geot_amd.openpoints.dataset.sample_draw import DeviceDraws
    for kw in (dict(sample_nums=0), dict(sample_nums=1025), dict(dim=0), dict(dim=257), dict(th=0.0), dict(th=1.5)):
        with pytest.raises(ValueError):
            nativeContrastLoss_t(**kw)
    for kw in (dict(sample_nums=16.0), dict(dim="128"), dict(draws=7)):
        with pytest.raises(TypeError):
            nativeContrastLoss_t(**kw)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        nativeContrastLoss_t(sample_nums=4, dim=8, device="cpu", draws=DeviceDraws(1))


@pytest.fixture(scope="module")
def replay():
    """The restatement run over the fixture's six calls with the recorded permutations: [(fixture call, helper call)].
    Every call starts from the bank the reference held (its fp32 rows); the pointer is the helper's own throughout."""
    z = np.load(FIXTURE)
    f = cref.FIXTURE
    ref = cref.Reference(f["S"], cref.fixture_bank(), f["th"])
    ref.ptr = f["ptr0"]
    assert np.array_equal(z["bank0"], cref.fixture_bank())
    calls = []
    for i in range(len(f["K"])):
        feat_s, score, feat_t = cref.fixture_inputs(i)
        ref.bank = np.array(z["bank_%d" % (i - 1)] if i else z["bank0"], dtype=np.float64)
        out = ref(feat_s, score, feat_t, perms=(z["perm_%d" % i], z["perm_q_%d" % i]))
        calls.append(({k: z["%s_%d" % (k, i)] for k in ("loss", "grad", "bank", "ptr")}, out))
    return calls


def test_the_fixture_covers_the_count_and_pointer_branches(replay):
    f = cref.FIXTURE
    s = f["S"]
    ks = [k for call in f["K"] for k in call]
    assert any(0 < k < s for k in ks) and any(k == s for k in ks) and any(k > s for k in ks) and 0 in ks
    before, seen = f["ptr0"], set()
    for fix, out in replay:
        cnt = min(out["A"], s)
        seen.add("exact" if before + cnt == 4 * s else "past" if before + cnt > 4 * s else "plain")
        before = int(fix["ptr"])
    assert seen == {"exact", "past", "plain"}


def test_the_reference_lies_within_the_derived_bounds_on_every_call(replay):
    f = cref.FIXTURE
    worst = {"loss": 0.0, "grad": 0.0, "bank": 0.0}
    for i, (fix, out) in enumerate(replay):
        bd = cref.bounds(f["D"], out["A"], f["S"], out["norm"])
        assert fix["loss"].dtype == np.float32 and fix["grad"].dtype == np.float32
        r_loss = cref.ratio(float(fix["loss"]) - out["loss"], bd["loss"])
        r_grad = cref.ratio(fix["grad"] - out["grad"], cref.grad_bound_dense(out["grad"].shape, out["anchors"], bd["grad"]))
        lo, hi = out["written"]
        bank_bound = np.zeros(fix["bank"].shape)
        bank_bound[lo:hi] = bd["bank"]
        r_bank = cref.ratio(fix["bank"] - out["bank"], bank_bound)        # rows outside [lo, hi): bit-unchanged
        assert r_loss <= 1 and r_grad <= 1 and r_bank <= 1, (i, r_loss, r_grad, r_bank)
        assert np.abs(out["grad"]).max() > 0 and hi - lo == min(out["A"], f["S"])
        for k, r in (("loss", r_loss), ("grad", r_grad), ("bank", r_bank)):
            worst[k] = max(worst[k], r)
    print("reference fp32 against the fp64 restatement, largest error / bound:", worst)
    assert all(v > 0 for v in worst.values())          # (an fp32 run that agreed with fp64 to the last bit would be no fp32 run)


def test_the_pointer_sequence_is_the_fixtures(replay):
    assert [int(fix["ptr"]) for fix, _ in replay] == [out["ptr"] for _, out in replay] == [57, 0, 16, 32, 48, 0]


def test_host_mode_draws_in_the_references_order():
    """The module's host draws -- randperm(K_b) per cloud, then randperm(A), from the global generator -- are the
    permutations the reference drew after the same seed (its constructor's randn for the bank included)."""
    import types
    import torch
    from geot_amd.utils.cluster_contrastloss import nativeContrastLoss_t
    z = np.load(FIXTURE)
    f = cref.FIXTURE
    torch.manual_seed(f["seed"])
    torch.randn((4 * f["S"], 128))
    me = types.SimpleNamespace(th=f["th"])
    for i in range(len(f["K"])):
        score = torch.from_numpy(cref.fixture_inputs(i)[1])
        perm, perm_q = nativeContrastLoss_t._host_perms(me, score, f["B"], f["S"])
        assert np.array_equal(perm.numpy(), z["perm_%d" % i]) and np.array_equal(perm_q.numpy(), z["perm_q_%d" % i]), i


def test_the_restatement_on_hand_checked_values():
    # one cloud, three points, two over the threshold; D = 2, S = 1: the first entry of the permutation picks the anchor
    score = np.array([[0.95, 0.1, 0.9]], np.float32)
    sel = cref.select(score, 0.9, 1, perms=([np.array([1, 0])], np.array([0])))
    assert list(sel["anchors"]) == [2] and sel["A"] == 1 and list(sel["m"]) == [1]
    sel = cref.select(np.array([[np.nan, 0.1, 0.2]], np.float32), 0.9, 4, perms=([np.zeros(0, np.int64)], np.zeros(0, np.int64)))
    assert sel["A"] == 0
    feat = np.array([[[3.0, 4.0], [1.0, 0.0], [0.0, 2.0]]])
    bank = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])
    out = cref.loss_grad(feat, feat, np.array([2]), bank, tau=0.5)
    # x^ = t^ = (0, 1): u = 2 alone (shift 0, sum 1); v = (0, 2, 0, -2) shifted by 2
    z = 1.0 + np.exp(-2.0) + 1.0 + np.exp(-2.0) + np.exp(-4.0)
    assert abs(out["loss"] - 0.5 * np.log(z)) < 1e-15
    w = np.array([0.0, 1.0]) + np.exp(-2.0) * bank[0] + bank[1] + np.exp(-2.0) * bank[2] + np.exp(-4.0) * bank[3]
    dy = -(np.array([0.0, 1.0]) - w / z)
    want = (dy - np.array([0.0, 1.0]) * dy[1]) / 2.0
    assert np.allclose(out["grad"][0, 2], want, atol=1e-15) and not out["grad"][0, :2].any()
    empty = cref.loss_grad(feat, feat, np.zeros(0, np.int64), bank)
    assert empty["loss"] == 0.0 and not empty["grad"].any()
    new, ptr, rng = cref.enqueue(np.array([[0.6, 0.8]]), np.array([0]), bank, 3, 1)
    assert ptr == 0 and rng == (3, 4) and np.allclose(new[3], [0.6, 0.8]) and np.array_equal(new[:3], bank[:3])
    new, ptr, rng = cref.enqueue(np.array([[0.6, 0.8]]), np.array([0]), bank, 1, 1)
    assert ptr == 2 and rng == (1, 2)
