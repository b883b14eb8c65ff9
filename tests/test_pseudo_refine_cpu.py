"""Refining FixMatch pseudo-label masks, the part that needs no GPU: the ABI and the binding of geot_pseudo_refine, its
refusals before any launch, the numpy restatement the GPU tests compare against (tests/_pseudo_refine_ref.py) against the
reference-executed fixture (tests/golden/pseudo_label_refine_ref.npz, every point, all three modes), and the cfg keys."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pseudo_refine_ref as pref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "pseudo_label_refine_ref.npz")


def test_abi_version_and_signature():
    from geot_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    assert int(re.search(r"GEOT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 23
    lib = _lib.load()
    assert lib.geot_abi_version() == _lib.ABI_VERSION
    decl = re.search(r"int geot_pseudo_refine\(([^;]*)\);", hdr).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["int b", "int c", "int npts", "int n", "int k", "int mode", "float th", "float beta", "const float *prob",
                    "const int *nbr", "const float *e_joint", "unsigned char *keep", "float *value", "void *stream"]
    proto = _lib.PROTOTYPES["geot_pseudo_refine"]
    assert len(proto) == len(args)
    for a, t in zip(args, proto):
        want = ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float") else ctypes.c_int
        assert t is want, (a, t)
    assert lib.geot_pseudo_refine.argtypes == proto
    for name, value in _lib.PSEUDO_MODES.items():
        assert int(re.search(r"#define GEOT_PSEUDO_%s (\d+)" % name.upper(), hdr).group(1)) == value
    assert int(re.search(r"#define GEOT_PSEUDO_REFINE_MAX_N (\d+)", hdr).group(1)) == _lib.PSEUDO_REFINE_MAX_N == 32
    assert "pseudo_refine.hip" in build.SOURCES


def test_entry_point_refusals_need_no_device():
    from geot_amd import _lib
    lib = _lib.load()
    fake = 1 << 20          # hipErrorInvalidValue (1) before the launch: the pointers are never followed
    good = dict(b=2, c=17, npts=300, n=4, k=1, mode=0, th=0.9, beta=0.6, prob=fake, nbr=fake, e=None, keep=fake, value=None)
    for change in (dict(k=5), dict(k=0), dict(n=0), dict(n=33, k=1), dict(npts=4), dict(c=0), dict(c=33), dict(b=0), dict(b=65536),
                   dict(mode=3), dict(mode=-1), dict(mode=1, c=1), dict(mode=2, c=1, e=fake), dict(mode=2), dict(prob=None),
                   dict(nbr=None), dict(keep=None)):
        a = dict(good, **change)
        assert lib.geot_pseudo_refine(*a.values(), None) == 1, change


def test_the_restatement_equals_the_reference_in_all_three_modes():
    from geot_amd.utils.pseudo_mask import E_JOINT
    z = np.load(FIXTURE)
    beta = np.array(z["beta_bits"], np.uint32).view(np.float32)
    cases = [str(c) for c in z["cases"]]
    assert {c.rsplit("_n", 1)[0] for c in cases} == set(pref.MODES) and len(cases) == 6
    assert z["prob"].shape == (2, 17, 300) and (z["min_gap_ulp"] >= 32).all() and (z["th_dist"] >= 1e-4).all()
    plain = z["prob"].max(1)
    for case, th in zip(cases, z["th"]):
        mode, n, k = re.match(r"(\w+)_n(\d+)_k(\d+)", case).groups()
        nbr = z["nbr_n" + n].astype(np.int32)
        assert np.array_equal(nbr, pref.neighbours_fp64(z["pos"], int(n))[0])
        keep, value = pref.refine(z["prob"], nbr, int(k), mode, th, beta, E_JOINT)
        want = z["mask_" + case]
        assert np.array_equal(keep, want), (case, int((keep != want).sum()))
        assert set(np.unique(want)) == {0, 1} and (want != (plain >= np.float32(th))).any(), case
        if mode != "max":
            assert np.array_equal(value.view(np.uint32), z["margin_" + case].view(np.uint32)), case
        assert np.abs(value.astype(np.float64) - th).min() >= 1e-4


def test_the_restatement_on_hand_checked_points():
    # one cloud, two classes, three points in a row: 0 - 1 - 2; n = 2, so everybody sees both others
    prob = np.array([[[0.9, 0.6, 0.2], [0.1, 0.4, 0.8]]], np.float32)
    nbr = np.array([[[1, 2], [0, 2], [1, 0]]], np.int32)
    beta = np.float32(0.5)
    f = np.float32
    keep, value = pref.refine(prob, nbr, 1, "max", 0.9, beta)
    # point 1: class 0 takes max(0.9, 0.2), class 1 max(0.1, 0.8)
    c0 = (f(0.6) + beta * f(0.9)) - ((f(0.6) * f(0.9)) * beta)
    c1 = (f(0.4) + beta * f(0.8)) - ((f(0.4) * f(0.8)) * beta)
    assert value[0, 1] == max(c0, c1) and keep[0, 1] == (max(c0, c1) >= f(0.9))
    keep2, margin = pref.refine(prob, nbr, 2, "margin", 0.0, beta)
    a = (f(0.6) + beta * f(0.9)) - ((f(0.6) * f(0.9)) * beta)
    a = (a + beta * f(0.2)) - ((a * f(0.2)) * beta)
    b = (f(0.4) + beta * f(0.8)) - ((f(0.4) * f(0.8)) * beta)
    b = (b + beta * f(0.1)) - ((b * f(0.1)) * beta)
    assert margin[0, 1] == abs(a - b) and keep2.all()
    # an id outside [0, N): that point alone is dropped
    nbr[0, 2, 1] = 3
    keep, value = pref.refine(prob, nbr, 1, "max", 0.0, beta)
    assert list(keep[0]) == [1, 1, 0] and np.isnan(value[0, 2]) and not np.isnan(value[0, :2]).any()


def test_check_cfg_accepts_and_rejects():
    from geot_amd import train_step as ts
    assert ts.NTM_CFG["pseudo_refine"] is False and ts.NTM_CFG["pseudo_refine_size"] == 4
    assert ts.NTM_CFG["pseudo_refine_neighbors"] == 1 and ts.pseudo_refine_mode(ts.NTM_CFG) is None
    for v, mode in ((False, None), (True, "max"), ("max", "max"), ("margin", "margin"), ("margin_v1", "margin_v1")):
        cfg = dict(ts.NTM_CFG, pseudo_refine=v)
        ts.check_cfg(cfg)
        assert ts.pseudo_refine_mode(cfg) == mode
    ts.check_cfg(dict(ts.NTM_CFG, pseudo_refine="margin", pseudo_refine_size=32, pseudo_refine_neighbors=32))
    for name in ("Poly1FocalLoss_U", "Poly1FocalLoss_U_corr", "Poly1FocalLoss_U_T"):
        ts.check_cfg(dict(ts.NTM_CFG, pseudo_refine=True, criterion_u=name))
    for bad in (None, 1, 0, 1.0, ["max"]):
        with pytest.raises(TypeError, match="pseudo_refine"):
            ts.check_cfg(dict(ts.NTM_CFG, pseudo_refine=bad))
    for bad in ("Max", "median", ""):
        with pytest.raises(ValueError, match="pseudo_refine"):
            ts.check_cfg(dict(ts.NTM_CFG, pseudo_refine=bad))
    for key in ("pseudo_refine_size", "pseudo_refine_neighbors"):
        for bad in (4.0, "4", True, None):
            with pytest.raises(TypeError, match=key):
                ts.check_cfg(dict(ts.NTM_CFG, pseudo_refine=True, **{key: bad}))
    for size, k in ((0, 1), (33, 1), (4, 0), (4, 5), (-1, -1)):
        with pytest.raises(ValueError, match="pseudo_refine"):
            ts.check_cfg(dict(ts.NTM_CFG, pseudo_refine=True, pseudo_refine_size=size, pseudo_refine_neighbors=k))
    with pytest.raises(ValueError, match="Weight_CELoss_U"):
        ts.check_cfg(dict(ts.NTM_CFG, pseudo_refine="max", criterion_u="Weight_CELoss_U"))
    ts.check_cfg(dict(ts.NTM_CFG, criterion_u="Weight_CELoss_U"))            # without refinement it stays allowed
    with pytest.raises(ValueError, match="margin_v1"):
        ts.check_cfg(dict(ts.NTM_CFG, pseudo_refine="margin_v1", num_classes=18))


def test_python_refusals_come_before_any_device_call():
    import torch
    from geot_amd.utils.pseudo_mask import neighbours, pseudo_refine_mask
    pred, pos = torch.full((2, 17, 12), 1 / 17), torch.zeros(2, 12, 3)
    with pytest.raises(RuntimeError, match="mode must be one of"):
        pseudo_refine_mask(pred, 0.9, pos, mode="median")
    with pytest.raises(RuntimeError, match="n_neigbors <= neigborhood_size"):
        pseudo_refine_mask(pred, 0.9, pos, neigborhood_size=4, n_neigbors=5)
    with pytest.raises(RuntimeError, match="n_neigbors <= neigborhood_size"):
        pseudo_refine_mask(pred, 0.9, pos, neigborhood_size=33)
    with pytest.raises(RuntimeError, match="no 12 nearest other points"):
        pseudo_refine_mask(pred, 0.9, pos, neigborhood_size=12)
    with pytest.raises(RuntimeError, match="fp32"):
        pseudo_refine_mask(pred.double(), 0.9, pos)
    with pytest.raises(RuntimeError, match="classes"):
        pseudo_refine_mask(pred[:, :1], 0.5, pos, mode="margin")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        pseudo_refine_mask(pred, 0.9, pos)
    with pytest.raises(RuntimeError, match="n must be an int"):
        neighbours(pos, 0)
    with pytest.raises(RuntimeError, match="no 12 nearest other points"):
        neighbours(pos, 12)
