"""geot_ntm_filtered_anchors (csrc/ntm_outlier.hip, include/geot_hip.h "ABI 26") called through the C ABI: the thresholds, the
anchor rows and the filtered maxima equal the numpy float32 restatement (tests/_outlier_ref.py, itself checked against the
reference's loop on CPU torch in tests/test_filter_outlier_cpu.py) BIT FOR BIT, at the smallest shapes that reach every branch
of the two kernels -- lo == hi, both interpolation forms, w = 0, one sweep of the workgroup +- 1, C = 1 and C = 32, N not a
multiple of 4 -- crossed with random, saturated (exact 1.0f, zeros, denormals), tied, constant, planted and negative inputs;
the public path; the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import _outlier_ref as ref
from geot_amd import _lib, ntm
from geot_amd.ext import _common
from geot_amd.ext._common import call, ptr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -7.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _abi(eta, q, with_v_star=True):
    B, C, N = eta.shape
    x = torch.from_numpy(np.array(eta)).to(DEV)
    class_T = torch.full((C, C), SENTINEL, device=DEV)
    v_star = torch.full((C,), SENTINEL, device=DEV) if with_v_star else None
    thresh = torch.full((C,), SENTINEL, device=DEV)
    call("geot_ntm_filtered_anchors", DEV, B, N, C, float(q), ptr(x), ptr(class_T), ptr(v_star), ptr(thresh))
    torch.cuda.synchronize()
    return class_T.cpu().numpy(), None if v_star is None else v_star.cpu().numpy(), thresh.cpu().numpy()


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_abi_equals_the_restatement_bit_for_bit(case):
    kind, shape, q, seed = case
    eta = ref.make_eta(kind, shape, seed)
    want_T, want_v, want_t, lo, hi = ref.expected(case)
    class_T, v_star, thresh = _abi(eta, q)
    bad = np.flatnonzero(_bits(thresh) != _bits(want_t))
    print("%s: lo %d hi %d, %d of %d thresholds differ" % (ref.case_id(case), lo, hi, bad.size, thresh.size))
    assert bad.size == 0, [(int(k), float(thresh[k]), float(want_t[k])) for k in bad[:4]]
    assert np.array_equal(_bits(v_star), _bits(want_v)), (v_star, want_v)
    assert np.array_equal(_bits(class_T), _bits(want_T)), np.argwhere(class_T != want_T)[:4]


def test_v_star_may_be_null():
    case = ("random", (1, 1025, 17), 0.97, 800)
    assert case in ref.CASES
    class_T, _, thresh = _abi(ref.make_eta(*case[:2], case[3]), 0.97, with_v_star=False)
    want_T, _, want_t, _, _ = ref.expected(case)
    assert np.array_equal(_bits(class_T), _bits(want_T)) and np.array_equal(_bits(thresh), _bits(want_t))


PUBLIC = [c for c in ref.CASES if c[2] == 0.97 and c[1][2] == 17 and (c[0] == "fixture" or (c[0] in ("random", "ties") and c[1] in (
    (2, 96, 17), (1, 1025, 17), (3, 5000, 17))))]


@pytest.mark.parametrize("case", PUBLIC, ids=ref.case_id)
def test_class_transition_takes_the_kernel_and_equals_the_composite(case, monkeypatch):
    """The public path: class_T of class_transition(filter_outlier=True) is the kernel's, equals the restatement (the referee)
    and the composite _filtered_anchor_rows patched in its place; should the device's torch.quantile ever differ in a
    threshold, the two thresholds are printed and the kernel must still equal the restatement."""
    kind, shape, q, seed = case
    eta = torch.from_numpy(np.array(ref.make_eta(kind, shape, seed))).to(DEV)
    sigma, ema_t = torch.full((17,), 0.4, device=DEV), torch.eye(17, device=DEV)
    names = []
    real = _common._launch
    monkeypatch.setattr(_common, "_launch", lambda name, *a: (names.append(name), real(name, *a))[1])
    fused = ntm.class_transition(eta, sigma, ema_t, filter_outlier=True)
    assert names == ["geot_ntm_filtered_anchors", "geot_ntm_class_transition"], names
    monkeypatch.setattr(ntm, "filtered_anchors", lambda e, q_: ntm._filtered_anchor_rows(e, q_) + (None,))
    composite = ntm.class_transition(eta, sigma, ema_t, filter_outlier=True)
    assert names[2:] == ["geot_ntm_class_transition"], names
    torch.cuda.synchronize()
    want_T, _, want_t, _, _ = ref.expected(case)
    assert np.array_equal(_bits(fused[2].cpu().numpy()), _bits(want_T))
    dev_t = torch.quantile(eta.transpose(0, 1).reshape(17, -1), q, dim=1).cpu().numpy()
    if not np.array_equal(dev_t, want_t):
        print("device torch.quantile differs from the restatement:", [(k, float(dev_t[k]), float(want_t[k]))
                                                                      for k in np.flatnonzero(dev_t != want_t)])
    for a, b in zip(fused, composite):
        assert torch.equal(a, b)


def test_filter_off_still_reaches_the_plain_anchor_kernel(monkeypatch):
    eta = torch.from_numpy(np.array(ref.make_eta("random", (2, 96, 17), 500))).to(DEV)
    names = []
    real = ntm.call
    monkeypatch.setattr(ntm, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    monkeypatch.setattr(ntm, "filtered_anchors", lambda *a, **k: pytest.fail("filter_outlier is off"))
    out = ntm.class_transition(eta, torch.full((17,), 0.4, device=DEV), torch.eye(17, device=DEV))
    torch.cuda.synchronize()
    assert names == ["geot_ntm_class_anchors", "geot_ntm_class_transition"], names
    assert not np.array_equal(out[2].cpu().numpy(), ref.expected(("random", (2, 96, 17), 0.97, 500))[0])


@pytest.mark.parametrize("b,n,c,q", [(1, 64, 0, 0.97), (1, 64, 33, 0.97), (0, 64, 17, 0.97), (1, 0, 17, 0.97), (1, 64, 17, 1.5),
                                     (1, 64, 17, -0.01), (1, 64, 17, float("nan")), (4097, 4096, 17, 0.97)],
                         ids=["c0", "c33", "b0", "n0", "q1.5", "q-0.01", "qnan", "points-over-2^24"])
def test_refusals_return_an_error_code_and_launch_nothing(b, n, c, q):
    lib = _lib.load()
    eta = torch.rand(1, 33, 64, device=DEV)         # (the refused sizes are never used to address it)
    out = torch.full((33 * 33 + 2 * 33,), SENTINEL, device=DEV)
    class_T, v_star, thresh = out[:33 * 33], out[33 * 33:33 * 34], out[33 * 34:]
    stream = torch.cuda.current_stream().cuda_stream
    err = lib.geot_ntm_filtered_anchors(b, n, c, ctypes.c_double(q), ptr(eta), ptr(class_T), ptr(v_star), ptr(thresh), stream)
    torch.cuda.synchronize()
    assert err != 0 and bool((out == SENTINEL).all())
    with pytest.raises(RuntimeError, match="geot_ntm_filtered_anchors"):
        call("geot_ntm_filtered_anchors", DEV, b, n, c, q, ptr(eta), ptr(class_T), ptr(v_star), ptr(thresh))


def test_wrapper_refuses_before_the_abi():
    with pytest.raises(RuntimeError, match="filtered_anchors: takes"):
        ntm.filtered_anchors(torch.rand(1, 33, 8, device=DEV))
    with pytest.raises(RuntimeError, match="filtered_anchors: takes"):
        ntm.filtered_anchors(torch.rand(1, 17, 8, device=DEV), q=1.5)
    with pytest.raises(RuntimeError, match="filtered_anchors: eta: CPU not supported"):
        ntm.filtered_anchors(torch.rand(1, 17, 8))
