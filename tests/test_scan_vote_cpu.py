"""Voting whole-scan predictions, the part that needs no GPU: the ABI and the binding of geot_scan_vote, the refusals that
come before any device call, and the fp64 reference the GPU tests compare against (tests/_scan_vote_ref.py) against a plain
loop."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scan_vote_ref as vref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_version_and_signature():
    import ctypes
    from geot_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    assert int(re.search(r"GEOT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 21
    assert int(re.search(r"#define GEOT_VOTE_SET (\d+)", hdr).group(1)) == _lib.VOTE_SET == 1
    assert int(re.search(r"#define GEOT_VOTE_FINISH (\d+)", hdr).group(1)) == _lib.VOTE_FINISH == 2
    lib = _lib.load()
    assert lib.geot_abi_version() == _lib.ABI_VERSION
    decl = re.search(r"int geot_scan_vote\(([^;]*)\);", hdr).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args[14:16] == ["float *acc", "int mode"] and args[-1] == "void *stream" and len(args) == 21
    proto = _lib.PROTOTYPES["geot_scan_vote"]
    assert len(proto) == len(args)
    for a, t in zip(args, proto):
        want = ctypes.c_void_p if "*" in a else ctypes.c_longlong if a.startswith("long long") else ctypes.c_int
        assert t is want, (a, t)
    assert lib.geot_scan_vote.argtypes == proto
    # the same arguments as geot_scan_predict, with (acc, mode) in front of pred
    predict = _lib.PROTOTYPES["geot_scan_predict"]
    assert proto[:14] + proto[16:] == predict


def test_num_votes_below_one_is_refused():
    from geot_amd.validation import validate_scans_voted, vote_scans

    class Never:
        def eval(self):
            raise AssertionError("called")
    for cfg, kw in ((type("Cfg", (), {"num_votes": 0, "num_points": 8})(), {}), ({"num_points": 8}, {}),
                    ({"num_votes": 10, "num_points": 8}, {"num_votes": 0}), ({"num_votes": 10}, {"num_votes": -3})):
        with pytest.raises(ValueError, match="validate_scans is the un-voted call"):
            validate_scans_voted(Never(), None, cfg, **kw)
    with pytest.raises(RuntimeError, match="num_votes >= 1"):
        vote_scans(Never(), None, [0], 0)


def test_vote_batcher_refuses_what_the_view_program_refuses_before_any_device_call():
    from geot_amd.openpoints.dataset import VoteBatcher
    for vote in (["RandomDropout"], ["PointCloudScaling", "ChromaticNormalize"], ["NoSuchTransform"]):
        with pytest.raises(NotImplementedError, match=vote[-1]):
            VoteBatcher(None, 2048, vote=vote)          # the scans are never looked at
    with pytest.raises(RuntimeError, match="DeviceScanSet"):
        VoteBatcher(None, 2048, vote=[])
    with pytest.raises(RuntimeError, match="list of transform class names"):
        VoteBatcher(None, 2048, vote="PointCloudScaling")


def _loop(unknown, known, probs):
    """The votes of a few vertices, one statement at a time in python floats (fp64) from fp32 squared distances."""
    m, c = unknown.shape[0], probs[0].shape[0]
    total = np.zeros((m, c))
    for kn, prob in zip(known, probs):
        for v in range(m):
            cand = []
            for j in range(kn.shape[0]):
                dx, dy, dz = (np.float32(unknown[v, a] - kn[j, a]) for a in range(3))
                cand.append((np.float32(np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(dz * dz)), j))
            cand = sorted(cand)[:3]
            cand += [(np.float32(np.inf), 0)] * (3 - len(cand))
            r = [1.0 / (float(np.sqrt(np.float64(d))) + 1e-8) for d, _ in cand]
            norm = (r[0] + r[2]) + r[1]
            for k in range(c):
                p = [float(prob[k, j]) for _, j in cand]
                total[v, k] += (p[0] * (r[0] / norm) + p[1] * (r[1] / norm)) + p[2] * (r[2] / norm)
    return total


@pytest.mark.parametrize("n", [1, 2, 3, 9])
def test_reference_equals_a_plain_loop(n):
    rng = np.random.default_rng(7 + n)
    m, c, votes = 50, 5, 3
    unknown = (rng.random((m, 3)) * 40 - 7).astype(np.float32)
    known = [(rng.random((n, 3)) * 40 - 7).astype(np.float32) for _ in range(votes)]
    if n >= 3:
        unknown[4] = known[1][2]                        # d = 0
        known[2][1] = known[2][0]                       # an exact tie, decided by index
    logits = [rng.normal(size=(c, n)) * 3 for _ in range(votes)]
    probs = [(np.exp(l) / np.exp(l).sum(0)).astype(np.float32) for l in logits]
    parts = []
    for kn, prob in zip(known, probs):
        d2, idx = vref.three_nn(unknown, kn)
        assert d2.dtype == np.float32 and (d2[:, :-1] <= d2[:, 1:]).all() and (idx[:, min(n, 3):] == 0).all()
        assert np.isinf(d2[:, min(n, 3):]).all()
        parts.append((prob, d2, idx))
    got, want = vref.vote_sum(parts), _loop(unknown, known, probs)
    assert got.shape == (m, c) and np.abs(got - want).max() <= 1e-14
    assert np.abs(got.sum(1) - votes).max() <= 1e-6     # probabilities: every vote's weights sum to one
    assert np.array_equal(vref.argmax(got), want.argmax(1))


def test_reference_argmax_rule_and_margins():
    nan = np.nan
    rows = np.array([[1.0, 3.0, 3.0, 2.0], [0.0, nan, 5.0, nan], [nan, 1.0, 2.0, 3.0], [2.0, 2.0, 2.0, 2.0], [0.0, 1.0, 1.0 + 1e-7, 0.5]])
    assert vref.argmax(rows).tolist() == [1, 1, 0, 0, 2]
    import torch
    assert torch.argmax(torch.from_numpy(rows), dim=1).tolist() == vref.argmax(rows).tolist()
    assert vref.decided(rows, 1).tolist() == [False, True, True, False, False]
    assert vref.decided(rows[:, :1], 4).all()
    assert vref.tolerance(1) == 17 * 2.0 ** -24 and vref.tolerance(4) == 80 * 2.0 ** -24
    d2, idx = vref.three_nn(np.array([[nan, 0, 0]], np.float32), np.zeros((5, 3), np.float32))
    assert np.isinf(d2).all() and (idx == 0).all()
    assert np.isnan(vref.interpolate(np.ones((2, 5), np.float32), d2, idx)).all()     # 0 / 0 weights, as in fp32
