"""The launch plan of the fused EdgeConv tail (csrc/edgeconv.hip), without a GPU.

geot_edgeconv_plan reports what geot_edgeconv_gn_max and its gradients launch for a shape, from the function the launchers
read.  Over random eligible shapes and dense grids around every switch, a plan must be launchable as it stands: LDS within
the CU's 160 KiB (forward rows of a CU shared by two workgroups within 64 KiB), slice counts within what the kernels'
partial areas hold, grid dimensions within 65535, the partial records, the backward's coefficients and the reverse index
inside the workspace without overlap.  Eligibility must equal the limits include/geot_hip.h states."""
import numpy as np
import pytest

from _edgeconv_ref import MODEL_SHAPES, plan

LDS_CU = 160 * 1024
LDS_LIMIT = 150 * 1024          # EC_LDS_BYTES: the dynamic rows of either kernel
SHARED_CU = 64 * 1024           # forward rows of ch >= 2 channels: two workgroups per CU
MAX_SLICES, MAX_RED_SLICES = 32, 16
EC_E = 4                        # pairs per lane's first share in the dP walk


@pytest.fixture(scope="module")
def lib():
    from geot_amd import _lib
    return _lib.load()


def header_eligible(b, c, nq, nk, k, groups):
    """include/geot_hip.h: c % groups == 0, k <= 255, b, c <= 65535, b nq k and b nk <= 2^31 - 16, nk <= 38400,
    nq <= 17066"""
    return (min(b, c, nq, nk, k, groups) >= 1 and c % groups == 0 and k <= 255 and b <= 65535 and c <= 65535 and
            b * nq * k <= 2 ** 31 - 16 and b * nk <= 2 ** 31 - 16 and nk <= 38400 and nq <= 17066)


def violations(lib, b, c, nq, nk, k, groups):
    """every bound a plan must meet; [] when it meets them all"""
    p = plan(lib, b, c, nq, nk, k, groups)
    bad = []

    def need(cond, what):
        if not cond:
            bad.append(what)
    need(p is not None, "not eligible")
    if p is None:
        return bad
    ch, bch = p["fwd_ch"], p["bwd_ch"]
    # channels per workgroup: the most of 4, 2, 1 whose rows fit 64 KiB (two workgroups per CU); rows past 16384 sources
    # take what one workgroup's 150 KiB holds (2 up to 19200 sources)
    need(ch == (4 if nk <= 4096 else 2 if nk <= 8192 else 1 if nk <= 16384 else 2 if nk <= 19200 else 1), "forward channels")
    need(bch == (4 if 9 * nq * 4 <= LDS_LIMIT else 2 if 9 * nq * 2 <= LDS_LIMIT else 1), "dP channels")
    need(p["fwd_lds"] == 4 * ch * nk and p["fwd_lds"] <= LDS_LIMIT, "forward LDS")
    need(ch == 1 or p["fwd_lds"] <= SHARED_CU or nk > 16384, "forward LDS of a shared CU")
    need(p["bwd_lds"] == 9 * bch * nq and p["bwd_lds"] <= LDS_LIMIT, "dP LDS")
    need(p["k4"] == (k == 4), "k4 instances")
    # slices: 1..32 (the reduce 1..16), at least 2048 items each, none empty (the forward's pivot is its first pair's y)
    for key, n, cap in (("fwd_slices", nq, MAX_SLICES), ("red_slices", nq, MAX_RED_SLICES), ("pslices", nk, MAX_SLICES)):
        s = p[key]
        need(1 <= s <= cap and (s == 1 or n // s >= 2048), key)
        need((s - 1) * -(-n // s) < n, key + " empty")
    need(-(-nq // p["fwd_slices"]) * k < 2 ** 24, "forward record count exact in fp32")
    # grids: (slices, ceil(c / ch), b) for both big kernels, (., c, b) for the element-wise ones
    need(c <= 65535 and b <= 65535 and -(-c // ch) <= 65535 and -(-c // bch) <= 65535, "grid")
    mean_len = -(-nq * k // nk)
    lg = 0
    while lg < 3 and (3 * EC_E) << lg < mean_len:
        lg += 1
    need(p["lg"] == lg, "dP lanes")
    # workspace: [partials | reverse index]; forward records, the reduce's pairs, then the coefficients at the tail
    need(p["rec"] == 4 and p["part_floats"] == b * c * MAX_SLICES * 4, "partials area")
    need(b * c * p["fwd_slices"] * p["rec"] <= p["coef_off"], "forward records under the coefficients")
    need(b * c * p["red_slices"] * 2 <= p["coef_off"], "reduce pairs under the coefficients")
    need(p["coef_off"] + 2 * b * groups <= p["part_floats"], "coefficients inside the partials area")
    need(p["rix_off"] >= 4 * p["part_floats"] and p["rix_off"] % 16 == 0, "reverse index after the partials")
    need(p["rix_off"] + 4 * int(lib.geot_edgeconv_rix_ints(b, nq, nk, k)) <= p["ws_bytes"], "reverse index inside")
    need(p["ws_bytes"] == lib.geot_edgeconv_ws_bytes(b, c, nq, nk, k), "workspace bytes = geot_edgeconv_ws_bytes")
    return bad


def _around(points, lo=1):
    return sorted({v + d for v in points for d in (-1, 0, 1) if v + d >= lo})


NK_SWITCHES = (4096, 8192, 16384, 19200, 38400)
NQ_SWITCHES = (4266, 8533, 17066)


def test_random_eligible_shapes_meet_every_bound(lib):
    rng = np.random.default_rng(7)
    n = 100_000
    b = np.exp(rng.uniform(0, np.log(64), n)).astype(int)
    c = np.exp(rng.uniform(0, np.log(4096), n)).astype(int)
    nq = np.exp(rng.uniform(0, np.log(17066), n)).astype(int)
    nk = np.exp(rng.uniform(0, np.log(38400), n)).astype(int)
    k = np.where(rng.random(n) < 0.5, 4, np.exp(rng.uniform(0, np.log(255), n)).astype(int))
    seen = set()
    for i in range(n):
        divs = [g for g in (1, 2, 4, 8, 32, int(c[i])) if c[i] % g == 0]
        g = divs[i % len(divs)]
        args = (int(b[i]), int(c[i]), int(nq[i]), int(nk[i]), int(k[i]), g)
        bad = violations(lib, *args)
        assert not bad, (args, bad)
        p = plan(lib, *args)
        seen.add(("fwd", p["k4"], p["fwd_ch"]))
        seen.add(("dP", p["k4"], p["bwd_ch"]))
    # the reachable kernel instances, each of them reached
    assert seen == {(d, k4, ch) for d in ("fwd", "dP") for k4 in (0, 1) for ch in (1, 2, 4)}


def test_switches_meet_every_bound(lib):
    ks = (1, 3, 4, 5, 16, 254, 255)
    for nk in _around(NK_SWITCHES) + [1, 2, 512, 2047, 2048, 2049]:
        for nq in _around(NQ_SWITCHES) + [1, 2047, 2048, 4095, 4096, 16384]:
            for k in ks:
                for b, c, g in ((1, 1, 1), (1, 4, 4), (1, 7, 1), (2, 512, 4), (8, 384, 4), (3, 6, 3)):
                    args = (b, c, nq, nk, k, g)
                    assert header_eligible(*args) == (plan(lib, *args) is not None), args
                    if header_eligible(*args):
                        bad = violations(lib, *args)
                        assert not bad, (args, bad)


def test_channel_switch_points(lib):
    def ch(nq, nk):
        p = plan(lib, 1, 8, nq, nk, 4, 1)
        return p["fwd_ch"], p["fwd_lds"], p["bwd_ch"]
    assert ch(100, 4096) == (4, 65536, 4) and ch(100, 4097)[0] == 2
    assert ch(100, 8192) == (2, 65536, 4) and ch(100, 8193)[:2] == (1, 32772)
    assert ch(100, 16384) == (1, 65536, 4) and ch(100, 16385)[:2] == (2, 131080)   # past 64 KiB: the LDS opt-in, 2 rows
    assert ch(100, 19200)[:2] == (2, 153600) and ch(100, 19201)[:2] == (1, 76804)
    assert ch(100, 38400)[1] == LDS_LIMIT and plan(lib, 1, 8, 100, 38401, 4, 1) is None
    assert ch(4266, 10)[2] == 4 and ch(4267, 10)[2] == 2
    assert ch(8533, 10)[2] == 2 and ch(8534, 10)[2] == 1
    assert ch(17066, 10)[2] == 1 and plan(lib, 1, 8, 17067, 10, 4, 1) is None
    # the slice caps: forward nq / 2048 (8 at most), dP nk / 2048 (18 at most), reduce 16
    p = plan(lib, 1, 4, 17066, 38400, 4, 1)
    assert (p["fwd_slices"], p["red_slices"], p["pslices"]) == (8, 8, 18)
    assert plan(lib, 1, 1, 17066, 38400, 4, 1)["red_slices"] == 8


def test_eligibility_equals_the_header(lib):
    rng = np.random.default_rng(8)
    cases = [(1, 8, 100, 100, 256, 1), (1, 8, 100, 100, 255, 1), (1, 6, 100, 100, 4, 4), (1, 65535, 10, 10, 4, 1),
             (1, 65536, 10, 10, 4, 1), (65535, 1, 10, 10, 4, 1), (65536, 1, 10, 10, 4, 1), (0, 1, 1, 1, 1, 1),
             (1, 0, 1, 1, 1, 1), (1, 1, 0, 1, 1, 1), (1, 1, 1, 0, 1, 1), (1, 1, 1, 1, 0, 1), (1, 1, 1, 1, 1, 0),
             (1, 8, 1, 1, 1, -1), (60000, 8, 17066, 38400, 2, 1), (55924, 8, 10, 38400, 4, 1),
             (55925, 8, 10, 38400, 4, 1), (65535, 8, 17066, 10, 1, 1), (65535, 8, 8192, 10, 4, 1)]
    for _ in range(20000):
        b = int(np.exp(rng.uniform(0, np.log(70000))))
        c = int(np.exp(rng.uniform(0, np.log(70000))))
        cases.append((b, c, int(rng.integers(1, 20000)), int(rng.integers(1, 42000)), int(rng.integers(1, 300)),
                      int(rng.choice([1, 2, 3, 4, 5, 8]))))
    for args in cases:
        assert header_eligible(*args) == (plan(lib, *args) is not None) == bool(lib.geot_edgeconv_eligible(*args)), args
        if header_eligible(*args):
            bad = violations(lib, *args)
            assert not bad, (args, bad)


def test_model_plans_are_pinned(lib):
    """the four call shapes of DGCNN_Propagation in the configured model: forward and dP at 2 channels per workgroup on
    8192 queries / sources, several slices per pass at one cloud"""
    want = {
        # (c, nq, nk): (fwd_ch, fwd_slices, red_slices, bwd_ch, pslices, lg) at b = 1, 2, 8
        (512, 4096, 512): ((4, 2, 1, 4, 1, 2), (4, 2, 1, 4, 1, 2), (4, 1, 1, 4, 1, 2)),
        (384, 4096, 4096): ((4, 2, 2, 4, 2, 0), (4, 2, 1, 4, 2, 0), (4, 1, 1, 4, 1, 0)),
        (512, 8192, 4096): ((4, 4, 1, 2, 2, 0), (4, 2, 1, 2, 1, 0), (4, 1, 1, 2, 1, 0)),
        (384, 8192, 8192): ((2, 3, 2, 2, 3, 0), (2, 2, 1, 2, 2, 0), (2, 1, 1, 2, 1, 0)),
    }
    for c, nq, nk, k, g in MODEL_SHAPES:
        for b, w in zip((1, 2, 8), want[(c, nq, nk)]):
            p = plan(lib, b, c, nq, nk, k, g)
            assert tuple(p[f] for f in ("fwd_ch", "fwd_slices", "red_slices", "bwd_ch", "pslices", "lg")) == w, (b, c, nq, nk)
            assert p["k4"] == 1 and p["fwd_lds"] == 4 * p["fwd_ch"] * nk and p["bwd_lds"] == 147456
            assert not violations(lib, b, c, nq, nk, k, g)
