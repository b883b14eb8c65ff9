"""The launch plan of the fused SetAbstraction kernel (csrc/sa_mlp.hip) and the host side that decides whether a module
takes it (geot_amd/sa_fused.py), without a GPU.

geot_sa_plan reports what geot_sa_group_mlp_max launches for a shape, from the function the launcher reads.  Over 100 k
random shapes and dense grids around every switch, a plan must be launchable as it stands (LDS within 160 KiB, threads
within the variant's __launch_bounds__, the most waves that fit), its path switches must hold their preconditions, its
persistent grid must cover every group exactly once, and it must be what the launcher chose before the plan was pulled out
of it.  fused_sa_available must mean exactly "the plan exists".  The module-structure cases pin which SharedMLP stacks the
fold accepts, and check pack_params against fp64 (it is plain torch)."""
import ctypes
import random

import numpy as np
import pytest
import torch
import torch.nn as nn

from _sa_ref import BENCH_SA, LDS_CU, PLAN_FIELDS, legacy_plan, make_mlp, pad_cols, plan

CUS = (80, 256, 304)
NSAMPLES = (8, 16, 32, 64, 96, 128, 256)
WIDTHS = (1, 2, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256)


@pytest.fixture(scope="module")
def lib():
    from geot_amd import _lib
    return _lib.load()


def nsample_ok(ns):
    return ns in (8, 16) or (ns >= 32 and ns % 32 == 0)


def violations(lib, b, npoint, nsample, c_feat, widths, cus, aligned=True):
    """every bound and switch rule a plan must meet; [] when it meets them all"""
    p = plan(lib, b, npoint, nsample, c_feat, widths, cus, aligned)
    old = legacy_plan(b, npoint, nsample, c_feat, widths, cus, aligned)
    bad = []

    def need(cond, what):
        if not cond:
            bad.append(what)
    need((p is None) == (old is None), "refusal differs from the launcher's")
    if p is None or old is None:
        return bad
    ngroups = b * npoint
    if ngroups:
        need(p == old, "plan differs from the launcher's: %s" % {k: (p[k], old[k]) for k in p if p[k] != old[k]})
    else:
        need(p["blocks"] == 0, "b * npoint == 0 launches nothing")
    nl = len(widths)
    cps = [pad_cols(w) for w in widths]
    # the descriptor
    kp0 = (3 + c_feat + 1) & ~1
    need([p["kp%d" % l] for l in range(nl)] == [kp0] + cps[:-1], "kp")
    need([p["cp%d" % l] for l in range(nl)] == cps, "cp")
    need(all(p[f % l] == 0 for l in range(nl, 4) for f in ("kp%d", "cp%d", "woff%d", "boff%d")), "unused layers")
    off = 0
    for l in range(nl):
        need(p["woff%d" % l] == off and p["boff%d" % l] == off + p["kp%d" % l] * cps[l], "offsets of layer %d" % l)
        off = p["boff%d" % l] + cps[l]
    need(p["param_floats"] == off, "parameter floats")
    arr = (ctypes.c_int * nl)(*widths)
    need(lib.geot_sa_param_floats(c_feat, nl, arr) == p["param_floats"], "geot_sa_param_floats")
    need(p["act_stride"] == max([kp0] + cps[:-1]) + 1 and p["act_stride"] % 2 == 1, "act_stride")
    # variant, waves, LDS
    wide = max(cps) > 128
    need(p["wide"] == int(wide), "wide <=> a padded width > 128")
    gpt = 1 if nsample >= 32 else 32 // nsample
    need(p["gpt"] == gpt and p["tpg"] == (nsample // 32 if nsample >= 32 else 1), "gpt / tpg")
    need(gpt * nsample == 32 or p["tpg"] * 32 == nsample, "tiles hold whole groups or groups whole tiles")
    per_wave = 32 * p["act_stride"] + gpt * cps[-1]

    def lds(w):
        return 4 * (p["param_floats"] + w * per_wave)
    need(p["lds"] == lds(p["waves"]) and p["lds"] <= LDS_CU, "LDS")
    choices = (8, 4) if wide else (12, 8, 4)
    need(p["waves"] in choices, "waves")
    need(all(lds(w) > LDS_CU for w in choices if w > p["waves"]), "not the most waves that fit")
    need(p["waves"] * 64 <= (512 if wide else 768), "threads over __launch_bounds__")
    # the persistent grid
    nunits = -(-ngroups // gpt)
    need(p["nunits"] == nunits, "units")
    need(p["blocks"] == min(-(-nunits // p["waves"]), cus) and p["blocks"] <= cus, "workgroups")
    # the fast path
    fast = (nsample == 32 and c_feat <= 8 and widths[-1] == cps[-1] and widths[-1] >= 64 and ngroups < 2 ** 31 - 1 and
            ngroups * 32 < (2 ** 31 - 1) * 4)
    need(p["fast_np"] == (widths[-1] // 64 if fast else 0), "fast_np")
    need(p["fast_np"] in (0, 1, 2, 4), "fast_np value")
    run8 = bool(p["fast_np"]) and npoint % 8 == 0 and aligned and nunits >= 16 * p["blocks"] * p["waves"]
    need(p["run_len"] == (8 if run8 else 1), "run_len")
    if p["blocks"]:
        if p["fast_np"]:
            nruns = ngroups // p["run_len"]
            need(nruns * p["run_len"] == ngroups, "runs drop groups")
            need(-(-nruns // p["blocks"]) * p["blocks"] >= nruns, "runs uncovered")
            need(nruns < 2 ** 31, "run index fits int")
        else:
            need(-(-nunits // p["blocks"]) * p["blocks"] >= nunits and nunits * gpt >= ngroups, "units uncovered")
    return bad


def coverage(p, b, npoint):
    """how often each group is visited by the kernel's partition (workgroup ranges x wave strides), restated"""
    ngroups = b * npoint
    seen = np.zeros(ngroups, np.int64)
    blocks, waves = p["blocks"], p["waves"]
    if p["fast_np"]:
        rl = p["run_len"]
        nruns = ngroups // rl
        chunk = -(-nruns // blocks)
        for blk in range(blocks):
            end = min((blk + 1) * chunk, nruns)
            for w in range(waves):
                for run in range(blk * chunk + w, end, waves):
                    seen[run * rl:(run + 1) * rl] += 1
    else:
        gpt, nunits = p["gpt"], p["nunits"]
        chunk = -(-nunits // blocks)
        for blk in range(blocks):
            end = min((blk + 1) * chunk, nunits)
            for w in range(waves):
                for u in range(blk * chunk + w, end, waves):
                    seen[u * gpt:min((u + 1) * gpt, ngroups)] += 1
    return seen


def test_bench_shape_plan(lib):
    """configs[1]: lean, 12 waves, 2 stores of 64 columns per group on the register-pooled path, 4-byte stores (6000 groups
    are too few for runs of 8 on 256 CUs)"""
    s = BENCH_SA
    p = plan(lib, s["b"], s["npoint"], s["nsample"], s["c_feat"], s["widths"], 256)
    assert (p["wide"], p["waves"], p["gpt"], p["tpg"], p["fast_np"], p["run_len"], p["blocks"]) == (0, 12, 1, 1, 2, 1, 256)
    assert violations(lib, s["b"], s["npoint"], s["nsample"], s["c_feat"], s["widths"], 256) == []


def test_plan_refusals_leave_out_untouched(lib):
    for args in ((1, 100, 24, 3, (64,)), (1, 100, 32, 3, (64, 0)), (1, 100, 32, 3, (257,)), (-1, 100, 32, 3, (64,)),
                 (1, -1, 32, 3, (64,)), (1, 100, 32, -1, (64,)), (1, 100, 32, 3, (64,) * 5), (1, 100, 32, 3, (128, 128, 128)),
                 (1, 100, 32, 40000, (64,)), (1, 100, 0, 3, (64,)), (1, 100, -32, 3, (64,))):
        b, npoint, ns, cf, ws = args
        arr = (ctypes.c_int * len(ws))(*ws)
        out = (ctypes.c_longlong * len(PLAN_FIELDS))(*([-7] * len(PLAN_FIELDS)))
        assert lib.geot_sa_plan(b, npoint, ns, cf, len(ws), arr, 256, 1, out, len(PLAN_FIELDS)) == 0, args
        assert list(out) == [-7] * len(PLAN_FIELDS)
        assert legacy_plan(b, npoint, ns, cf, ws) is None, args
    arr = (ctypes.c_int * 1)(64)
    assert lib.geot_sa_plan(1, 100, 32, 3, 1, arr, 0, 1, None, 0) == 0            # no CUs
    assert lib.geot_sa_plan(1, 100, 32, 3, 1, None, 256, 1, None, 0) == 0         # no widths
    out = (ctypes.c_longlong * len(PLAN_FIELDS))(*([-7] * len(PLAN_FIELDS)))
    assert lib.geot_sa_plan(1, 100, 32, 3, 1, arr, 256, 1, out, 3) == 1 and list(out)[3:] == [-7] * (len(PLAN_FIELDS) - 3)


def test_dispatcher_forwards_the_plan(lib):
    """the compiled dispatcher forwards geot_sa_plan too (host arrays as addresses, like geot_edgeconv_plan)"""
    from geot_amd import build_torch_ext
    disp = build_torch_ext.load("_geot_dispatch_cpp")
    s = BENCH_SA
    arr = (ctypes.c_int * 3)(*s["widths"])
    out = (ctypes.c_longlong * len(PLAN_FIELDS))(*([-7] * len(PLAN_FIELDS)))
    assert disp.geot_sa_plan(s["b"], s["npoint"], s["nsample"], s["c_feat"], 3, ctypes.addressof(arr), 256, 1,
                             ctypes.addressof(out), len(PLAN_FIELDS)) == 1
    assert dict(zip(PLAN_FIELDS, out)) == plan(lib, s["b"], s["npoint"], s["nsample"], s["c_feat"], s["widths"], 256)
    assert disp.geot_sa_plan(1, 100, 24, 3, 3, ctypes.addressof(arr), 256, 1, None, 0) == 0


def test_random_shapes(lib):
    rng = random.Random(20261016)
    seen = set()
    for _ in range(100_000):
        nl = rng.randint(1, 4)
        widths = tuple(rng.choice(WIDTHS) if rng.random() < 0.5 else rng.randint(1, 256) for _ in range(nl))
        c_feat = rng.choice((0, 1, 2, 3, 5, 8, 9, 13, 29, 61, 62, 125, 200, 509, 1000)) if rng.random() < 0.7 else rng.randint(0, 300)
        nsample = rng.choice(NSAMPLES + (24, 48, 4))
        b = rng.choice((0, 1, 2, 3, 8, 16, 64))
        npoint = rng.choice((0, 1, 7, 8, 100, 512, 1024, 6000, 8192, 40000)) if rng.random() < 0.6 else rng.randint(1, 70000)
        cus = rng.choice(CUS)
        aligned = rng.random() < 0.8
        bad = violations(lib, b, npoint, nsample, c_feat, widths, cus, aligned)
        assert bad == [], (b, npoint, nsample, c_feat, widths, cus, aligned, bad)
        p = plan(lib, b, npoint, nsample, c_feat, widths, cus, aligned)
        if p:
            seen.add((p["wide"], p["waves"], p["gpt"], p["fast_np"], p["run_len"]))
    # the sample reaches every (variant, waves) pair, every gpt, every fast_np, both run lengths
    assert {(w, v) for w, v, _, _, _ in seen} == {(0, 12), (0, 8), (0, 4), (1, 8), (1, 4)}
    assert {g for _, _, g, _, _ in seen} == {1, 2, 4} and {f for _, _, _, f, _ in seen} == {0, 1, 2, 4}
    assert {r for *_, r in seen} == {1, 8}


def test_switch_grids(lib):
    """dense around every switch: the waves as the widths and c_feat grow, run_len 8 as b * npoint crosses
    16 * blocks * waves, the fast path's c_feat <= 8 / width >= 64 / unpadded width, npoint % 8, alignment"""
    for cus in CUS:
        for nsample in (8, 16, 32, 64):
            for widths in ((64, 64, 128), (128, 64), (64, 256), (32,), (1,), (33, 129), (256, 256), (100, 200, 31, 256),
                           (128, 128, 128), (128, 128), (64, 128, 128), (256,), (200, 64)):
                for c_feat in list(range(0, 12)) + list(range(56, 70)) + [120, 125, 126, 127, 128, 250, 253, 254, 255, 256, 509, 510]:
                    for b, npoint in ((1, 6000), (1, 6001), (2, 8192), (3, 7)):
                        bad = violations(lib, b, npoint, nsample, c_feat, widths, cus)
                        assert bad == [], (b, npoint, nsample, c_feat, widths, cus, bad)
        # run_len 8 switches on where every wave of the grid gets 16 units, for each waves count of the fast path
        waves_seen = set()
        for c_feat, widths in ((3, (64, 64, 128)), (3, (64, 64, 64, 128)), (3, (128, 64)), (3, (64, 256)), (3, (64, 64, 64, 256))):
            p0 = plan(lib, 1, 8, 32, c_feat, widths, cus)
            assert p0["fast_np"] > 0
            waves_seen.add((p0["wide"], p0["waves"]))
            edge = 16 * cus * p0["waves"]
            for npoint in range(edge - 24, edge + 25, 8):
                p = plan(lib, 1, npoint, 32, c_feat, widths, cus)
                assert p["run_len"] == (8 if npoint >= edge else 1), (cus, c_feat, widths, npoint)
                assert plan(lib, 1, npoint, 32, c_feat, widths, cus, aligned=False)["run_len"] == 1
                assert plan(lib, 1, npoint + 4, 32, c_feat, widths, cus)["run_len"] == 1
                assert violations(lib, 1, npoint, 32, c_feat, widths, cus) == []
        assert waves_seen == {(0, 12), (0, 8), (0, 4), (1, 8), (1, 4)}, waves_seen


def test_issue_examples(lib):
    """switch points named where the plan was introduced, from the arithmetic: (variant, waves) per stack"""
    def vw(c_feat, widths, nsample=32):
        p = plan(lib, 1, 1000, nsample, c_feat, widths)
        return None if p is None else (p["wide"], p["waves"])
    assert vw(3, (64, 64, 128)) == (0, 12)
    assert vw(3, (128, 64)) == (0, 4)
    assert vw(61, (64, 64, 128)) == (0, 8)
    assert vw(3, (64, 256)) == (1, 8) and vw(3, (64, 256), 8) == (1, 4)
    assert vw(3, (128, 128, 128)) is None


def test_partition_covers_every_group_once(lib):
    rng = random.Random(7)
    cases = [(1, 6000, 32, 3, (64, 64, 128), 256), (2, 8192, 32, 3, (128, 64), 256), (1, 3073 * 12, 32, 3, (64, 64, 128), 256),
             (3, 1001, 16, 5, (64,), 80), (2, 999, 8, 0, (33, 31), 304), (1, 257, 64, 9, (100, 200), 256), (1, 5, 96, 1, (1,), 256)]
    for _ in range(100):
        cases.append((rng.randint(1, 4), rng.randint(1, 3000), rng.choice(NSAMPLES[:4]), rng.choice((0, 3, 8, 9)),
                      tuple(rng.choice(WIDTHS) for _ in range(rng.randint(1, 3))), rng.choice(CUS)))
    empty_ranges = 0
    for b, npoint, ns, cf, ws, cus in cases:
        p = plan(lib, b, npoint, ns, cf, ws, cus)
        if p is None:
            continue
        seen = coverage(p, b, npoint)
        assert (seen == 1).all(), (b, npoint, ns, cf, ws, cus, int(seen.min()), int(seen.max()))
        total = b * npoint // p["run_len"] if p["fast_np"] else p["nunits"]
        chunk = -(-total // p["blocks"])
        empty_ranges += (p["blocks"] - 1) * chunk >= total
    assert empty_ranges > 0          # some grids leave their last workgroups nothing


@pytest.mark.parametrize("nsample", NSAMPLES + (0, 4, 24, 48, 33))
def test_available_iff_plan(lib, nsample):
    from geot_amd.sa_fused import fused_sa_available
    for c_in, widths in ((6, (64, 64, 128)), (3, (64, 256)), (6, (128, 128, 128)), (64, (128, 128)), (130, (256,)),
                         (12, (1,)), (3, (32, 32, 32, 32)), (3, (32,) * 5), (2, (64,)), (512, (64,)), (260, (256, 128))):
        mlp = make_mlp(c_in, widths, device="cpu")
        want = c_in >= 3 and len(widths) <= 4 and plan(lib, 1, 1, nsample, c_in - 3, widths) is not None
        assert fused_sa_available(mlp, nsample) == want, (c_in, widths, nsample)
        assert want == (c_in >= 3 and len(widths) <= 4 and legacy_plan(1, 1, nsample, c_in - 3, widths) is not None)


# ---- which SharedMLP stacks fold --------------------------------------------------------------------------------------

def _stage(*mods):
    return nn.Sequential(*mods)


def _bn(c, **kw):
    m = nn.BatchNorm2d(c, **kw)
    with torch.no_grad():
        if m.running_mean is not None:
            m.running_mean.uniform_(-0.5, 0.5)
            m.running_var.uniform_(0.5, 2.0)
        if m.weight is not None:
            m.weight.uniform_(-1.5, 1.5)
            m.bias.uniform_(-0.3, 0.3)
    return m


def _refused_stacks():
    torch.manual_seed(0)
    c = nn.Conv2d
    return {
        "padding 1": nn.Sequential(_stage(c(6, 32, 1, padding=1), _bn(32), nn.ReLU())),
        "kernel 3": nn.Sequential(_stage(c(6, 32, 3), _bn(32), nn.ReLU())),
        "stride 2": nn.Sequential(_stage(c(6, 32, 1, stride=2), _bn(32), nn.ReLU())),
        "groups 2": nn.Sequential(_stage(c(6, 32, 1, groups=2), _bn(32), nn.ReLU())),
        "relu before bn": nn.Sequential(_stage(c(6, 32, 1), nn.ReLU(), _bn(32))),
        "bn twice": nn.Sequential(_stage(c(6, 32, 1), _bn(32), _bn(32), nn.ReLU())),
        "relu twice": nn.Sequential(_stage(c(6, 32, 1), nn.ReLU(), nn.ReLU())),
        "bn first (pre-activation)": nn.Sequential(_stage(_bn(6), c(6, 32, 1))),
        "no running stats": nn.Sequential(_stage(c(6, 32, 1), _bn(32, track_running_stats=False), nn.ReLU())),
        "bn in training": nn.Sequential(_stage(c(6, 32, 1), _bn(32).train(), nn.ReLU())),
        "leaky relu": nn.Sequential(_stage(c(6, 32, 1), _bn(32), nn.LeakyReLU())),
        "instance norm": nn.Sequential(_stage(c(6, 32, 1), nn.InstanceNorm2d(32), nn.ReLU())),
        "dropout": nn.Sequential(_stage(c(6, 32, 1), nn.Dropout()), _stage(c(32, 32, 1))),
        "bare conv": nn.Sequential(c(6, 32, 1)),
        "empty": nn.Sequential(),
        "five layers": nn.Sequential(*[_stage(c(6 if i == 0 else 32, 32, 1), nn.ReLU()) for i in range(5)]),
    }


@pytest.mark.parametrize("name", sorted(_refused_stacks()))
def test_refused_stacks(name):
    from geot_amd.sa_fused import _stages, fused_sa_available, pack_params
    mlp = _refused_stacks()[name].eval()
    if name == "bn in training":
        mlp[0][1].train()
    assert not fused_sa_available(mlp, 32)
    if name != "five layers":         # (a stack the fold takes, but the kernel does not)
        assert _stages(mlp) is None
        with pytest.raises(Exception):
            pack_params(mlp)


def _fold64(st):
    """the folded (W'^T (kp, cp), b' (cp)) blocks in fp64, from the unfolded stages"""
    blocks = []
    kp = (st[0][0].in_channels + 1) & ~1
    for conv, bn, _ in st:
        w = conv.weight.double().reshape(conv.out_channels, -1)
        b = conv.bias.double() if conv.bias is not None else torch.zeros(conv.out_channels, dtype=torch.float64)
        if bn is not None:
            g = bn.weight.double() if bn.weight is not None else torch.ones_like(b)
            beta = bn.bias.double() if bn.bias is not None else torch.zeros_like(b)
            s = g / torch.sqrt(bn.running_var.double() + bn.eps)
            w, b = w * s[:, None], (b - bn.running_mean.double()) * s + beta
        cp = pad_cols(conv.out_channels)
        wt = torch.zeros(kp, cp, dtype=torch.float64)
        wt[:conv.in_channels, :conv.out_channels] = w.t()
        bb = torch.zeros(cp, dtype=torch.float64)
        bb[:conv.out_channels] = b
        blocks += [wt.reshape(-1), bb]
        kp = cp
    return torch.cat(blocks)


ACCEPTED = {
    "pointnet2 SharedMLP": lambda: __import__("geot_amd.pointnet2.pytorch_utils", fromlist=["SharedMLP"]).SharedMLP([6, 64, 64, 128], bn=True),
    "affine=False": lambda: nn.Sequential(_stage(nn.Conv2d(6, 33, 1, bias=False), _bn(33, affine=False), nn.ReLU()),
                                          _stage(nn.Conv2d(33, 64, 1), _bn(64, affine=False))),
    "conv bias + bn": lambda: nn.Sequential(_stage(nn.Conv2d(9, 31, 1), _bn(31), nn.ReLU()), _stage(nn.Conv2d(31, 129, 1), _bn(129))),
    "no bn, bias, last without relu": lambda: nn.Sequential(_stage(nn.Conv2d(5, 100, 1), nn.ReLU()), _stage(nn.Conv2d(100, 1, 1))),
    "interior without relu": lambda: nn.Sequential(_stage(nn.Conv2d(3, 64, 1, bias=False), _bn(64)), _stage(nn.Conv2d(64, 64, 1), nn.ReLU())),
    "padding valid": lambda: nn.Sequential(_stage(nn.Conv2d(4, 32, 1, padding="valid"), _bn(32), nn.ReLU())),
}


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_pack_params_folds_like_fp64(name):
    from geot_amd.sa_fused import _stages, pack_params
    torch.manual_seed(5)
    mlp = ACCEPTED[name]()
    for m in mlp.modules():
        if isinstance(m, nn.BatchNorm2d) and m.running_mean is not None:
            with torch.no_grad():
                m.running_mean.uniform_(-0.5, 0.5)
                m.running_var.uniform_(0.5, 2.0)
    mlp.eval()
    st = _stages(mlp)
    assert st is not None
    params, widths, relu_mask, c_feat = pack_params(mlp)
    assert widths == [c.out_channels for c, _, _ in st] and c_feat == st[0][0].in_channels - 3
    assert relu_mask == sum(int(r) << l for l, (_, _, r) in enumerate(st))
    ref = _fold64(st)
    assert params.dtype == torch.float32 and params.shape == ref.shape
    # fp32 fold: s = gamma / sqrt(var + eps) (3 roundings), W' (1 more), b' (3 more) -- 8 u of the terms' magnitudes
    mag = _fold64_abs(st)
    assert ((params.double() - ref).abs() <= 8 * 2.0 ** -24 * mag).all()
    assert (params[ref == 0] == 0).all()                  # padding stays exactly 0


def _fold64_abs(st):
    """the magnitudes of the fold's terms, laid out like _fold64: |W s| and |b - mean| |s| + |beta|"""
    blocks = []
    kp = (st[0][0].in_channels + 1) & ~1
    for conv, bn, _ in st:
        w = conv.weight.double().reshape(conv.out_channels, -1).abs()
        b = conv.bias.double().abs() if conv.bias is not None else torch.zeros(conv.out_channels, dtype=torch.float64)
        if bn is not None:
            g = bn.weight.double() if bn.weight is not None else torch.ones_like(b)
            beta = bn.bias.double().abs() if bn.bias is not None else torch.zeros_like(b)
            s = (g / torch.sqrt(bn.running_var.double() + bn.eps)).abs()
            bm = ((conv.bias.double() if conv.bias is not None else torch.zeros_like(b)) - bn.running_mean.double()).abs()
            w, b = w * s[:, None], bm * s + beta
        cp = pad_cols(conv.out_channels)
        wt = torch.zeros(kp, cp, dtype=torch.float64)
        wt[:conv.in_channels, :conv.out_channels] = w.t()
        bb = torch.zeros(cp, dtype=torch.float64)
        bb[:conv.out_channels] = b
        blocks += [wt.reshape(-1), bb]
        kp = cp
    return torch.cat(blocks)


def test_pack_params_cache_follows_eps_and_structure():
    from geot_amd.sa_fused import pack_params
    torch.manual_seed(2)
    mlp = nn.Sequential(_stage(nn.Conv2d(6, 64, 1, bias=False), _bn(64), nn.ReLU())).eval()
    p1 = pack_params(mlp)[0].clone()
    assert pack_params(mlp)[0] is pack_params(mlp)[0]              # cached while nothing changes
    mlp[0][1].eps = 0.5
    p2 = pack_params(mlp)[0]
    assert not torch.equal(p1, p2)
    assert torch.allclose(p2.double(), _fold64([(mlp[0][0], mlp[0][1], True)]), rtol=1e-6, atol=1e-7)
    conv, bn = mlp[0][0], mlp[0][1]
    mlp[0] = _stage(conv, bn)              # the same tensors, the ReLU gone
    p3, _, relu_mask, _ = pack_params(mlp)
    assert relu_mask == 0 and torch.equal(p3, p2)
    mlp[0] = _stage(conv, nn.ReLU())       # the same conv, the norm gone
    p4, _, relu_mask, _ = pack_params(mlp)
    assert relu_mask == 1 and torch.equal(p4[:6 * 64].view(6, 64), conv.weight.detach().reshape(64, 6).t())
    mlp[0] = _stage(conv, nn.Identity(), nn.ReLU())     # now refused outright
    with pytest.raises(Exception):
        pack_params(mlp)
