"""The fused SetAbstraction kernel (csrc/sa_mlp.hip: geot_sa_group_mlp_max through geot_amd/sa_fused.py) against an fp64
reference of the unfolded SharedMLP, on every branch of its launch plan.

Every case first asserts its plan from geot_sa_plan at this device's CU count (a retune fails loudly), then compares the
kernel with tests/_sa_ref.reference within the propagated error bound, elementwise.  Switch points come from the query.
Cases cover both variants at every waves count, 4 / 2 / 1 groups per tile and 2 / 3 / 4 tiles per group, the
register-pooled path at 1 / 2 / 4 stores per group and each reason for the LDS-pooled one, runs of 8 and of 1 (natural,
from npoint % 8 and from a misaligned output), persistent grids whose last workgroups get nothing, one to four layers of
widths from 1 to 256, c_feat 0 (NULL features) to 61, no ReLU on the last or an interior layer, conv bias with and
without BatchNorm, xyz_scale != 1, clouds far from the origin, repeated indices and empty inputs.  NaN and +-inf inputs
must come out where the composed module has them; the loop forms must agree to the bit.  At module level
PointnetSAModuleVotes and openpoints' ConvPool take the kernel where they should and the composed path where the stack
cannot be folded."""
import pytest
import torch
import torch.nn as nn

from _sa_ref import BENCH_SA, SaLaunches, assert_within, composed, make_mlp, plan, reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from geot_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _env(monkeypatch, fast=None, run=None):
    for k in ("GEOT_SA_FAST", "GEOT_SA_RUN"):
        monkeypatch.delenv(k, raising=False)
    if fast is not None:
        monkeypatch.setenv("GEOT_SA_FAST", str(fast))
    if run is not None:
        monkeypatch.setenv("GEOT_SA_RUN", str(run))


def cloud(b, n, npoint, nsample, c_feat, seed, offset=0.0, spread=1.0):
    """random points (b, n, 3) around `offset`, centres = points near the first npoint, features, idx (b, npoint, nsample)
    int32 with repeats (the ball query pads with its first hit)"""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(b, n, 3, generator=g) * spread + offset
    new_xyz = xyz[:, :npoint] + torch.randn(b, npoint, 3, generator=g) * 0.01 * spread if npoint <= n else \
        torch.rand(b, npoint, 3, generator=g) * spread + offset
    feats = torch.randn(b, c_feat, n, generator=g)
    idx = torch.randint(0, n, (b, npoint, nsample), generator=g, dtype=torch.int32)
    if npoint and nsample > 2:
        cut = torch.randint(1, nsample, (b, npoint, 1), generator=g)
        pad = torch.arange(nsample).view(1, 1, -1) >= cut
        idx = torch.where(pad, idx[..., :1], idx)              # ball-query padding: the first index repeated
    return xyz.to(DEV), new_xyz.contiguous().to(DEV), feats.to(DEV), idx.to(DEV)


def launch(xyz, new_xyz, feats, idx, mlp, xyz_scale=1.0, out_offset=0):
    """geot_sa_group_mlp_max straight through the ABI: features NULL when c_feat == 0, the output at out_offset floats"""
    from geot_amd.ext._common import call, ptr
    from geot_amd.sa_fused import pack_params
    import ctypes
    params, widths, relu_mask, c_feat = pack_params(mlp)
    b, n, _ = xyz.shape
    npoint, nsample = idx.shape[1], idx.shape[2]
    buf = torch.full((out_offset + b * widths[-1] * npoint,), 12345.0, device=DEV)
    out = buf[out_offset:].view(b, widths[-1], npoint)
    warr = (ctypes.c_int * len(widths))(*widths)
    call("geot_sa_group_mlp_max", torch.device(DEV), b, n, npoint, nsample, c_feat, ptr(xyz), ptr(new_xyz),
         ptr(feats) if c_feat else None, ptr(idx), float(xyz_scale), len(widths), warr, relu_mask, ptr(params), ptr(out))
    torch.cuda.synchronize()
    return out


def check_plan(lib, cus, b, npoint, nsample, c_feat, widths, want, aligned=True):
    p = plan(lib, b, npoint, nsample, c_feat, widths, cus, aligned)
    assert p is not None, "refused"
    got = {k: p[k] for k in want}
    assert got == want, (got, want)
    return p


def empty_ranges(p, b, npoint):
    """some workgroup of the persistent grid owns no unit / run"""
    total = b * npoint // p["run_len"] if p["fast_np"] else p["nunits"]
    chunk = -(-total // p["blocks"])
    return (p["blocks"] - 1) * chunk >= total


def bits_equal(a, b):
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32))


# (id, c_feat, widths, nsample, b, npoint, n, kwargs of make_mlp, want plan fields)
CASES = [
    ("bench-like 12 waves fast 2", 3, (64, 64, 128), 32, 1, 3000, 8000, {}, dict(wide=0, waves=12, gpt=1, tpg=1, fast_np=2)),
    ("lean 8 waves fast 2", 3, (64, 64, 64, 128), 32, 2, 1001, 4000, {}, dict(wide=0, waves=8, fast_np=2)),
    ("lean 8 waves c_feat 61 generic", 61, (64, 64, 128), 32, 2, 777, 3000, {}, dict(wide=0, waves=8, fast_np=0)),
    ("lean 4 waves fast 1", 3, (128, 64), 32, 3, 333, 2000, {}, dict(wide=0, waves=4, fast_np=1)),
    ("wide 8 waves fast 4", 3, (64, 256), 32, 2, 999, 3000, {}, dict(wide=1, waves=8, fast_np=4)),
    ("wide 4 waves gpt 4", 3, (64, 256), 8, 3, 1001, 3000, {}, dict(wide=1, waves=4, gpt=4, fast_np=0)),
    ("wide 4 waves 4 layers fast 4", 3, (64, 64, 64, 256), 32, 1, 1111, 3000, {}, dict(wide=1, waves=4, fast_np=4)),
    ("gpt 2", 5, (32, 100), 16, 3, 1001, 3000, {}, dict(gpt=2, tpg=1, fast_np=0)),
    ("gpt 4 width 1", 1, (33, 1), 8, 2, 999, 2000, {}, dict(gpt=4, fast_np=0)),
    ("tpg 2 generic", 3, (64, 64, 128), 64, 2, 517, 3000, {}, dict(gpt=1, tpg=2, fast_np=0, waves=12)),
    ("tpg 3 width 129", 8, (64, 129), 96, 1, 301, 2000, {}, dict(wide=1, tpg=3, fast_np=0)),
    ("tpg 4", 9, (31, 33, 32, 100), 128, 1, 257, 2000, {}, dict(tpg=4, fast_np=0)),
    ("generic: c_feat 9", 9, (64, 128), 32, 2, 800, 3000, {}, dict(fast_np=0)),
    ("generic: last width padded", 3, (64, 100), 32, 2, 800, 3000, {}, dict(fast_np=0)),
    ("generic: last width 32", 3, (128, 32), 32, 2, 800, 3000, {}, dict(fast_np=0)),
    ("widths 1 layer 256", 8, (256,), 32, 2, 640, 3000, {}, dict(wide=1, fast_np=4)),
    ("widths 31 33 32 100 gpt 2", 1, (31, 33, 32, 100), 16, 2, 555, 3000, {}, dict(gpt=2)),
    ("widths 33 200 c_feat 0", 0, (33, 200), 16, 2, 444, 2000, {}, dict(wide=1, gpt=2)),
    ("widths 128 128 lean 4 waves", 3, (128, 128), 32, 2, 700, 3000, {}, dict(wide=0, waves=4, fast_np=2)),
    ("no relu last, all negative", 3, (64, 128), 32, 2, 600, 3000, dict(relu=[True, False], last_bias=-50.0), dict(fast_np=2)),
    ("no relu interior", 8, (64, 64, 64), 16, 2, 600, 3000, dict(relu=[True, False, True]), dict(gpt=2)),
    ("conv bias and bn", 5, (64, 128), 32, 2, 600, 3000, dict(bias=True), dict(fast_np=2)),
    ("conv bias no bn", 5, (100, 64), 8, 2, 600, 3000, dict(bn=False, bias=True), dict(gpt=4)),
    ("no bias no bn", 3, (64, 64), 32, 2, 600, 3000, dict(bn=False, bias=False), dict(fast_np=1)),
    ("bn affine=False", 3, (33, 128), 32, 2, 600, 3000, dict(affine=False), dict(fast_np=2)),
]


def _mlp_for(c_feat, widths, kw, seed):
    kw = dict(kw)
    last_bias = kw.pop("last_bias", None)
    mlp = make_mlp(3 + c_feat, widths, seed=seed, **kw)
    if last_bias is not None:           # every output of the last (ReLU-free) layer below 0
        conv = mlp[-1][0]
        with torch.no_grad():
            if conv.bias is None:
                conv.bias = nn.Parameter(torch.zeros(conv.out_channels, device=DEV))
            conv.bias.fill_(last_bias)
            if len(mlp[-1]) > 1 and isinstance(mlp[-1][1], nn.BatchNorm2d):
                mlp[-1][1].weight.abs_()
    return mlp


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_case_against_fp64(case, lib, cus, monkeypatch):
    name, c_feat, widths, nsample, b, npoint, n, kw, want = case
    _env(monkeypatch)
    p = check_plan(lib, cus, b, npoint, nsample, c_feat, widths, want)
    xyz, new_xyz, feats, idx = cloud(b, n, npoint, nsample, c_feat, seed=sum(map(ord, name)) + nsample)
    mlp = _mlp_for(c_feat, widths, kw, seed=sum(map(ord, name)))
    from geot_amd.sa_fused import fused_group_mlp_max
    got = fused_group_mlp_max(xyz, new_xyz, feats, idx, mlp)
    ref, bound = reference(xyz, new_xyz, feats, idx, mlp)
    assert_within(got, ref, bound, name)
    if "last_bias" in kw:
        assert (ref < 0).all()
    # the same through the ABI with the output 4 bytes off 16-byte alignment (no runs of 8 there)
    if p["fast_np"] and npoint % 8 == 0:
        check_plan(lib, cus, b, npoint, nsample, c_feat, widths, dict(run_len=1), aligned=False)
    got1 = launch(xyz, new_xyz, feats, idx, mlp, out_offset=1)
    assert bits_equal(got1, got), name


def test_bound_catches_a_dropped_term(lib, cus):
    """the reference and its bound are tight enough to see one input channel's contribution go missing"""
    xyz, new_xyz, feats, idx = cloud(2, 2000, 500, 32, 3, seed=1)
    mlp = make_mlp(6, (64, 64, 128), seed=3)
    from geot_amd.sa_fused import fused_group_mlp_max
    got = fused_group_mlp_max(xyz, new_xyz, feats, idx, mlp)
    bad = feats.clone()
    bad[:, 2] = 0                          # as if the kernel dropped the k-pair of its last feature channel
    ref, bound = reference(xyz, new_xyz, bad, idx, mlp)
    with pytest.raises(AssertionError):
        assert_within(got, ref, bound)
    ref, bound = reference(xyz, new_xyz, feats, idx, mlp)
    assert_within(got, ref, bound)
    assert float(bound.median()) < 1e-3 * float(ref.abs().median())       # and still a tight bound


def test_c_feat_zero_null_features(lib, cus):
    xyz, new_xyz, _, idx = cloud(2, 2000, 700, 32, 0, seed=4)
    mlp = make_mlp(3, (64, 128), seed=4)
    check_plan(lib, cus, 2, 700, 32, 0, (64, 128), dict(fast_np=2))
    got = launch(xyz, new_xyz, None, idx, mlp)
    ref, bound = reference(xyz, new_xyz, None, idx, mlp)
    assert_within(got, ref, bound, "c_feat 0")
    mlp16 = make_mlp(3, (32, 64), seed=5)
    check_plan(lib, cus, 2, 700, 16, 0, (32, 64), dict(gpt=2))
    idx16 = idx[..., :16].contiguous()
    assert_within(launch(xyz, new_xyz, None, idx16, mlp16), *reference(xyz, new_xyz, None, idx16, mlp16), what="c_feat 0 ns 16")


@pytest.mark.parametrize("scale,offset", [(1.0 / 0.15, 0.0), (1.0, 1000.0), (1.0 / 0.07, -3000.0)])
def test_xyz_scale_and_far_clouds(scale, offset, lib, cus):
    """(p - q) * xyz_scale: the reference forms it the kernel's way in fp32 (so a far cloud's cancellation is the input's,
    not the kernel's error)"""
    xyz, new_xyz, feats, idx = cloud(2, 3000, 800, 32, 3, seed=6, offset=offset, spread=0.3)
    mlp = make_mlp(6, (64, 64, 128), seed=6)
    check_plan(lib, cus, 2, 800, 32, 3, (64, 64, 128), dict(fast_np=2))
    from geot_amd.sa_fused import fused_group_mlp_max
    got = fused_group_mlp_max(xyz, new_xyz, feats, idx, mlp, xyz_scale=scale)
    assert_within(got, *reference(xyz, new_xyz, feats, idx, mlp, scale), what="scale %g offset %g" % (scale, offset))


def test_one_point_groups_and_repeats(lib, cus):
    """groups whose indices all point at one point (pooled = that row), and heavy repetition"""
    xyz, new_xyz, feats, idx = cloud(2, 500, 640, 32, 3, seed=8)
    idx[:, ::3] = idx[:, ::3, :1]
    idx[:, 1::7] = 17
    mlp = make_mlp(6, (64, 128), seed=8)
    from geot_amd.sa_fused import fused_group_mlp_max
    got = fused_group_mlp_max(xyz, new_xyz, feats, idx.contiguous(), mlp)
    ref, bound = reference(xyz, new_xyz, feats, idx.contiguous(), mlp)
    assert_within(got, ref, bound, "repeats")
    # a group of one point repeated pools that point's row: the same as a group of nsample 1
    one, one_bound = reference(xyz, new_xyz[:, ::3].contiguous(), feats, idx[:, ::3, :1].contiguous(), mlp)
    assert_within(got[:, :, ::3], one, one_bound, "one-point groups")


def test_runs_of_eight_natural_and_the_other_forms(lib, cus, monkeypatch):
    """run_len 8 where the plan chooses it (b * npoint >= 16 blocks * waves), run_len 1 just off it from npoint % 8, and
    the three loop forms bit-identical"""
    c_feat, widths = 3, (128, 64)                            # the 4-wave lean plan: the smallest grid to fill
    waves = plan(lib, 1, 8, 32, c_feat, widths, cus)["waves"]
    b = 2
    npoint = -(-16 * cus * waves // b // 8) * 8
    p = check_plan(lib, cus, b, npoint, 32, c_feat, widths, dict(wide=0, waves=4, fast_np=1, run_len=8))
    assert p["blocks"] == cus
    xyz, new_xyz, feats, idx = cloud(b, 20000, npoint, 32, c_feat, seed=9)
    mlp = make_mlp(3 + c_feat, widths, seed=9)
    from geot_amd.sa_fused import fused_group_mlp_max
    _env(monkeypatch)
    got8 = fused_group_mlp_max(xyz, new_xyz, feats, idx, mlp)
    ref, bound = reference(xyz, new_xyz, feats, idx, mlp)
    assert_within(got8, ref, bound, "run 8")
    got_mis = launch(xyz, new_xyz, feats, idx, mlp, out_offset=1)           # plan: run 1 at a misaligned output
    check_plan(lib, cus, b, npoint, 32, c_feat, widths, dict(run_len=1), aligned=False)
    assert bits_equal(got_mis, got8)
    forms = {}
    for name, fast, run in (("generic", 0, None), ("run1", None, 1), ("run8", None, 8)):
        _env(monkeypatch, fast, run)
        forms[name] = fused_group_mlp_max(xyz, new_xyz, feats, idx, mlp)
    _env(monkeypatch)
    assert bits_equal(forms["generic"], got8) and bits_equal(forms["run1"], got8) and bits_equal(forms["run8"], got8)
    # npoint % 8 != 0 at the same size: run 1
    np2 = npoint + 3
    check_plan(lib, cus, b, np2, 32, c_feat, widths, dict(fast_np=1, run_len=1))
    xyz2, new2, feats2, idx2 = cloud(b, 20000, np2, 32, c_feat, seed=10)
    assert_within(fused_group_mlp_max(xyz2, new2, feats2, idx2, mlp), *reference(xyz2, new2, feats2, idx2, mlp), what="run 1")


@pytest.mark.parametrize("fast", [True, False])
def test_persistent_grid_with_empty_workgroups(fast, lib, cus, monkeypatch):
    """units just past blocks * waves: the grid is capped at the CU count and its last workgroups own nothing"""
    c_feat, widths = (3, (64, 64, 128)) if fast else (9, (64, 64, 128))
    waves = plan(lib, 1, 8, 32, c_feat, widths, cus)["waves"]
    npoint = cus * waves + 1
    p = check_plan(lib, cus, 1, npoint, 32, c_feat, widths, dict(fast_np=2 if fast else 0, run_len=1))
    assert p["blocks"] == cus and empty_ranges(p, 1, npoint)
    xyz, new_xyz, feats, idx = cloud(1, 8000, npoint, 32, c_feat, seed=11)
    mlp = make_mlp(3 + c_feat, widths, seed=11)
    from geot_amd.sa_fused import fused_group_mlp_max
    _env(monkeypatch)
    assert_within(fused_group_mlp_max(xyz, new_xyz, feats, idx, mlp), *reference(xyz, new_xyz, feats, idx, mlp), what="empty ranges")


def test_empty_inputs(lib, cus):
    from geot_amd.sa_fused import fused_group_mlp_max
    mlp = make_mlp(6, (64, 128), seed=12)
    for b, npoint in ((0, 100), (2, 0)):
        xyz = torch.rand(b, 50, 3, device=DEV)
        p = plan(lib, b, npoint, 32, 3, (64, 128), cus)
        assert p is not None and p["blocks"] == 0
        out = fused_group_mlp_max(xyz, torch.rand(b, npoint, 3, device=DEV), torch.randn(b, 3, 50, device=DEV),
                                  torch.zeros(b, npoint, 32, dtype=torch.int32, device=DEV), mlp)
        torch.cuda.synchronize()
        assert out.shape == (b, 128, npoint)


# ---- NaN and infinities -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nsample,widths,relu_last", [(32, (64, 128), True), (32, (64, 64, 128), False), (16, (33, 64), True),
                                                      (64, (64, 200), True), (8, (64, 256), False)])
def test_nan_and_inf_masks_match_the_composed_module(nsample, widths, relu_last, lib, cus, monkeypatch):
    """a NaN in one feature of one neighbour comes out NaN in exactly the (group, column) entries the composed module has
    NaN; +-inf features give its NaNs and infinities too.  ReLU and max propagate NaN (fmaxf would drop it), and the
    padding columns stay 0 (0 * inf would be NaN)."""
    b, n, npoint, c_feat = 2, 600, 256, 3
    assert plan(lib, b, npoint, nsample, c_feat, widths, cus) is not None
    xyz, new_xyz, feats, idx = cloud(b, n, npoint, nsample, c_feat, seed=13)
    relu = [True] * (len(widths) - 1) + [relu_last]
    mlp = make_mlp(3 + c_feat, widths, relu=relu, seed=13)
    feats[0, 1, 5] = float("nan")
    feats[1, 0, 7] = float("inf")
    feats[1, 2, 9] = float("-inf")
    feats[0, 2, 11] = float("inf")
    cpu = lambda t: t.cpu()
    want = composed(cpu(xyz), cpu(new_xyz), cpu(feats), cpu(idx), mlp.cpu()).to(DEV)
    mlp = mlp.to(DEV)
    touched = torch.zeros(b, npoint, dtype=torch.bool, device=DEV)
    for bi, j in ((0, 5), (1, 7), (1, 9), (0, 11)):
        touched[bi] |= (idx[bi] == j).any(-1)
    assert touched.any() and not touched.all()
    from geot_amd.sa_fused import fused_group_mlp_max
    outs = []
    forms = [(None, None)] + ([(0, None), (None, 1), (None, 8)] if nsample == 32 else [])
    for fast, run in forms:
        _env(monkeypatch, fast, run)
        outs.append(fused_group_mlp_max(xyz, new_xyz, feats, idx, mlp))
    _env(monkeypatch)
    got = outs[0]
    assert torch.isnan(got).any()
    assert torch.equal(torch.isnan(got), torch.isnan(want)), (int(torch.isnan(got).sum()), int(torch.isnan(want).sum()))
    inf = torch.isinf(want)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], want[inf])
    assert not (torch.isnan(got) | torch.isinf(got)).permute(0, 2, 1)[~touched].any()    # other groups stay finite
    ref, bound = reference(xyz, new_xyz, feats, idx, mlp)
    assert_within(got, ref, bound, "nan/inf")
    for o in outs[1:]:
        assert bits_equal(o, got)


# ---- module level ----------------------------------------------------------------------------------------------------

def _votes(mlp_spec, nsample, normalize, npoint=500):
    from geot_amd.pointnet2.pointnet2_modules import PointnetSAModuleVotes
    sa = PointnetSAModuleVotes(mlp=list(mlp_spec), npoint=npoint, radius=0.15, nsample=nsample, normalize_xyz=normalize).to(DEV)
    with torch.no_grad():
        for m in sa.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.uniform_(-0.3, 0.3)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(-1.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
    return sa.eval()


def _module_reference(sa, xyz, feats, new_xyz):
    from geot_amd.pointnet2 import pointnet2_utils as pu
    idx = pu.ball_query(sa.radius, sa.nsample, xyz, new_xyz)
    return reference(xyz, new_xyz, feats, idx, sa.mlp_module, 1.0 / sa.radius if sa.normalize_xyz else 1.0)


@pytest.mark.parametrize("mlp_spec,nsample,normalize", [([3, 64, 64, 128], 32, False), ([5, 32, 48], 16, True),
                                                        ([13, 64, 40, 64, 200], 32, False), ([3, 64, 128], 64, True)])
def test_votes_module_fused_eval_against_fp64(mlp_spec, nsample, normalize, monkeypatch):
    from geot_amd.synth import make_batch
    torch.manual_seed(3)
    xyz = torch.from_numpy(make_batch(2, 3000, start_index=5)[0]).to(DEV)
    feats = torch.randn(2, mlp_spec[0], 3000, device=DEV)
    sa = _votes(mlp_spec, nsample, normalize)
    rec = SaLaunches(monkeypatch)
    with torch.no_grad():
        new_xyz, got, _ = sa(xyz, feats)
    assert rec.take() == ["geot_sa_group_mlp_max"]
    assert_within(got, *_module_reference(sa, xyz, feats, new_xyz), what=str(mlp_spec))


def test_convpool_fused_eval_against_fp64(monkeypatch):
    from geot_amd.openpoints.models.layers.local_aggregation import ConvPool
    from geot_amd.openpoints.models.layers.group import ball_query
    from geot_amd.synth import make_batch
    torch.manual_seed(4)
    xyz = torch.from_numpy(make_batch(2, 2048, start_index=7)[0]).to(DEV)
    feats = torch.randn(2, 6, 2048, device=DEV)
    query = xyz[:, :512].contiguous()
    for normalize_dp in (False, True):
        cp = ConvPool([6, 32, 64], conv_args={}, norm_args={'norm': 'bn'}, act_args={'act': 'relu'},
                      group_args={'NAME': 'ballquery', 'radius': 0.15, 'nsample': 32, 'normalize_dp': normalize_dp},
                      feature_type='dp_fj', reduction='max').to(DEV)
        with torch.no_grad():
            for m in cp.modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.running_mean.uniform_(-0.3, 0.3)
                    m.running_var.uniform_(0.5, 1.5)
                    m.weight.uniform_(-1.5, 1.5)
                    m.bias.uniform_(-0.2, 0.2)
        cp.eval()
        rec = SaLaunches(monkeypatch)
        with torch.no_grad():
            got = cp(query, xyz, feats)
        assert rec.take() == ["geot_sa_group_mlp_max"]
        idx = ball_query(0.15, 32, xyz, query)
        assert_within(got, *reference(xyz, query, feats, idx, cp.convs, 1.0 / 0.15 if normalize_dp else 1.0), what="ConvPool")


def _bn_plain(c, **kw):
    m = nn.BatchNorm2d(c, **kw)
    with torch.no_grad():
        if m.running_mean is not None:
            m.running_mean.uniform_(-0.3, 0.3)
            m.running_var.uniform_(0.5, 1.5)
    return m


REFUSED = {
    "relu before bn": lambda: nn.Sequential(nn.Sequential(nn.Conv2d(6, 32, 1, bias=False), nn.ReLU(), _bn_plain(32)),
                                            nn.Sequential(nn.Conv2d(32, 64, 1, bias=False), _bn_plain(64), nn.ReLU())),
    "bn twice": lambda: nn.Sequential(nn.Sequential(nn.Conv2d(6, 32, 1, bias=False), _bn_plain(32), _bn_plain(32), nn.ReLU())),
    "no running stats": lambda: nn.Sequential(nn.Sequential(nn.Conv2d(6, 64, 1, bias=False),
                                                            _bn_plain(64, track_running_stats=False), nn.ReLU())),
    "leaky relu": lambda: nn.Sequential(nn.Sequential(nn.Conv2d(6, 64, 1, bias=False), _bn_plain(64), nn.LeakyReLU(0.1))),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_votes_module_refused_stacks_take_the_composed_path(name, monkeypatch):
    """stacks the fold cannot represent: no fused launch, and the output is the composed module's"""
    from geot_amd.synth import make_batch
    torch.manual_seed(5)
    xyz = torch.from_numpy(make_batch(2, 2000, start_index=3)[0]).to(DEV)
    feats = torch.randn(2, 3, 2000, device=DEV)
    sa = _votes([3, 64], 32, False, npoint=300)
    sa.mlp_module = REFUSED[name]().to(DEV).eval()
    rec = SaLaunches(monkeypatch)
    with torch.no_grad():
        _, got, _ = sa(xyz, feats)
        assert "geot_sa_group_mlp_max" not in rec.take()
        sa.fused_eval = False
        _, want, _ = sa(xyz, feats)
    assert torch.allclose(got, want, rtol=1e-6, atol=1e-7)       # the same composed ops (library GEMMs: not pinned to the bit)


def test_votes_module_affine_false_bn_is_folded(monkeypatch):
    from geot_amd.synth import make_batch
    torch.manual_seed(6)
    xyz = torch.from_numpy(make_batch(2, 2000, start_index=3)[0]).to(DEV)
    feats = torch.randn(2, 3, 2000, device=DEV)
    sa = _votes([3, 64], 32, False, npoint=300)
    sa.mlp_module = make_mlp(6, (64, 128), affine=False, seed=6)
    rec = SaLaunches(monkeypatch)
    with torch.no_grad():
        new_xyz, got, _ = sa(xyz, feats)
    assert rec.take() == ["geot_sa_group_mlp_max"]
    assert_within(got, *_module_reference(sa, xyz, feats, new_xyz), what="affine=False")


def test_bench_shape_plan_pinned(lib, cus, monkeypatch):
    """bench.py --workload sa (configs[1]): the module's call is BENCH_SA, with the plan the plan test pins"""
    import ctypes
    from geot_amd import sa_fused
    from geot_amd.pointnet2.pointnet2_modules import PointnetSAModuleVotes
    s = BENCH_SA
    seen = []
    real = sa_fused.call

    def rec(name, dev, *args):
        b, n, npoint, nsample, c_feat = args[:5]
        nl, warr = args[10], args[11]
        seen.append((b, n, npoint, nsample, c_feat, tuple(warr[i] for i in range(nl)), args[-1] % 16 == 0))
        return real(name, dev, *args)
    monkeypatch.setattr(sa_fused, "call", rec)
    xyz = torch.rand(s["b"], s["n"], 3, device=DEV)
    feats = torch.randn(s["b"], s["c_feat"], s["n"], device=DEV)
    sa = PointnetSAModuleVotes(mlp=[s["c_feat"], *s["widths"]], npoint=s["npoint"], radius=0.1, nsample=s["nsample"],
                               use_xyz=True).to(DEV).eval()
    with torch.no_grad():
        sa(xyz, feats)
    assert seen == [(s["b"], s["n"], s["npoint"], s["nsample"], s["c_feat"], s["widths"], True)]
    p = check_plan(lib, cus, s["b"], s["npoint"], s["nsample"], s["c_feat"], s["widths"], dict(wide=0, waves=12, fast_np=2))
    if cus == 256:
        assert p["run_len"] == 1 and p["blocks"] == 256


def test_every_branch_reached(lib, cus):
    """the shapes above, planned at this device's CU count, reach every plan branch"""
    shapes = [(b, npoint, ns, cf, ws) for _, cf, ws, ns, b, npoint, _, _, _ in CASES]
    waves = plan(lib, 1, 8, 32, 3, (128, 64), cus)["waves"]
    shapes.append((2, -(-16 * cus * waves // 2 // 8) * 8, 32, 3, (128, 64)))          # test_runs_of_eight_...
    reached = {tuple(plan(lib, *sh, cus)[k] for k in ("wide", "waves", "gpt", "tpg", "fast_np", "run_len")) for sh in shapes}
    assert {(w, v) for w, v, *_ in reached} == {(0, 12), (0, 8), (0, 4), (1, 8), (1, 4)}
    assert {r[2] for r in reached} == {1, 2, 4} and {r[3] for r in reached} == {1, 2, 3, 4}
    assert {r[4] for r in reached} == {0, 1, 2, 4} and {r[5] for r in reached} == {1, 8}
