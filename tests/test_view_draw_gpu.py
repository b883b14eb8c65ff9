"""GPU suite of geot_view_draw (geot_amd/csrc/view_draw.hip; geot_amd/openpoints/dataset/view_draw.py) and of the batchers'
DeviceDraws(views=True) mode, against the numpy float32 restatement of the contract (tests/_view_draw_ref.py).  The contract
is bit-reproducible: every drawn scalar, noise element and mask element is compared for EQUALITY OF BITS (the job table as
int32 words, floats through their int32 view), and so is every output of the views built from them -- there is no tolerance
anywhere in this file.  The expected views come from the unchanged host path (view_program_views / geot_fixmatch_views)
fed the restatement's parameters."""
import functools
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sample_draw_ref as sd  # noqa: E402
import _view_draw_ref as vr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEED = 0x5EEDC0DE1234567
INVALID = 1            # hipErrorInvalidValue

FM_KW = {"scale": [0.9, 1.1], "gravity_dim": 1, "scale_s": [0.8, 1.2], "shift_s": [0.2, 0.2, 0.2], "angle": [1, 1, 1]}
FM_LISTS = {"train": ["PointCloudScaling", "PointCloudCenterAndNormalize"], "train_w": ["PointCloudCenterAndNormalize"],
            "train_s": ["PointCloudScaling_s", "PointCloudCenterAndNormalize", "PointCloudRotation_s", "PointCloudTranslation_s"]}
# every drawing transform.  Order A: the colour drops come after x has left pos (STORE_X modes 1 and 2, masks folded into one
# row) and once before (ZERO / MASK ops on pos); order B: all of them before the first rebinding transform (STORE_X mode 0)
ALL_KW = {"upright_axis": "z", "mirror": [0.5, 0, 1], "angle": [1, 0.25, 0.1], "jitter_sigma_s": 0.01, "color_drop": 0.3,
          "gravity_dim": 1}
ALL_A = ["PointsToTensor", "PointCloudJitter_s", "ChromaticPerDropGPU", "RandomHorizontalFlip", "ChromaticDropGPU",
         "PointCloudScaleAndJitter", "PointCloudRotation", "ChromaticPerDropGPU", "PointCloudTranslation",
         "PointCloudScaleAndTranslate", "ChromaticPerDropGPU", "ChromaticDropGPU"]
ALL_B = ["PointCloudTranslation", "ChromaticDropGPU", "RandomHorizontalFlip", "ChromaticPerDropGPU", "PointCloudJitter_s",
         "PointCloudCenterAndNormalize", "PointCloudScaleAndTranslate", "PointCloudRotation", "PointCloudScaleAndJitter"]


@functools.lru_cache(maxsize=None)
def _program(name):
    from geot_amd.openpoints.dataset import DEFAULT_TRAIN, DEFAULT_TRAIN_KWARGS, ViewProgram
    if name == "default":
        return ViewProgram(DEFAULT_TRAIN, DEFAULT_TRAIN_KWARGS)
    if name in FM_LISTS:
        return ViewProgram(FM_LISTS[name], FM_KW)
    return ViewProgram({"all_a": ALL_A, "all_b": ALL_B}[name], ALL_KW)


def _bits(t):
    t = t.detach().cpu() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(got, want, what):
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError("%s: %d of %d words differ, first at %s" % (what, len(bad), got.numel(), bad[0].tolist()))


def _raw(rows, m, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((rows, m, 3), generator=g) * 2 - 1).to(DEV)


def _check_layout(name, m, n_jobs, base, raw_seed=5):
    """The draws of n_jobs jobs of one list (slots 0.., views cycling 0, 1, 2) against the restatement: table, noise,
    masks, then the views against the host path on the restatement's parameters -> the parameters, for coverage checks."""
    from geot_amd.openpoints.dataset import DrawLayout, pack_fixed_jobs, view_program_draw, view_program_views, view_program_views_drawn
    prog = _program(name)
    views, slots = [j % 3 for j in range(n_jobs)], list(range(n_jobs))
    rows = [(j * 5) % n_jobs for j in range(n_jobs)]                      # the source rows, permuted
    layout = DrawLayout([(rows[j], j, prog) for j in range(n_jobs)], n_jobs, n_jobs, m, DEV, views, slots)
    drawn = view_program_draw(layout, SEED, base)
    params = [vr.draw(prog, m, SEED, base + slots[j], views[j]) for j in range(n_jobs)]
    jobs = [(rows[j], j, prog, params[j]) for j in range(n_jobs)]
    table, plans, noise, masks = pack_fixed_jobs(jobs, n_jobs, n_jobs, m, views, slots)
    assert np.array_equal(plans, layout.plans)
    _same_bits(drawn["table"], table, "%s m=%d: job table" % (name, m))
    _same_bits(drawn["noise"], noise, "%s m=%d: noise" % (name, m))
    _same_bits(drawn["mask"], masks, "%s m=%d: masks" % (name, m))
    raw = _raw(n_jobs, m, raw_seed)
    got, want = view_program_views_drawn(raw, layout, drawn), view_program_views(raw, jobs, n_jobs)
    for key in ("pos", "x", "heights", "view_center", "view_scale"):
        if want[key] is None:
            assert got[key] is None
        else:
            assert torch.equal(_bits(got[key]), _bits(want[key])), "%s m=%d: %s differs from the host path" % (name, m, key)
    return params, drawn


@pytest.mark.parametrize("m", [1, 5, 255, 256, 257, 1000])
@pytest.mark.parametrize("name", ["default", "train", "train_w", "train_s", "all_a", "all_b"])
def test_draws_and_views_equal_the_restatement(name, m):
    _check_layout(name, m, 7, 2 ** 32 - 3)            # the draw ids cross into the high counter word


def test_streaming_views_read_device_drawn_noise():
    """m = 24 577 > GEOT_VIEW_REG_POINTS: geot_view_program's streaming instantiation reads the noise rows drawn here."""
    params, drawn = _check_layout("default", 24577, 2, 11)
    noise = drawn["noise"].cpu().numpy()
    # sigma 0.001, clip 0.005 = 5 sigma: the clip bounds the rows but is rarely reached among 147 462 normals; the
    # standard error of their deviation is 0.001 / sqrt(2 * 147 462) = 1.8e-6, so 2 % is over ten of them
    assert noise.shape == (2, 24577, 3) and np.abs(noise).max() <= np.float32(0.005)
    assert 0.98e-3 < noise.std() < 1.02e-3


def test_every_branch_of_the_drawn_ops_is_seen():
    """Flips and drops taken and not taken, STORE_X in modes 0, 1 and 2, every rotation order: over 48 draw ids of both orders."""
    from geot_amd.openpoints.dataset import view_program as vp
    pa, _ = _check_layout("all_a", 5, 48, 100)
    pb, drawn_b = _check_layout("all_b", 5, 48, 2 ** 64 - 20)             # and the draw ids wrap at 2^64

    def mode(name, p):
        fixed = _program(name).compile_fixed(p, 5)
        return fixed["ops"][fixed["store_at"]][1] & 3
    modes = {mode("all_a", p) for p in pa} | {mode("all_b", p) for p in pb}
    assert {mode("all_b", p) for p in pb} == {0}
    assert modes == {0, 1, 2}
    assert {tuple(p[3]["flip"]) for p in pa} == {(), (0,), (1,), (0, 1)}
    assert {p[4]["drop"] for p in pa} == {p[11]["drop"] for p in pa} == {p[1]["drop"] for p in pb} == {False, True}
    kinds = drawn_b["table"].cpu().numpy()[:, 8 + 14 * 1]                 # order B's second op: ZERO, or SCALE when not drawn
    assert set(kinds.tolist()) == {vp.ZERO, vp.SCALE}


def test_same_seed_and_counter_give_equal_bits_whatever_the_process_drew_before():
    from geot_amd.openpoints.dataset import DrawLayout, view_program_draw
    prog = _program("all_a")
    layout = DrawLayout([(j, j, prog) for j in range(4)], 4, 4, 300, DEV, [0, 1, 2, 0], [0, 1, 1, 2])
    out = []
    for s in (1, 2):
        torch.manual_seed(s), np.random.seed(s), random.seed(s), torch.cuda.manual_seed(s)
        out.append(view_program_draw(layout, SEED, 7))
    for key in ("table", "noise", "mask"):
        _same_bits(out[0][key], out[1][key], key)
    # jobs 1 and 2 share slot 1's id as views 1 and 2: other values; another seed or base: other values
    noise = out[0]["noise"].cpu().numpy()
    assert not np.array_equal(noise[2], noise[4])
    assert not torch.equal(view_program_draw(layout, SEED + 1, 7)["noise"], out[0]["noise"])
    shifted = view_program_draw(layout, SEED, 8)
    assert not torch.equal(shifted["noise"], out[0]["noise"])
    # job 0 draws with base + its slot: ALL_A's first noise row is PointCloudJitter_s, the list's transform number 1
    _same_bits(shifted["noise"][0], vr.noise_rows(300, 0, 1, SEED, 8, 0.01, 0.05), "slot 0 of base 8")


def test_ctypes_and_the_compiled_binding_return_the_same_tensors():
    from geot_amd.ext import _common
    from geot_amd.openpoints.dataset import DrawLayout, view_program_draw
    prog = _program("all_b")
    layout = DrawLayout([(j, j, prog) for j in range(3)], 3, 3, 257, DEV)
    assert _common.dispatcher() is not None and hasattr(_common.dispatcher(), "geot_view_draw")
    saved, out = _common._dispatch, {}
    try:
        for name, disp in (("dispatcher", saved), ("ctypes", False)):
            _common._dispatch = disp
            out[name] = view_program_draw(layout, 2 ** 64 - 5, 2 ** 64 - 2)      # values past 2^63 cross both bindings
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(side):
                on_side = view_program_draw(layout, 2 ** 64 - 5, 2 ** 64 - 2)
            side.synchronize()
            for key in ("table", "noise", "mask"):
                _same_bits(on_side[key], out[name][key], key)
    finally:
        _common._dispatch = saved
    for key in ("table", "noise", "mask"):
        _same_bits(out["dispatcher"][key], out["ctypes"][key], key)


def test_bad_plans_are_refused_on_the_host_and_write_nothing_on_the_device():
    from geot_amd import _lib
    from geot_amd.openpoints.dataset import DrawLayout
    lib, prog, m = _lib.load(), _program("all_a"), 64
    layout = DrawLayout([(0, 0, prog), (1, 1, prog)], 2, 2, m, DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    table = torch.full((2, _lib.VIEW_PROGRAM_JOB_WORDS), -7, dtype=torch.int32, device=DEV)
    noise = torch.full((layout.n_noise, m, 3), -7.0, device=DEV)
    mask = torch.full((layout.n_mask, m), -7.0, device=DEV)

    def call(plans_host, plans_dev):
        return lib.geot_view_draw(2, m, layout.n_noise, layout.n_mask, layout.tmpl.ctypes.data, plans_host.ctypes.data,
                                  layout.tmpl_dev.data_ptr(), plans_dev.data_ptr(), SEED, 0, table.data_ptr(), noise.data_ptr(),
                                  mask.data_ptr(), stream)
    bad = layout.plans.copy()
    bad[1, 8 + 1] = 9                                  # job 1's first step, a NOISE step, names the template's last op, which is no jitter op
    assert call(bad, layout.plans_dev) == INVALID
    torch.cuda.synchronize()
    assert bool((table == -7).all()) and bool((noise == -7).all()) and bool((mask == -7).all())
    # the host copy is good, the device copy is not: the kernel's own test leaves job 1 unwritten and draws job 0
    bad_dev = torch.from_numpy(bad).to(DEV)
    assert call(layout.plans, bad_dev) == 0
    torch.cuda.synchronize()
    assert bool((table[1] == -7).all()) and bool((noise[2:] == -7).all()) and bool((mask[2:] == -7).all())
    assert int(table[0, 2]) == 10 and bool((noise[:2] != -7).all()) and bool((mask[:2] != -7).all())


# ------------------------------------------------------------------------------------------------ the batchers
BATCH_SIZES = (3000, 700, 1500, 1024)       # m = 1024: without replacement, with (700), and n == m
M_BATCH = 1024


def _scan_set(sizes, seed=0):
    from geot_amd.openpoints.dataset import DeviceScanSet
    rng = np.random.default_rng(seed)
    return DeviceScanSet([rng.standard_normal((n, 3)).astype(np.float32) for n in sizes],
                         [rng.integers(0, 17, n).astype(np.int32) for n in sizes], cls=[i % 2 for i in range(len(sizes))], device=DEV)


def _same_batch(a, b):
    assert set(a) == set(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.is_tensor(b[k]) and a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            assert torch.equal(_bits(a[k]), _bits(b[k])), k
        elif isinstance(a[k], list) and a[k] and torch.is_tensor(a[k][0]):
            assert all(torch.equal(x, y) for x, y in zip(a[k], b[k])), k
        elif k == "scans":
            assert a[k] is b[k]
        else:
            assert a[k] == b[k], k


def _host_states():
    return torch.get_rng_state(), np.random.get_state(), random.getstate()


def _states_equal(a, b):
    return (torch.equal(a[0], b[0]) and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1])
            and tuple(a[1][2:]) == tuple(b[1][2:]) and a[2] == b[2])


@pytest.fixture()
def no_host_draws(monkeypatch):
    """From here on any host draw of the batchers' is an error."""
    def refuse(*args, **kwargs):
        raise AssertionError("a host generator was used in the device-draw mode")

    def arm():
        for mod, name in ((np.random, "choice"), (np.random, "uniform"), (np.random, "shuffle"), (random, "random"),
                          (torch, "rand"), (torch, "randn_like")):
            monkeypatch.setattr(mod, name, refuse)
    yield arm


@pytest.mark.parametrize("stream", [False, True])
def test_supervised_batcher_draws_its_views_on_the_device(stream, no_host_draws):
    from geot_amd.openpoints.dataset import DeviceDraws, SupervisedBatcher, ViewDrawHandle
    scans = _scan_set(BATCH_SIZES, 3)
    host = SupervisedBatcher(scans, M_BATCH)
    idx, base = [3, 1, 0, 2, 1], 2 ** 32 - 2
    sizes = [BATCH_SIZES[i] for i in idx]
    rows, _ = sd.sample_draw_ref(sizes, M_BATCH, SEED, base)
    params = [vr.draw(host.program, M_BATCH, SEED, base + i, 0) for i in range(len(idx))]
    want = host.batch(idx, sel=rows, params=params, check=True)           # the unchanged host path on the restatement
    side = torch.cuda.Stream() if stream else None
    ctor = SupervisedBatcher(scans, M_BATCH, stream=side, draws=DeviceDraws(SEED, base, views=True))
    plain = SupervisedBatcher(scans, M_BATCH, stream=side)
    no_host_draws()
    out = []
    for s, (batcher, kw) in enumerate(((ctor, {}), (plain, {"draws": DeviceDraws(SEED, base, views=True)}))):
        torch.manual_seed(s), np.random.seed(s), random.seed(s)
        before = _host_states()
        data = batcher.batch(idx, check=True, **kw)
        assert _states_equal(before, _host_states())
        batcher.join(data)
        torch.cuda.synchronize()
        _same_batch(data, want)
        out.append(data)
    assert ctor.draws.counter == 2 ** 32 + 3                               # one id per slot, as without the flag
    # draw() hands out the device rows and a handle; batch(params=handle) replays it and takes no id
    draws = DeviceDraws(SEED, base, views=True)
    sel, handle = plain.draw(idx, draws=draws)
    assert isinstance(handle, ViewDrawHandle) and (handle.seed, handle.base, handle.count) == (SEED, base, 5)
    assert torch.is_tensor(sel) and np.array_equal(sel.cpu().numpy(), rows)
    data = plain.batch(idx, sel=sel, params=handle, draws=draws)
    plain.join(data)
    torch.cuda.synchronize()
    _same_batch(data, want)
    assert draws.counter == 2 ** 32 + 3
    # explicit params= win for that call: host parameters, device rows
    other = [vr.draw(host.program, M_BATCH, SEED + 1, i, 0) for i in range(len(idx))]
    data = plain.batch(idx, params=other, draws=DeviceDraws(SEED, base, views=True))
    plain.join(data)
    torch.cuda.synchronize()
    _same_batch(data, host.batch(idx, sel=rows, params=other))
    with pytest.raises(RuntimeError, match="handle"):
        plain.batch(idx[:2], params=handle)


@pytest.mark.parametrize("stream", [False, True])
@pytest.mark.parametrize("lists", ["configured", "custom"])
def test_fixmatch_batcher_draws_its_views_on_the_device(lists, stream, no_host_draws):
    from geot_amd.openpoints.dataset import DeviceDraws, FixMatchBatcher, ViewProgram
    lab, unl = _scan_set(BATCH_SIZES, 1), _scan_set(BATCH_SIZES[::-1], 2)
    idx_l, idx_u, base = [1, 3, 0], [0, 2, 3, 1], 40
    bl = len(idx_l)
    sizes = [BATCH_SIZES[i] for i in idx_l] + [BATCH_SIZES[::-1][i] for i in idx_u]
    rows, _ = sd.sample_draw_ref(sizes, M_BATCH, SEED, base)
    if lists == "configured":
        # transforms=None: the expected batch runs on geot_fixmatch_views, whose bits the three ViewPrograms give
        transforms, kwargs = None, FM_KW
        progs = {k: ViewProgram(v, FM_KW) for k, v in FM_LISTS.items()}

        def as_fixmatch(kind, p):
            out = {"kind": kind, "s": np.ones(3, np.float32), "R": np.eye(3, dtype=np.float32), "t": np.zeros(3, np.float32),
                   "rotate": kind == "train_s", "translate": kind == "train_s"}
            if kind != "train_w":
                out["s"] = p[0]["scale"]
            if kind == "train_s":
                out["R"], out["t"] = p[2]["R"], p[3]["t"]
                assert np.array_equal(out["R"], np.eye(3, dtype=np.float32))     # angle_s is absent: the bound is 0
            return out
    else:
        transforms = {"train": ["PointCloudScaling", "PointCloudCenterAndNormalize", "PointCloudJitter", "ChromaticDropGPU"],
                      "train_w": ["PointCloudCenterAndNormalize", "ChromaticPerDropGPU"],
                      "train_s": ["PointCloudScaling_s", "PointCloudJitter_s", "PointCloudCenterAndNormalize", "PointCloudRotation_s",
                                  "RandomHorizontalFlip", "PointCloudTranslation_s"]}
        kwargs = dict(FM_KW, angle_s=[0.1, 1, 0.2], upright_axis="y", jitter_sigma_s=0.01)
        progs = {k: ViewProgram(v, kwargs) for k, v in transforms.items()}

        def as_fixmatch(kind, p):
            return p
    params = [as_fixmatch("train", vr.draw(progs["train"], M_BATCH, SEED, base + i, 0)) for i in range(bl)]
    params += [(as_fixmatch("train_w", vr.draw(progs["train_w"], M_BATCH, SEED, base + bl + i, 1)),
                as_fixmatch("train_s", vr.draw(progs["train_s"], M_BATCH, SEED, base + bl + i, 2))) for i in range(len(idx_u))]
    host = FixMatchBatcher(lab, unl, M_BATCH, kwargs=kwargs, transforms=transforms)
    want = host.batch(idx_l, idx_u, sel_l=rows[:bl], sel_u=rows[bl:], params=params, check=True)
    side = torch.cuda.Stream() if stream else None
    ctor = FixMatchBatcher(lab, unl, M_BATCH, kwargs=kwargs, transforms=transforms, stream=side,
                           draws=DeviceDraws(SEED, base, views=True))
    plain = FixMatchBatcher(lab, unl, M_BATCH, kwargs=kwargs, transforms=transforms, stream=side)
    no_host_draws()
    for s, (batcher, kw) in enumerate(((ctor, {}), (plain, {"draws": DeviceDraws(SEED, base, views=True)}))):
        torch.manual_seed(s), np.random.seed(s), random.seed(s)
        before = _host_states()
        data, data_u = batcher.batch(idx_l, idx_u, check=True, **kw)
        assert _states_equal(before, _host_states())
        batcher.join(data, data_u)
        torch.cuda.synchronize()
        _same_batch(data, want[0])
        _same_batch(data_u, want[1])
    assert ctor.draws.counter == base + 7
    draws = DeviceDraws(SEED, base, views=True)
    sel, handle = plain.draw(idx_l, idx_u, draws=draws)
    assert (handle.seed, handle.base, handle.count) == (SEED, base, 7) and np.array_equal(sel.cpu().numpy(), rows)
    data, data_u = plain.batch(idx_l, idx_u, sel_l=sel[:bl], sel_u=sel[bl:], params=handle)
    plain.join(data, data_u)
    torch.cuda.synchronize()
    _same_batch(data_u, want[1])
    # explicit rows with device views: the slots still take their ids, for the views alone
    data, data_u = plain.batch(idx_l, idx_u, sel_l=rows[:bl], sel_u=rows[bl:], draws=draws)
    plain.join(data, data_u)
    torch.cuda.synchronize()
    assert draws.counter == base + 14 and not torch.equal(data_u["pos_s"], want[1]["pos_s"])
    _same_batch({k: data_u[k] for k in ("pos", "y", "pos_w")}, {k: want[1][k] for k in ("pos", "y", "pos_w")})   # (no draw in these)


def test_val_batcher_accepts_the_flag_and_draws_nothing(no_host_draws):
    from geot_amd.openpoints.dataset import DeviceDraws, ValBatcher
    scans = _scan_set(BATCH_SIZES, 4)
    batcher = ValBatcher(scans, M_BATCH)
    idx = [0, 1, 2, 3]
    rows, _ = sd.sample_draw_ref(BATCH_SIZES, M_BATCH, SEED, 0)
    want = batcher.batch(idx, sel=rows, check=True)
    no_host_draws()
    before = _host_states()
    draws = DeviceDraws(SEED, views=True)
    got = batcher.batch(idx, check=True, draws=draws)
    assert draws.counter == 4 and _states_equal(before, _host_states())
    _same_batch(got, want)
    side = ValBatcher(scans, M_BATCH, stream=torch.cuda.Stream(), draws=DeviceDraws(SEED, views=True))
    data = side.batch(idx)
    side.join(data)
    torch.cuda.synchronize()
    _same_batch(data, want)


def test_without_the_flag_the_views_are_the_seeded_host_draws():
    """views=False is the behaviour before the flag existed: device rows, the list's draws from the global host generators."""
    from geot_amd.openpoints.dataset import DeviceDraws, FixMatchBatcher, SupervisedBatcher
    scans = _scan_set(BATCH_SIZES, 3)
    batcher = SupervisedBatcher(scans, M_BATCH)
    idx = [3, 1, 0, 2]
    rows, _ = sd.sample_draw_ref([BATCH_SIZES[i] for i in idx], M_BATCH, SEED, 9)

    def seed_all():
        torch.manual_seed(21), np.random.seed(21), random.seed(21)
    seed_all()
    params = [batcher.program.draw(M_BATCH) for _ in idx]
    want = batcher.batch(idx, sel=rows, params=params)
    after = _host_states()
    seed_all()
    draws = DeviceDraws(SEED, 9)
    got = batcher.batch(idx, draws=draws)
    assert _states_equal(after, _host_states()) and draws.counter == 13 and draws.state() == {"seed": SEED, "counter": 13}
    _same_batch(got, want)
    sel, drawn = batcher.draw(idx, draws=DeviceDraws(SEED, 9))
    assert isinstance(drawn, list) and len(drawn) == 4 and isinstance(drawn[0], list)
    lab, unl = _scan_set(BATCH_SIZES, 1), _scan_set(BATCH_SIZES[::-1], 2)
    fm = FixMatchBatcher(lab, unl, M_BATCH)
    seed_all()
    sel, params = fm.draw([0, 1], [2, 3], draws=DeviceDraws(SEED, 9))
    want = fm.batch([0, 1], [2, 3], sel_l=sel[:2], sel_u=sel[2:], params=params)
    seed_all()
    got = fm.batch([0, 1], [2, 3], draws=DeviceDraws(SEED, 9))
    _same_batch(got[0], want[0])
    _same_batch(got[1], want[1])
