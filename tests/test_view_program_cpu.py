"""CPU suite: the host half of the view programs (geot_amd/openpoints/dataset/view_program.py, supervised_batch.py) against
the reference-executed fixture tests/golden/view_program_ref.npz (tests/golden/make_view_program_golden.py) -- the random
draws of every supported transform, the three generators' state after them, the compiler's aliasing decisions, the tests'
own restatement (tests/_view_program_ref.py), the argument checks of the host and of the entry point.  No GPU."""
import ctypes
import json
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _view_program_ref as vpr  # noqa: E402
from _view_program_ref import fixture_params  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("a", "b", "c", "d")
DRAWN = ("scale", "t", "R", "noise", "mask")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("view_program_ref.npz")


def _case(fx, case):
    return [str(n) for n in fx[case + "_names"]], json.loads(str(fx[case + "_kwargs"]))


def _sizes(fx):
    return [fx["scan%d" % i].shape[0] for i in range(3)]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _replay(fx, case):
    """The per-item sequence of the reference under the fixture's seed: np.random.choice, then the list's draws."""
    from geot_amd.openpoints.dataset import ViewProgram
    names, kwargs = _case(fx, case)
    program = ViewProgram(names, kwargs)
    m, seed = int(fx["num_points"]), int(fx[case + "_seed"])
    np.random.seed(seed)
    torch.manual_seed(seed)
    random.seed(seed)
    drawn = []
    for i, n in enumerate(_sizes(fx)):
        sel = np.random.choice(n, m, replace=n < m)
        assert np.array_equal(sel, fx[case + "_sel"][i])
        drawn.append(program.draw(m))
    return program, drawn


def _assert_params_equal(got, want, where):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w), (where, k, sorted(g), sorted(w))
        for what in g:
            if what in DRAWN:
                assert _same_bits(g[what], w[what]), (where, k, what)
            else:
                assert g[what] == w[what], (where, k, what, g[what], w[what])


@pytest.mark.parametrize("case", CASES)
def test_draws_match_the_reference_bit_for_bit(fx, case):
    _, drawn = _replay(fx, case)
    for i, got in enumerate(drawn):
        _assert_params_equal(got, fixture_params(fx, case, i), (case, i))


@pytest.mark.parametrize("case", CASES)
def test_generators_end_where_the_reference_left_them(fx, case):
    _replay(fx, case)
    assert np.array_equal(np.random.random_sample(4), fx[case + "_next_np"])
    assert np.array_equal(torch.rand(4).numpy(), fx[case + "_next_torch"])
    assert np.array_equal(np.array([random.random() for _ in range(4)]), fx[case + "_next_py"])


@pytest.mark.parametrize("case", CASES)
def test_supervised_batcher_draw_order_is_the_per_item_order(fx, case):
    """SupervisedBatcher.draw (host only) consumes the three streams as the dataset and its transform list do."""
    from geot_amd.openpoints.dataset import SupervisedBatcher, ViewProgram
    names, kwargs = _case(fx, case)
    b = SupervisedBatcher.__new__(SupervisedBatcher)          # the draw needs the sizes alone: no device
    b.m, b.program = int(fx["num_points"]), ViewProgram(names, kwargs)
    b.scans = type("Sizes", (), {"sizes": _sizes(fx)})()
    seed = int(fx[case + "_seed"])
    np.random.seed(seed)
    torch.manual_seed(seed)
    random.seed(seed)
    sel, params = b.draw([0, 1, 2])
    assert np.array_equal(sel, fx[case + "_sel"])
    for i in range(3):
        _assert_params_equal(params[i], fixture_params(fx, case, i), (case, i))
    assert np.array_equal(np.random.random_sample(4), fx[case + "_next_np"])
    assert np.array_equal(torch.rand(4).numpy(), fx[case + "_next_torch"])
    assert np.array_equal(np.array([random.random() for _ in range(4)]), fx[case + "_next_py"])


@pytest.mark.parametrize("case", CASES)
def test_aliasing_decision_matches_the_reference(fx, case):
    """x is still pos after the list, or not; heights exist, or not -- and where the compiler puts the one x store."""
    from geot_amd.openpoints.dataset import ViewProgram, view_program as vp
    names, kwargs = _case(fx, case)
    program = ViewProgram(names, kwargs)
    assert program.x_is_pos == bool(fx[case + "_x_is_pos"]) == (case == "c")
    assert program.has_heights == bool(fx[case + "_has_heights"]) == (case != "c")
    assert ((case + "_b_heights") in fx.files) == program.has_heights
    m = int(fx["num_points"])
    for i in range(3):
        params = fixture_params(fx, case, i)
        ops, noise, masks = program.compile(params, m)
        kinds = [op[0] for op in ops]
        assert kinds.count(vp.STORE_X) == 1 and len(ops) <= 16
        if case == "a":       # scaled in place, separated by the centring; the drop, when it fires, folds into the store
            drop = params[-1]["drop"]
            assert kinds == [vp.SCALE, vp.STORE_X, vp.CENTER_NORM, vp.JITTER]
            assert ops[1][1] == (1 if drop else 0) and ops[2][1] == (1 | 2 | (1 << 2)) and len(noise) == 1 and not masks
        if case == "b":       # the first transform rebinds: x is the sample
            assert kinds == [vp.STORE_X, vp.SCALE_TRANSLATE, vp.CENTER_NORM, vp.JITTER, vp.ROTATE, vp.TRANSLATE]
        if case == "c":       # nothing rebinds: the mask hits pos, x is stored last
            flips = len(params[3]["flip"])
            assert kinds == [vp.JITTER, vp.SCALE] + [vp.FLIP] * flips + [vp.XYZ_ALIGN, vp.MASK, vp.STORE_X]
            assert len(masks) == 1 and ops[-1][1] == 0
        if case == "d":       # centering=False still rebinds through the normalisation
            assert kinds == [vp.STORE_X, vp.SCALE_JITTER, vp.CENTER_NORM, vp.TRANSLATE] and ops[2][1] == (2 | (1 << 2))
    # a chromatic transform AFTER the separation folds into the store; a second mask multiplies into the first
    late = ViewProgram(["PointCloudRotation", "ChromaticPerDropGPU", "ChromaticPerDropGPU", "ChromaticDropGPU"], {})
    m1, m2 = (np.arange(8) % 2).astype(np.float32), (np.arange(8) % 3 > 0).astype(np.float32)
    base = [{"R": np.eye(3)}, {"mask": m1}, {"mask": m2}]
    ops, _, masks = late.compile(base + [{"drop": False}], 8)
    assert [op[:2] for op in ops] == [(vp.STORE_X, 2), (vp.ROTATE, 0)] and np.array_equal(masks[0], m1 * m2)
    ops, _, masks = late.compile(base + [{"drop": True}], 8)
    assert [op[:2] for op in ops] == [(vp.STORE_X, 1), (vp.ROTATE, 0)]


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_fixture_within_e_ref(fx, case):
    names, kwargs = _case(fx, case)
    for i in range(3):
        params, raw = fixture_params(fx, case, i), fx[case + "_raw_pos"][i]
        ref = vpr.run(raw, names, kwargs, params, np.float64)
        f32 = vpr.run(raw, names, kwargs, params, np.float32)
        assert ref["x_is_pos"] == f32["x_is_pos"] == bool(fx[case + "_x_is_pos"])
        for key, want in (("pos", ref["pos"]), ("x", ref["x"].T), ("heights", ref["heights"])):
            if want is None:
                assert (case + "_b_" + key) not in fx.files
                continue
            e_ref = float(fx[case + "_eref_" + key])
            assert e_ref < 1e-6
            err = np.abs(fx[case + "_b_" + key][i].astype(np.float64) - want).max()
            print("%s %s[%d]: |fixture - fp64| = %.3e (e_ref %.3e)" % (case, key, i, err, e_ref))
            assert err <= e_ref
        # single fp32 elementwise operations of identical inputs: the fp32 restatement carries the reference's bits
        if case != "c":
            assert _same_bits(fx[case + "_b_x"][i], f32["x"].T)
            assert _same_bits(fx[case + "_b_heights"][i], f32["heights"])
        else:
            dropped = fx["c_t5_mask"][i] == 0
            assert dropped.any() and not dropped.all()
            assert not f32["pos"][dropped].any() and not fx["c_b_pos"][i][dropped].any()
            assert np.array_equal(np.signbit(f32["pos"]), np.signbit(fx["c_b_pos"][i]))
        assert np.abs(f32["pos"].astype(np.float64) - ref["pos"]).max() <= 1e-6


def _interpret(raw, ops, noise, masks):
    """The ops of one view executed as include/geot_hip.h states them, one fp32 numpy operation per statement (the mean:
    fp64, rounded once) -> pos (m, 3), x (m, 3), heights (m, 1) or None."""
    from geot_amd.openpoints.dataset import view_program as vp
    p, x, heights = np.array(raw, dtype=np.float32), None, None
    for kind, arg, f in ops:
        f = np.asarray(f, dtype=np.float32)
        if kind == vp.SCALE:
            p = p * f[:3]
        elif kind == vp.CENTER_NORM:
            g = arg >> 2
            heights = p[:, g:g + 1] - p[:, g].min()
            if arg & 1:
                p = p - p.astype(np.float64).mean(axis=0).astype(np.float32)
            if arg & 2:
                p = p / np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]).max()
        elif kind == vp.XYZ_ALIGN:
            p = p - p.astype(np.float64).mean(axis=0).astype(np.float32)
            p[:, arg] = p[:, arg] - p[:, arg].min()
        elif kind == vp.TRANSLATE:
            p = p + f[:3]
        elif kind == vp.SCALE_TRANSLATE:
            p = p * f[:3] + f[3:6]
        elif kind == vp.JITTER:
            p = p + noise[arg]
        elif kind == vp.SCALE_JITTER:
            p = p * f[:3] + noise[arg]
        elif kind == vp.ROTATE:
            p = np.stack([(p[:, 0] * f[3 * k] + p[:, 1] * f[3 * k + 1]) + p[:, 2] * f[3 * k + 2] for k in range(3)], axis=1)
        elif kind == vp.FLIP:
            p[:, arg] = p.max() - p[:, arg]
        elif kind == vp.ZERO:
            p = np.zeros_like(p)
        elif kind == vp.MASK:
            p = p * masks[arg][:, None]
        elif kind == vp.STORE_X:
            assert x is None, "x is stored once"
            x = {0: p.copy(), 1: np.zeros_like(p), 2: p * masks[arg >> 2][:, None] if arg & 3 == 2 else None}[arg & 3]
        else:
            raise AssertionError(kind)
        assert p.dtype == np.float32
    return p, x, heights


@pytest.mark.parametrize("case", CASES)
def test_compiled_ops_read_as_the_header_states_them_give_the_restatements_bits(fx, case):
    """The compiler against the referee: the referee works from the class names with literal aliasing, the ops from the
    compiler's decisions; executed with the same single fp32 operations the two must agree in every bit -- and, where the
    reference reaches a value through such operations alone, with the fixture."""
    from geot_amd.openpoints.dataset import ViewProgram
    names, kwargs = _case(fx, case)
    program = ViewProgram(names, kwargs)
    for i in range(3):
        params, raw = fixture_params(fx, case, i), fx[case + "_raw_pos"][i]
        pos, x, heights = _interpret(raw, *program.compile(params, raw.shape[0]))
        f32 = vpr.run(raw, names, kwargs, params, np.float32)
        assert _same_bits(pos, f32["pos"]) and _same_bits(x, f32["x"]), (case, i)
        assert (heights is None) == (f32["heights"] is None) and (heights is None or _same_bits(heights, f32["heights"]))
        if case != "c":
            assert _same_bits(x.T, fx[case + "_b_x"][i]) and _same_bits(heights, fx[case + "_b_heights"][i])
        assert np.abs(pos.astype(np.float64) - fx[case + "_b_pos"][i]).max() <= 1e-5


def test_fixture_is_data_with_provenance_and_both_branches(fx):
    meta = json.loads(str(fx["meta"]))
    assert meta["generator"] == "tests/golden/make_view_program_golden.py" and meta["provenance"]
    assert all(a.dtype.kind in "fiuU" for a in (fx[k] for k in fx.files))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "view_program_ref.npz")) < \
        os.path.getsize(os.path.join(ROOT, "tests", "golden", "fixmatch_views_ref.npz"))
    from geot_amd.openpoints.dataset import DEFAULT_TRAIN, DEFAULT_TRAIN_KWARGS
    names, kwargs = _case(fx, "a")
    assert names == DEFAULT_TRAIN and kwargs == DEFAULT_TRAIN_KWARGS
    assert min(_sizes(fx)) < int(fx["num_points"]) >= 200 and fx["a_b_pos"].shape[0] >= 3
    drops = fx["a_t4_drop"]
    assert drops.any() and not drops.all()
    for i in range(3):
        assert (not fx["a_b_x"][i].any()) == bool(drops[i])
    flips = fx["c_t3_flip"][:, [0, 2]]
    assert flips.any() and not flips.all() and not fx["c_t3_flip"][:, 1].any()
    signs = np.sign(fx["c_t2_scale"])
    assert (signs < 0).any() and (signs > 0).any()
    kept = fx["c_t5_mask"].sum(axis=1)
    assert ((kept >= 1) & (kept <= int(fx["num_points"]) - 1)).all()
    assert set(np.unique(np.abs(np.sign(fx["d_t1_scale"][:, 1])))) == {1.0} and (fx["d_t1_scale"][:, 1] > 0).all()   # mirror 0: never


def test_unsupported_transforms_raise_before_any_device_call():
    from geot_amd.openpoints.dataset import DeviceScanSet, FixMatchBatcher, SupervisedBatcher, ViewProgram  # noqa: F401
    for names, kwargs, word in ((["PointsToTensor", "RandomDropout"], {}, "RandomDropout"),
                                (["ChromaticNormalize"], {}, "ChromaticNormalize"),
                                (["PointCloudCenterAndNormalize"], {"append_xyz": True}, "append_xyz"),
                                (["PointCloudFloorCentering"], {}, "PointCloudFloorCentering")):
        with pytest.raises(NotImplementedError, match=word):
            ViewProgram(names, kwargs)
    with pytest.raises(RuntimeError, match="upright_axis"):
        ViewProgram(["RandomHorizontalFlip"], {})
    with pytest.raises(RuntimeError, match="the kernel takes 16"):
        ViewProgram(["PointCloudTranslation"] * 16, {})
    with pytest.raises(RuntimeError, match="must be a DeviceScanSet"):
        SupervisedBatcher(None, 16)
    # the batchers build their programs before they touch their scans
    sizes = type("NotAScanSet", (DeviceScanSet,), {"__init__": lambda self: None})()
    with pytest.raises(NotImplementedError, match="RandomDropout"):
        SupervisedBatcher(sizes, 16, transforms=["RandomDropout"])


def test_bad_records_are_refused_on_the_host():
    from geot_amd import _lib
    from geot_amd.openpoints.dataset import ViewProgram, pack_program_jobs, view_program_views
    from geot_amd.openpoints.dataset import view_program as vp
    prog = ViewProgram(["PointCloudScaling", "PointCloudCenterAndNormalize", "PointCloudJitter", "ChromaticPerDropGPU"],
                       {"gravity_dim": 1})
    m = 8
    good = [{"scale": [1, 2, 3]}, {}, {"noise": np.full((m, 3), .5, np.float32)}, {"mask": np.ones(m, np.float32)}]
    with pytest.raises(RuntimeError, match="CPU not supported"):
        view_program_views(torch.zeros(1, m, 3), [(0, 0, prog, good)])
    with pytest.raises(RuntimeError, match="reads row 2 of 2"):
        pack_program_jobs([(2, 0, prog, good)], 2, 1, m)
    with pytest.raises(RuntimeError, match="each row once"):
        pack_program_jobs([(0, 0, prog, good), (1, 0, prog, good)], 2, 2, m)
    with pytest.raises(RuntimeError, match="each row once"):
        pack_program_jobs([(0, 1, prog, good)], 2, 1, m)
    with pytest.raises(RuntimeError, match="at least one job"):
        pack_program_jobs([], 1, 1, m)
    with pytest.raises(RuntimeError, match="one dict per transform"):
        pack_program_jobs([(0, 0, prog, good[:2])], 1, 1, m)
    with pytest.raises(RuntimeError, match="lack 'scale'"):
        pack_program_jobs([(0, 0, prog, [{}] + good[1:])], 1, 1, m)
    with pytest.raises(RuntimeError, match=r"noise must be \(8, 3\)"):
        pack_program_jobs([(0, 0, prog, good[:2] + [{"noise": np.zeros((m + 1, 3))}] + good[3:])], 1, 1, m)
    with pytest.raises(RuntimeError, match=r"mask must be \(8,\)"):
        pack_program_jobs([(0, 0, prog, good[:3] + [{"mask": np.zeros((m, 1))}])], 1, 1, m)
    with pytest.raises(RuntimeError, match="source row, output row, program, params"):
        pack_program_jobs([(0, 0, good)], 1, 1, m)
    # the record layout the kernel reads (include/geot_hip.h): header 0-4, then ops of 14 words: kind, arg, 12 floats
    table, noise, masks = pack_program_jobs([(1, 0, prog, good), (0, 1, prog, good)], 2, 2, m)
    assert table.shape == (2, _lib.VIEW_PROGRAM_JOB_WORDS) == (2, 232) and table.dtype == np.int32
    assert table[0, :8].tolist() == [1, 0, 4, 0, 0, 0, 0, 0] and table[1, :8].tolist() == [0, 1, 4, 1, 1, 0, 0, 0]
    assert noise.shape == (2, m, 3) and masks.shape == (2, m) and noise.dtype == masks.dtype == np.float32
    as_f = table.view(np.float32)
    assert table[0, 8:10].tolist() == [vp.SCALE, 0] and as_f[0, 10:13].tolist() == [1, 2, 3]
    assert table[0, 22:24].tolist() == [vp.STORE_X, 2 | (0 << 2)]           # the mask of job 0: its row 0, folded into the store
    assert table[0, 36:38].tolist() == [vp.CENTER_NORM, 1 | 2 | (1 << 2)] and table[0, 50:52].tolist() == [vp.JITTER, 0]
    assert not table[0, 64:].any()


def test_entry_point_refuses_bad_arguments_without_a_device():
    """hipErrorInvalidValue (1) before any launch: null pointers, sizes, and every field of the host copy of the records.
    The device pointers are the bogus non-null address of tests/test_views_cpu.py: every call here must be refused BEFORE
    the launch.  (The hazard of the idiom: on a machine with a GPU, a host check that stopped working would launch a kernel
    on that address instead of failing here -- which is why no accepted call can be part of this test.)"""
    from geot_amd import _lib
    from geot_amd.openpoints.dataset import ViewProgram, pack_program_jobs
    lib = _lib.load()
    prog = ViewProgram(["PointCloudJitter", "ChromaticPerDropGPU", "PointCloudCenterAndNormalize", "ChromaticPerDropGPU",
                        "RandomHorizontalFlip"], {"upright_axis": "z"})      # -> JITTER, MASK, STORE_X (masked), CENTER_NORM, FLIP
    m = 8
    ones = {"mask": np.ones(m, np.float32)}
    good = [{"noise": np.zeros((m, 3), np.float32)}, ones, {}, ones, {"flip": [0]}]
    table, _, _ = pack_program_jobs([(0, 0, prog, good), (0, 1, prog, good)], 1, 2, m)
    one = 4096          # any non-null address: the checks come before it is used

    def args(tab, **over):
        a = dict(j=2, m=m, n_rows=1, n_out=2, n_noise=2, n_mask=4, raw=one, jobs_host=tab.ctypes.data, jobs=one, noise=one,
                 mask=one, pos=one, x=one, heights=one, view_center=one, view_scale=one)
        a.update(over)
        return list(a.values()) + [None]
    bad_scalar = [dict(j=0), dict(j=70000), dict(m=0), dict(m=400000000), dict(n_rows=0), dict(n_out=0), dict(n_noise=-1),
                  dict(n_mask=-1), dict(raw=None), dict(jobs_host=None), dict(jobs=None), dict(pos=None), dict(x=None),
                  dict(view_center=None), dict(view_scale=None), dict(noise=None), dict(mask=None), dict(heights=None),
                  dict(n_noise=1), dict(n_mask=3), dict(n_out=1)]
    assert [int(k) for k in table[0, 8::14][:5]] == [6, 11, 12, 2, 9] and table[1, 3:5].tolist() == [1, 2]
    for over in bad_scalar:
        assert lib.geot_view_program(*args(table, **over)) == 1, over
    # [job, word] <- value: rows, the op count, an unknown kind, args out of range, an output row named twice
    kinds = [int(k) for k in table[0, 8::14][:int(table[0, 2])]]
    at = {k: 8 + 14 * i for i, k in enumerate(kinds)}
    bad_words = [(0, 0, 1), (0, 0, -1), (0, 1, 2), (1, 1, 0), (0, 2, 17), (0, 2, -1), (0, 3, -1), (1, 3, 2), (0, 4, 5),
                 (0, 8, 0), (0, 8, 13), (0, 8, 99), (0, at[6] + 1, 2), (0, at[6] + 1, -1), (0, at[2] + 1, 3 << 2),
                 (0, at[2] + 1, -1), (0, at[9] + 1, 3), (0, at[11] + 1, 4), (0, at[11] + 1, -1), (0, at[12] + 1, 3), (0, at[12] + 1, -4)]
    for job, word, value in bad_words:
        tab = table.copy()
        tab[job, word] = value
        assert lib.geot_view_program(*args(tab)) == 1, (job, word, value)
    tab = table.copy()
    tab[0, at[12] + 1] = 2 | (5 << 2)         # x store through a mask row that does not exist
    assert lib.geot_view_program(*args(tab)) == 1
    assert _lib.VIEW_MAX_OPS == 16 and _lib.VIEW_PROGRAM_JOB_WORDS == 8 + 14 * 16


def test_header_declares_the_entry_point_and_abi_16():
    from geot_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    assert re.search(r"\bint geot_view_program\(", hdr) and "geot_view_program" in _lib.PROTOTYPES
    assert int(re.search(r"GEOT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 16
    assert int(re.search(r"#define GEOT_VIEW_MAX_OPS (\d+)", hdr).group(1)) == _lib.VIEW_MAX_OPS
    assert _lib.load().geot_abi_version() == _lib.ABI_VERSION
    from geot_amd import build
    assert "view_program.hip" in build.SOURCES and "views.h" in build.HEADERS
    assert len(_lib.PROTOTYPES["geot_view_program"]) == 17 and _lib.PROTOTYPES["geot_view_program"][-1] is ctypes.c_void_p


def test_register_resident_kernel_compiles_without_scratch(tmp_path):
    """view_program_kernel<48> keeps 144 values per thread in registers at 256 VGPRs; that it does so without scratch rests
    on how the source is shaped for this compiler (one diamond per op kind, the opaque thread index, no packed-fp32 pairs:
    geot_amd/build.py SOURCE_FLAGS).  A compiler update that brings the spills back must fail here, not go unnoticed."""
    import subprocess
    from geot_amd import build
    src = os.path.join(build.CSRC, "view_program.hip")
    cmd = [build._hipcc()] + build.FLAGS + ["-DGEOT_DISTANCE_MODE=0"] + build.SOURCE_FLAGS["view_program.hip"] + \
        ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "view_program.o")]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    seen = {}
    for block in out.split("Function Name: ")[1:]:
        name = block.split()[0]
        if "view_program_kernel" in name:
            seen[name] = {k: int(re.search(re.escape(k) + r": (\d+)", block).group(1))
                          for k in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")}
    assert len(seen) == 2, sorted(seen)
    for name, use in seen.items():
        print(name, use)
        assert use["ScratchSize [bytes/lane]"] == 0 and use["VGPRs"] <= 256 and use["Occupancy [waves/SIMD]"] >= 2, (name, use)
