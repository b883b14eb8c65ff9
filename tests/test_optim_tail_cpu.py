"""The fused tail of an iteration (clip + AdamW + the teacher's EMA; include/geot_hip.h "ABI 25") without a GPU: the fp64
restatement the GPU tests referee with against torch itself in float64, that its derived error bounds are not vacuous, the
launch plan through the built library on either side of every boundary, the cfg checks and the ABI."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import _optim_tail_ref as ref
from geot_amd import _lib, optim_tail as ot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53


def test_constants_agree_with_the_restatement():
    assert ot.BLOCK_ELEMS == ref.BLOCK == _lib.OPTIM_TAIL_BLOCK_ELEMS
    assert ot.CAP == _lib.OPTIM_TAIL_CAP >= 2
    # the by-value table, the groups and the launch's scalars fit the 4 KB of kernel arguments
    words = _lib.OPTIM_TAIL_REC_WORDS, _lib.OPTIM_TAIL_GROUP_WORDS
    assert 4 * (ot.CAP * words[0] + ot.MAX_GROUPS * words[1]) + 64 <= 4096
    assert 4 * _lib.OPTIM_TAIL_STEP_CAP + 64 <= 4096


@pytest.mark.parametrize("hp", [ref.REFERENCE_HP, ref.EXAGGERATED_HP], ids=["reference", "exaggerated"])
def test_restatement_equals_torch_in_float64(hp):
    """clip_grad_norm_ + torch.optim.AdamW + lerp in float64 on the CPU, three consecutive steps: every step agrees with
    the restatement, started from torch's own state, within the derived bound at u = 2^-53 (the sum in any order: chain = the
    number of terms) -- twice that bound: at this precision the restatement rounds as often as torch does."""
    recs = ref.make_records(1, warm=False)
    groups = ref.groups_of(hp)
    params = [torch.nn.Parameter(torch.from_numpy(r["p"].astype(np.float64))) for r in recs]
    teachers = [None if r["t"] is None else torch.from_numpy(r["t"].astype(np.float64)) for r in recs]
    opt = torch.optim.AdamW([dict(params=[p for p, r in zip(params, recs) if r["group"] == k], **groups[k]) for k in (0, 1)])
    clipped = [p for p, r in zip(params, recs) if r["clipped"]]
    n_terms = sum(p.numel() for p in clipped)
    decay, max_norm = 0.9, 1.0
    rng = np.random.default_rng(5)
    for step in range(3):
        state = []
        for p, r, t in zip(params, recs, teachers):
            g = rng.standard_normal(p.numel())
            p.grad = torch.from_numpy(g.copy())
            st = opt.state.get(p, {})
            state.append(dict(kind="adamw", p=p.detach().numpy().copy(), g=g, group=r["group"], clipped=r["clipped"], step=step,
                              m=st["exp_avg"].numpy().copy() if st else np.zeros(p.numel()),
                              v=st["exp_avg_sq"].numpy().copy() if st else np.zeros(p.numel()),
                              t=None if t is None else t.numpy().copy()))
        want, norm, coef = ref.tail(state, groups, max_norm, decay, u=U64, chain=n_terms)
        assert coef < 1.0
        got_norm = float(torch.nn.utils.clip_grad_norm_(clipped, max_norm))
        opt.step()
        assert abs(got_norm - norm) <= 2 * ref.norm_error(n_terms, U64) * norm
        for p, t, w in zip(params, teachers, want):
            st = opt.state[p]
            assert float(st["step"]) == w["step"]
            assert ref.ratio(p.detach().numpy(), w["p"], w["E_p"]) <= 2.0
            assert ref.ratio(st["exp_avg"].numpy(), w["m"], w["E_m"]) <= 2.0
            assert ref.ratio(st["exp_avg_sq"].numpy(), w["v"], w["E_v"]) <= 2.0
            if t is not None:
                t.lerp_(p.detach(), 1.0 - decay)
                assert ref.ratio(t.numpy(), w["t"], w["E_t"]) <= 2.0


@pytest.mark.parametrize("term", ["wd", "bc1", "bc2", "eps", "clip", "ema"])
def test_the_bound_is_not_vacuous(term):
    """Under the exaggerated hyper-parameters, leaving out any single term moves some element by far more than the bound
    (the restatement alone): a kernel that forgot it cannot pass."""
    recs = ref.make_records(2, warm=True)
    groups = ref.groups_of(ref.EXAGGERATED_HP)
    full, _, coef = ref.tail(recs, groups, 1.0, 0.9)
    assert coef < 0.5
    less, _, _ = ref.tail(recs, groups, 1.0, 0.9, drop=(term,))
    key, bound = ("t", "E_t") if term == "ema" else ("p", "E_p")
    worst = 0.0
    for a, b in zip(full, less):
        if key in a and a[key].size:
            worst = max(worst, float((np.abs(a[key] - b[key]) / a[bound]).max()))
    assert worst > 1000.0, (term, worst)


def test_the_bound_is_small_under_the_reference_hyperparameters():
    """... and the bound itself stays at rounding level: a few fp32 ulp of the values it bounds."""
    recs = ref.make_records(3, warm=True)
    out, _, _ = ref.tail(recs, ref.groups_of(ref.REFERENCE_HP), 1.0, 0.99)
    for r in out:
        if r["p"].size:
            assert float((r["E_p"] / np.maximum(np.abs(r["p"]), 1e-3)).max()) < 64 * ref.U
            assert float((r["E_t"] / np.maximum(np.abs(r["t"]), 1e-3)).max()) < 64 * ref.U if "t" in r else True


# ---- the plan, through the built library -------------------------------------------------------------------------------------------
def _blocks(n):
    return -(-n // ref.BLOCK)


def test_plan_element_counts_on_either_side_of_every_boundary():
    counts = list(ref.COUNTS)
    assert counts == [0, 1, 3, 4, 5, ref.BLOCK, ref.BLOCK + 1, 3 * ref.BLOCK + 7]
    t = len(counts)
    flags = [ot.CLIPPED] * t
    pl = ot.plan(counts, [1] * t, flags)
    assert list(pl["blocks"]) == [0, 1, 1, 1, 1, 1, 2, 4]
    assert list(pl["vector"]) == [1] * t
    assert pl["update_blocks"] == pl["slots"] == 11
    assert pl["update_launches"] == pl["norm_launches"] == 1
    # a record that is not 16-byte aligned takes the scalar path, alone
    aligned = [1] * t
    aligned[6] = 0
    pl = ot.plan(counts, aligned, flags)
    assert list(pl["vector"]) == aligned and list(pl["blocks"]) == [0, 1, 1, 1, 1, 1, 2, 4]
    # only clipped AdamW records are part of the norm; an integer record never takes the vector path
    flags = [ot.CLIPPED, 0, ot.CLIPPED | ot.EMA_ONLY, ot.INT64, ot.CLIPPED, 0, ot.CLIPPED, ot.EMA_ONLY]
    pl = ot.plan(counts, [1] * t, flags)
    assert pl["slots"] == _blocks(counts[0]) + _blocks(counts[4]) + _blocks(counts[6]) == 3
    assert list(pl["vector"]) == [1, 1, 1, 0, 1, 1, 1, 1]
    assert pl["update_blocks"] == 11
    # nothing to do: no launch
    pl = ot.plan([0, 0], [1, 1], [ot.CLIPPED, 0])
    assert pl["update_launches"] == pl["norm_launches"] == pl["slots"] == 0
    assert ot.plan([], [], [])["update_launches"] == 0
    with pytest.raises(RuntimeError):
        ot.plan([4, -1], [1, 1], [0, 0])


@pytest.mark.parametrize("t", [ot.CAP - 1, ot.CAP, ot.CAP + 1, 2 * ot.CAP + 1])
def test_plan_record_counts_around_the_launch_capacity(t):
    counts = [(7 * i) % 9000 + 1 for i in range(t)]
    pl = ot.plan(counts, [1] * t, [ot.CLIPPED] * t)
    assert pl["update_launches"] == pl["norm_launches"] == -(-t // ot.CAP)
    assert list(pl["blocks"]) == [_blocks(n) for n in counts] and pl["slots"] == sum(_blocks(n) for n in counts)
    # every second record unclipped: the norm sweep packs the clipped ones, the update sweep keeps the table's chunks
    flags = [ot.CLIPPED if i % 2 == 0 else 0 for i in range(t)]
    pl = ot.plan(counts, [1] * t, flags)
    assert pl["update_launches"] == -(-t // ot.CAP)
    assert pl["norm_launches"] == -(-((t + 1) // 2) // ot.CAP)
    assert pl["slots"] == sum(_blocks(n) for n in counts[::2])
    # a whole launch of empty records is not issued
    counts = [0] * ot.CAP + [1] * (t - ot.CAP) if t > ot.CAP else [0] * t
    pl = ot.plan(counts, [1] * t, [0] * t)
    assert pl["update_launches"] == (-(-t // ot.CAP) - 1 if t > ot.CAP else 0)


# ---- cfg and ABI ------------------------------------------------------------------------------------------------------------------
def test_cfg_keys_defaults_and_checks():
    from geot_amd import train_step as ts
    assert ts.NTM_CFG["ema_teacher"] is False and ts.NTM_CFG["fused_tail"] is False and ts.NTM_CFG["ema_decay"] == 0.99
    ts.check_cfg(dict(ts.NTM_CFG))
    ts.check_cfg(dict(ts.NTM_CFG, ema_teacher=True, fused_tail=True, ema_decay=0))
    old = {k: v for k, v in ts.NTM_CFG.items() if k not in ("ema_teacher", "fused_tail", "ema_decay")}
    ts.check_cfg(old)                                            # a cfg from before the keys: the switches are off
    for key in ("ema_teacher", "fused_tail"):
        for bad in (1, 0, "yes", None):
            with pytest.raises(TypeError):
                ts.check_cfg(dict(ts.NTM_CFG, **{key: bad}))
    for bad in ("0.9", None, True):
        with pytest.raises(TypeError):
            ts.check_cfg(dict(ts.NTM_CFG, ema_decay=bad))
    for bad in (1.0, 1, -0.1, 2.5, float("nan")):
        with pytest.raises(ValueError):
            ts.check_cfg(dict(ts.NTM_CFG, ema_decay=bad))
    with pytest.raises(TypeError):
        ts.SupervisedStep(torch.nn.Linear(2, 2), fused_tail=1)


def test_header_parses_and_abi_agrees():
    hdr = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    assert int(re.search(r"GEOT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 25
    lib = _lib.load()
    assert lib.geot_abi_version() == _lib.ABI_VERSION
    for name in ("geot_optim_tail_norm", "geot_optim_tail_finish", "geot_optim_tail_update"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert "geot_optim_tail_plan" in _lib.PLAIN
    assert ot.RECORD.itemsize == 64 and ot.GROUP.itemsize == 40


def test_construction_refuses_what_the_kernels_do_not_do():
    """amsgrad / maximize, another optimizer class, a teacher that does not pair by name: RuntimeError before any launch
    (the parameter checks need no GPU: a CPU parameter is refused too, there is no CPU path)."""
    lin = torch.nn.Linear(3, 2)
    with pytest.raises(RuntimeError, match="contiguous float32 tensors on the GPU"):
        ot.OptimTail([torch.optim.AdamW(lin.parameters())])
    for kw in (dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(RuntimeError, match="amsgrad / maximize"):
            ot.OptimTail([torch.optim.AdamW(lin.parameters(), **kw)])
    with pytest.raises(RuntimeError, match="not a torch.optim.AdamW"):
        ot.OptimTail([torch.optim.SGD(lin.parameters(), lr=0.1)])
    with pytest.raises(RuntimeError, match="same entries"):
        ot.teacher_pairs(lin, torch.nn.Linear(3, 2, bias=False))
    with pytest.raises(RuntimeError, match="in the student"):
        ot.teacher_pairs(lin, torch.nn.Linear(4, 2))
    pairs = ot.teacher_pairs(torch.nn.BatchNorm1d(4), copy.deepcopy(torch.nn.BatchNorm1d(4)))
    assert [n for _, _, n in pairs] == ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
