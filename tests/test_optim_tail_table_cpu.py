"""The table harness of the optimizer tail without a GPU (tests/_optim_tail_table.py): its layout -- guards, no overlap, the
misalignment asked for --, that the per-slot bound _optim_tail_ref.slot_error is not vacuous, and, through the library's own
planners on the host, that every case tests/test_optim_tail_table_gpu.py runs sits on the branch it is named after."""
import numpy as np
import pytest

import _optim_tail_ref as ref
import _optim_tail_table as tt
from geot_amd import _lib, optim_tail as ot

CAP, BLOCK, STEP_CAP = tt.CAP, tt.BLOCK, tt.STEP_CAP


def test_constants_agree_with_the_header():
    assert (CAP, BLOCK, STEP_CAP) == (_lib.OPTIM_TAIL_CAP, _lib.OPTIM_TAIL_BLOCK_ELEMS, _lib.OPTIM_TAIL_STEP_CAP)
    assert len(tt.GROUPS) == _lib.OPTIM_TAIL_MAX_GROUPS == 4
    keys = [(g["lr"], g["betas"], g["eps"], g["weight_decay"]) for g in tt.GROUPS]
    assert len(set(keys)) == 4 and len({g["lr"] for g in tt.GROUPS}) == 4 and len({g["betas"] for g in tt.GROUPS}) >= 3


# ---- the layout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tt.CASES))
def test_layout_guards_every_tensor_and_gives_the_alignment_asked_for(name):
    spec = tt.CASES[name]()
    lay = tt.layout(spec)
    for arena, per16 in (("f32", 4), ("i64", 2)):
        guard, spans = lay["guard"][arena], sorted(lay["spans"][arena])
        assert lay["size"][arena] == guard.size
        # no two tensors overlap, every tensor has G guard elements on either side, all of them marked as guards
        assert int((~guard).sum()) == sum(b - a for a, b in spans)
        edge = 0
        for a, b in spans:
            assert a - edge >= tt.G and guard[a - tt.G:a].all() and not guard[a:b].any(), (name, arena, a, b)
            edge = b
        assert guard.size - edge >= tt.G and guard[edge:].all()
    for r, row in zip(spec, lay["at"]):
        size = 8 if r["kind"] == "int" else 4
        for key in tt.KEYS:
            if key not in tt.tensors_of(r):
                assert row[key] is None                     # an empty record, a missing teacher: a null pointer
            else:
                assert (row[key] * size) % 16 == (4 if key in r["misalign"] else 0), (name, key)
    # a record is aligned exactly when nothing it holds was asked off
    assert tt.requested_alignment(spec) == [int(all((row[k] * 4) % 16 == 0 for k in tt.tensors_of(r)) or r["kind"] == "int")
                                            for r, row in zip(spec, lay["at"])]


@pytest.mark.parametrize("name", sorted(tt.CASES))
def test_every_case_clips_and_leaves_some_records_unclipped(name):
    """coef < 0.5 from the inputs of every case (a case without a clipped record would check no slot and no coef), with
    neighbouring step counts that differ."""
    spec = tt.CASES[name]()
    ins = tt.make_inputs(spec, 3)
    held = [r for r in spec if tt.in_norm(r) and r["n"]]
    assert held and ref.clip_coef(ref.total_norm([a["g"] for a, r in zip(ins, spec) if tt.in_norm(r)]), 1.0) < 0.5
    assert tt.plans_of(spec)[0]["slots"] >= 1
    adamw = [r for r in spec if r["kind"] == "adamw"]
    if name != "unissued_launch":
        assert any(not r["clipped"] for r in adamw)
    assert len({r["step0"] for r in adamw}) == 3 and len({r["group"] for r in adamw}) >= 2
    steps = [r["step_index"] for r in adamw]
    assert len(set(steps)) == len(steps) and max(steps) < tt.N_STEPS.get(name, tt.n_steps_of(spec))


def test_inputs_make_a_misrouted_record_visible():
    spec = tt.case_norm_packing()
    a, b = tt.make_inputs(spec, 1), tt.make_inputs(spec, 1, call=1)
    clipped = [x["g"] for x, r in zip(a, spec) if tt.in_norm(r)]
    assert ref.clip_coef(ref.total_norm(clipped), 1.0) < 0.5
    assert all(np.array_equal(x["p"], y["p"]) for x, y in zip(a, b))
    assert any(not np.array_equal(x["g"], y["g"]) for x, y, r in zip(a, b, spec) if r["kind"] == "adamw")
    rows = [r for r in spec if r["kind"] == "adamw"]
    assert all(x["step0"] != y["step0"] or x["group"] != y["group"] for x, y in zip(rows, rows[1:]))
    ints = [x["p"] for x, r in zip(tt.make_inputs(tt.case_int64(), 1), tt.case_int64()) if r["kind"] == "int"]
    assert all(int(x.min()) > 2 ** 40 for x in ints)
    offs, n_acc = tt.acc_offsets(spec, tt.N_STEPS["norm_packing"])
    assert np.all(offs % 4 == 0) and n_acc >= sum(r["n"] for r in spec if r["kind"] == "adamw")
    order = [offs[r["step_index"]] for r in spec if r["kind"] == "adamw"]
    assert order != sorted(order)                           # the accumulator's stretches are not in table order


# ---- the slot bound --------------------------------------------------------------------------------------------------------------
def _kernel_slot(g, vector=True):
    """One workgroup's sum of squares in fp32 in the kernel's order: 16 elements per thread (as 4 quads on the vector path),
    6 shuffle levels over the 64 lanes of a wave, the 4 waves in turn."""
    g = np.zeros(BLOCK, np.float32) + np.pad(np.asarray(g, np.float32), (0, BLOCK - len(g)))
    sq = (g * g).astype(np.float32)
    if vector:
        per_thread = sq.reshape(4, 256, 4).transpose(1, 0, 2).reshape(256, 16)      # e = (it * 256 + tid) * 4 + k
    else:
        per_thread = sq.reshape(16, 256).T                                           # e = it * 256 + tid
    acc = np.zeros(256, np.float32)
    for j in range(16):
        acc = (acc + per_thread[:, j]).astype(np.float32)
    waves = acc.reshape(4, 64).copy()
    off = 32
    while off:
        waves[:, :off] = (waves[:, :off] + waves[:, off:2 * off]).astype(np.float32)
        off //= 2
    total = np.float32(0)
    for w in range(4):
        total = np.float32(total + waves[w, 0])
    return float(total)


def test_slot_error_is_the_counted_bound():
    assert ref.KERNEL_CHAIN == 15 + 6 + 3 and ref.slot_error(ref.KERNEL_CHAIN) == 25 * ref.U
    assert ref.slot_error(0) == ref.U                       # one element: the rounding of its square


@pytest.mark.parametrize("vector", [True, False])
def test_the_slot_bound_is_not_vacuous(vector):
    rng = np.random.default_rng(9)
    g = (rng.standard_normal(3 * BLOCK + 7) * 3.0).astype(np.float32)
    want = tt.expected_slots([tt.rec("adamw", g.size)], [g])
    assert want.size == 4
    got = [_kernel_slot(g[b:b + BLOCK], vector) for b in range(0, g.size, BLOCK)]
    bound = ref.slot_error(ref.KERNEL_CHAIN)
    worst = max(abs(x - w) / (bound * w) for x, w in zip(got, want))
    assert 0.0 < worst <= 1.0, worst
    # a slot that holds its neighbour's value lies far outside
    for i in range(4):
        assert abs(got[(i + 1) % 4] - want[i]) > 1000 * bound * want[i]


# ---- every GPU case on its branch ------------------------------------------------------------------------------------------------
def test_norm_packing_case_has_a_second_norm_launch_whose_slot_base_is_not_its_record_count():
    spec = tt.case_norm_packing()
    pl, ap = tt.plans_of(spec)
    assert len(spec) == 2 * CAP + 1 and sum(tt.in_norm(r) for r in spec) == CAP + 1
    assert pl["norm_launches"] == 2 and pl["update_launches"] == 3
    clipped = [r for r in spec if tt.in_norm(r)]
    slot0 = sum(-(-r["n"] // BLOCK) for r in clipped[:CAP])
    assert slot0 == CAP + 1 + 1 + 3 != CAP and pl["slots"] == slot0 + 1
    assert sorted(r["n"] for r in clipped[:CAP])[-3:] == [BLOCK + 1, 2 * BLOCK, 3 * BLOCK + 7]
    # the accumulate sweep: more than CAP AdamW records, and a clipped one with a slot base above 0 in its second launch
    adamw = [r for r in spec if r["kind"] == "adamw"]
    assert ap["acc_launches"] == 2 and len(adamw) > CAP and any(tt.in_norm(r) for r in adamw[CAP:])
    assert any(not tt.in_norm(r) for r in adamw[:CAP]) and any(not tt.in_norm(r) for r in adamw[CAP:])      # -1 in both launches
    assert {r["kind"] for r in spec} == {"adamw", "ema", "int"}
    assert any(r["kind"] == "ema" and r["clipped"] for r in spec)
    steps = [r["step_index"] for r in adamw]
    assert len(set(steps)) == len(steps) and steps != sorted(steps) and max(steps) < tt.N_STEPS["norm_packing"]


def test_empty_record_cases_meet_ot_find_everywhere():
    spec = tt.case_empty_records()
    n = [r["n"] for r in spec]
    assert n[0] == 0 and n[CAP - 1] == 0 and n[CAP] == 0 and n[-1] == 0 and n[-2] == 0 and n[20:23] == [0, 0, 0]
    assert n[1] > BLOCK and n[23] > BLOCK and n[CAP + 1] > BLOCK           # an empty record in front of a multi-workgroup one
    assert {spec[i]["kind"] for i in (20, 21, 22)} == {"adamw", "ema", "int"}
    pl, ap = tt.plans_of(spec)
    assert pl["update_launches"] == 2 and pl["norm_launches"] >= 1 and ap["acc_launches"] >= 1
    assert [int(b) for b, r in zip(pl["blocks"], spec) if r["n"] == 0] == [0] * 8
    lay = tt.layout(spec)
    assert all(v is None for r, row in zip(spec, lay["at"]) if r["n"] == 0 for v in row.values())
    # a launch of CAP empty records is not issued, in any sweep
    spec = tt.case_unissued_launch()
    pl, ap = tt.plans_of(spec)
    assert len(spec) == CAP + 1 and [r["n"] for r in spec] == [0] * CAP + [5]
    assert pl["update_launches"] == pl["norm_launches"] == ap["acc_launches"] == 1 and pl["slots"] == 1
    assert sum(tt.in_norm(r) for r in spec) == CAP + 1


def test_many_counters_case_takes_a_second_finish_launch():
    spec = tt.case_many_counters()
    pl, ap = tt.plans_of(spec)
    assert len(spec) == STEP_CAP + 1 and ap["finish_launches"] == 2
    assert tt.plans_of(spec[:-1])[1]["finish_launches"] == 1
    steps = [r["step_index"] for r in spec]
    assert len(set(steps)) == len(steps) and max(steps) < tt.N_STEPS_MANY and steps != sorted(steps)
    assert tt.N_STEPS_MANY - len(steps) == 6                # counters no record points at
    assert all(1 <= r["n"] <= 4 for r in spec)
    assert pl["update_launches"] == ap["acc_launches"] == -(-len(spec) // CAP) <= 24


def test_misaligned_case_takes_the_scalar_path_record_by_record():
    spec = tt.case_misaligned()
    pl, _ = tt.plans_of(spec)
    want = [int(not r["misalign"]) for r in spec]
    assert list(pl["vector"]) == want == tt.requested_alignment(spec)
    assert [sorted(r["misalign"]) for r in spec if r["kind"] == "adamw"] == [[k] if j == 0 else [] for k in tt.KEYS for j in (0, 1)]
    assert [sorted(r["misalign"]) for r in spec if r["kind"] == "ema"] == [["p"], [], ["t"], []]
    assert all(r["n"] == BLOCK + 1 for r in spec if r["kind"] == "adamw") and all(r["n"] == BLOCK + 3 for r in spec if r["kind"] == "ema")
    assert {r["group"] for r in spec if r["kind"] == "adamw"} == {0, 1, 2, 3}


def test_quad_tail_case_stays_on_the_vector_path():
    spec = tt.case_quad_tails()
    pl, _ = tt.plans_of(spec)
    assert list(pl["vector"]) == [1] * len(spec)
    for kind in ("adamw", "ema"):
        assert [r["n"] for r in spec if r["kind"] == kind] == list(range(BLOCK - 3, BLOCK + 4)) + [2 * BLOCK + 1, 2 * BLOCK + 2, 2 * BLOCK + 3]
    assert {r["teacher"] for r in spec if r["kind"] == "adamw"} == {True, False}
    assert {r["n"] % 4 for r in spec} == {0, 1, 2, 3}


def test_int64_case_goes_past_one_workgroup_and_past_the_first_launch():
    spec = tt.case_int64()
    pl, _ = tt.plans_of(spec)
    ints = [(i, r["n"]) for i, r in enumerate(spec) if r["kind"] == "int"]
    assert [n for _, n in ints] == [BLOCK - 1, BLOCK, BLOCK + 3, 2 * BLOCK + 1] and ints[-1][0] > CAP
    assert [int(pl["blocks"][i]) for i, _ in ints] == [1, 1, 2, 3] and all(pl["vector"][i] == 0 for i, _ in ints)
    assert pl["update_launches"] == 2


def test_window_case_is_the_norm_packing_table_with_a_sometimes_record():
    spec = tt.case_window()
    assert spec[:-1] == tt.case_norm_packing() and tt.in_norm(spec[tt.SOMETIMES]) and spec[tt.SOMETIMES]["n"] > BLOCK
    for g_null in ((), (tt.SOMETIMES,)):
        pl, ap = tt.plans_of(spec, g_null)
        assert pl["norm_launches"] == 2 and pl["update_launches"] == 3 and ap["acc_launches"] == 2 and ap["finish_launches"] == 1
    # one record's gradient is misaligned in every call: the accumulate sweep takes the scalar path there, and so must the
    # norm sweep it is held against
    assert [i for i, r in enumerate(spec) if "g" in r["misalign"]] == [8] and tt.plans_of(spec)[0]["vector"][8] == 0
    steps = [r["step_index"] for r in spec if r["kind"] == "adamw"]
    assert len(set(steps)) == len(steps) and max(steps) < tt.N_STEPS["window"]


def test_refusal_case_is_accepted_as_it_stands():
    spec = tt.case_refusals()
    pl, ap = tt.plans_of(spec)
    assert pl["slots"] == 3 and pl["update_launches"] == 1 and ap["finish_launches"] == 1
    assert {r["kind"] for r in spec} == {"adamw", "ema", "int"}


def test_optimtail_level_sizes():
    """STEP_CAP + 4 parameters: the un-gated finish stage takes two launches as well (OptimTail counts them itself)."""
    t = STEP_CAP + 4
    pl = ot.plan([1 + i % 3 for i in range(t)], [1] * t, [ot.CLIPPED] * t)
    ap = ot.acc_plan([1 + i % 3 for i in range(t)], [1] * t, [ot.CLIPPED] * t)
    assert ap["finish_launches"] == 2 == -(-t // STEP_CAP) and pl["update_launches"] == pl["norm_launches"] == -(-t // CAP)
