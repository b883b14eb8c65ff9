"""The optimizer tail's kernels at every table and launch branch (csrc/optim_tail.hip), driven through hand-built record tables
in guarded arenas (tests/_optim_tail_table.py) against the fp64 restatement of tests/_optim_tail_ref.py within its counted
bounds.  tests/test_optim_tail_table_cpu.py proves, through the library's planners, that each case sits on the branch it is
named after.  Every updating sequence is held to the same checks (_check): p, m, v, t within E_p, E_m, E_v, E_t; the step
counters exactly; total_norm and coef within norm_error(KERNEL_CHAIN); every slot within slot_error(KERNEL_CHAIN) of the fp64
sum of its own stretch; every guard element, every guard slot and every student tensor bit for bit as it was."""
import numpy as np
import pytest
import torch

import _optim_tail_ref as ref
import _optim_tail_table as tt

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CAP, BLOCK, STEP_CAP = tt.CAP, tt.BLOCK, tt.STEP_CAP
E_NORM = ref.norm_error(ref.KERNEL_CHAIN)
E_SLOT = ref.slot_error(ref.KERNEL_CHAIN)
SEED = {name: 100 + i for i, name in enumerate(sorted(tt.CASES))}


def _table(name, **kw):
    return tt.Table(tt.CASES[name](), seed=SEED[name], n_steps=tt.N_STEPS.get(name), dev=DEV, **kw)


def _grads(arrays):
    return [a["g"] for a in arrays["rec"]]


def _state_bits_equal(a, b, keys=("rec", "steps", "scalars")):
    """The names of what differs between two readbacks, bit for bit."""
    bad = []
    for key in keys:
        if key == "rec":
            for i, (x, y) in enumerate(zip(a["rec"], b["rec"])):
                bad += ["rec %d %s" % (i, k) for k in tt.KEYS if (x[k] is None) != (y[k] is None)
                        or (x[k] is not None and not tt.same_bits(x[k], y[k]))]
        elif not tt.same_bits(a[key], b[key]):
            bad.append(key)
    return bad


def _check(what, tab, before, after, grads, max_norm, decay=tt.DECAY, clipping=True):
    """An updating sequence ran between `before` and `after` with `grads` as the gradients -> (the worst error / bound, where it
    is)."""
    spec = tab.spec
    assert before["guards_intact"], (what, before["guard_faults"])
    assert after["guards_intact"], (what, after["guard_faults"])            # arenas, steps, scalars, guard slots, gate, accumulator
    recs = tt.to_ref_records(spec, before, grads)
    want, norm, coef = ref.tail(recs, tab.groups, max_norm, decay, chain=ref.KERNEL_CHAIN)
    worst = (0.0, "-")
    steps = before["steps"].copy()
    for i, (r, b, a, w) in enumerate(zip(spec, before["rec"], after["rec"], want)):
        if r["kind"] == "adamw":
            steps[r["step_index"]] += 1
            assert tt.same_bits(a["g"], b["g"]), (what, i, "g was written")
            for key, e in (("p", "E_p"), ("m", "E_m"), ("v", "E_v")) + ((("t", "E_t"),) if r["teacher"] else ()):
                x = ref.ratio(a[key], w[key], w[e])
                assert x <= 1.0, (what, i, key, x, r)
                worst = max(worst, (x, "%s of record %d" % (key, i)))
            continue
        assert tt.same_bits(a["p"], b["p"]), (what, i, "a student tensor was written")
        if r["kind"] == "int":
            assert np.array_equal(a["t"], b["p"]), (what, i, "int64 copy")
        else:
            x = ref.ratio(a["t"], w["t"], w["E_t"])
            assert x <= 1.0, (what, i, "t", x, r)
            worst = max(worst, (x, "t of record %d" % i))
    assert np.array_equal(after["steps"], steps), (what, "step counters", np.flatnonzero(after["steps"] != steps)[:8])
    if max_norm is None:
        assert tuple(after["scalars"]) == (0.0, 1.0), (what, after["scalars"])
        return worst
    if clipping:
        assert coef < 0.5, (what, coef)
    total, got_coef = float(after["scalars"][0]), float(after["scalars"][1])
    assert abs(total - norm) <= E_NORM * norm, (what, total, norm)
    assert abs(got_coef - coef) <= (E_NORM + 4 * ref.U) * coef, (what, got_coef, coef)
    slots = tt.expected_slots(spec, grads)
    assert after["slots"].shape == slots.shape, (what, after["slots"].shape, slots.shape)
    x = ref.ratio(after["slots"], slots, E_SLOT * slots)
    assert x <= 1.0, (what, "slots", x, np.flatnonzero(np.abs(after["slots"] - slots) > E_SLOT * slots)[:8])
    return max(worst, (x, "a slot"), (abs(total - norm) / (E_NORM * norm) if norm else 0.0, "total_norm"))


def _run(name, form, max_norm=1.0, clipping=True):
    tab = _table(name)
    spec = tab.spec
    assert list(tab.aligned_now()) == tt.requested_alignment(spec)
    assert list(tab.plan["vector"]) == [int(a and r["kind"] != "int") for a, r in zip(tt.requested_alignment(spec), spec)]
    before = tab.read()
    if form == "ungated":
        tab.ungated(max_norm)
    else:
        tab.gated(1, max_norm)             # a window of one call: the gated kernels, updating at once
    after = tab.read()
    worst = _check((name, form), tab, before, after, _grads(before), max_norm, clipping=clipping)
    if form == "gated":
        assert tuple(after["gate"]) == (0, 1) and not after["acc"].view(np.uint32).any()
    print(name, form, "worst error / bound: %.3f (%s)" % worst)
    assert worst[0] <= 1.0
    return tab, before, after


FORMS = ["ungated", "gated"]


# ---- 1, 2, 4, 5, 6: one call, either form --------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_norm_sweep_packed_otherwise_than_the_update_sweep(form):
    """A second norm launch of one record whose first slot is 53, not 48; gated: the global slot base of the accumulate
    sweep's second launch, and -1 for the unclipped records of both."""
    tab, _, after = _run("norm_packing", form)
    assert tab.plan["norm_launches"] == 2 and tab.plan["update_launches"] == 3 and after["slots"].size == CAP + 6


@pytest.mark.parametrize("form", FORMS)
def test_empty_records_wherever_ot_find_meets_them(form):
    _run("empty_records", form)


@pytest.mark.parametrize("form", FORMS)
def test_a_launch_of_empty_records_is_not_issued(form):
    tab, _, after = _run("unissued_launch", form)
    assert tab.plan["update_launches"] == 1 and after["slots"].size == 1
    assert np.array_equal(after["steps"], [r["step0"] + 1 for r in sorted(tab.spec, key=lambda r: r["step_index"])])


@pytest.mark.parametrize("form", FORMS)
def test_each_pointer_misaligned_alone_takes_the_scalar_loops(form):
    tab, _, _ = _run("misaligned", form)
    assert list(tab.plan["vector"]) == [int(not r["misalign"]) for r in tab.spec] and 0 < sum(tab.plan["vector"]) < len(tab.spec)


@pytest.mark.parametrize("form", FORMS)
def test_quad_tails_write_nothing_past_a_tensors_end(form):
    tab, _, _ = _run("quad_tails", form)
    assert all(tab.plan["vector"])


@pytest.mark.parametrize("form", FORMS)
def test_int64_records_past_one_workgroup_are_copied_exactly(form):
    tab, before, after = _run("int64", form)
    for r, b, a in zip(tab.spec, before["rec"], after["rec"]):
        if r["kind"] == "int":
            assert int(b["p"].min()) > 2 ** 40 and np.array_equal(a["t"], b["p"]) and not np.array_equal(b["t"], b["p"])


@pytest.mark.parametrize("name", ["norm_packing", "misaligned"])
def test_a_max_norm_above_the_norm_reproduces_the_unclipped_bits(name):
    runs = []
    for max_norm in (2e6, None):
        tab, _, after = _run(name, "ungated", max_norm, clipping=False)
        runs.append(after)
    assert float(runs[0]["scalars"][1]) == 1.0 and float(runs[0]["scalars"][0]) > 1.0
    assert _state_bits_equal(runs[0], runs[1], keys=("rec", "steps")) == []


# ---- 3: more step counters than one finish launch --------------------------------------------------------------------------------
def test_a_second_finish_launch_raises_the_last_counter():
    tab, before, after = _run("many_counters", "ungated")
    used = sorted(r["step_index"] for r in tab.spec)
    unused = sorted(set(range(tab.n_steps)) - set(used))
    assert len(used) == STEP_CAP + 1 and len(unused) == 6
    assert np.all(after["steps"][unused] == tt.UNUSED_STEP) and np.all(after["steps"][used] == before["steps"][used] + 1)


def test_the_second_gated_finish_launch_follows_the_flag():
    """k = 2: call 1 changes no counter, scalar or parameter through either finish launch; call 2 changes all of them."""
    name = "many_counters"
    tab = _table(name)
    spec = tab.spec
    assert tab.acc_plan_now()["finish_launches"] == 2
    start = tab.read()
    g1 = _grads(start)
    tab.gated(2)
    mid = tab.read()
    assert mid["guards_intact"], mid["guard_faults"]
    assert _state_bits_equal(start, mid) == [] and tuple(mid["gate"]) == (1, 0)
    assert tt.same_bits(mid["acc"], tt.acc_expected(spec, tab.offsets, tab.n_acc, g1))
    g2 = [a.get("g") for a in tt.make_inputs(spec, SEED[name], call=1)]
    tab.set_grads(g2)
    before = tab.read()
    assert _state_bits_equal(mid, before, keys=("steps", "scalars")) == []
    tab.gated(2)
    after = tab.read()
    sums = [None if a is None else (np.zeros_like(a) + a) + b for a, b in zip(g1, g2)]
    worst = _check(name, tab, before, after, sums, 1.0)
    assert tuple(after["gate"]) == (0, 1) and not after["acc"].view(np.uint32).any()
    changed = [i for i, (b, a) in enumerate(zip(before["rec"], after["rec"])) if not tt.same_bits(a["p"], b["p"])]
    assert len(changed) == len(spec)
    print(name, "gated k=2 worst error / bound: %.3f (%s)" % worst)


# ---- 7: the gated window in full -------------------------------------------------------------------------------------------------
def test_a_window_of_three_over_seven_calls():
    """Inside a window only the accumulator and gate[0] change, and the accumulator is the sequential fp32 sum, bit for bit.
    An update leaves the accumulator zero, lies within the bounds of the restatement started from the fp32 sum, and has the
    bits of the un-gated sequence fed with that sum in a twin table -- its norm slots included: the accumulate sweep of the
    update call writes what geot_optim_tail_norm writes for the summed gradient stored with that call's alignment."""
    name, k = "window", 3
    tab, twin = _table(name), _table(name)
    spec = tab.spec
    sums = [None] * len(spec)
    updates = 0
    for call in range(7):
        grads = [a.get("g") for a in tt.make_inputs(spec, SEED[name], call=call)]
        g_null = () if call % 3 == 1 else (tt.SOMETIMES,)
        tab.set_grads(grads)
        before = tab.read()
        pl = tab.gated(k, g_null=g_null)
        assert pl["acc_launches"] == 2 and pl["update_launches"] == 3 and pl["finish_launches"] == 1
        after = tab.read()
        for i, g in enumerate(grads):
            if g is not None and i not in g_null:
                sums[i] = (np.zeros_like(g) if sums[i] is None else sums[i]) + g
        if (call + 1) % k:
            assert after["guards_intact"], (call, after["guard_faults"])
            assert _state_bits_equal(before, after) == [], call
            assert tuple(after["gate"]) == ((call + 1) % k, 0)
            assert tt.same_bits(after["acc"], tt.acc_expected(spec, tab.offsets, tab.n_acc, sums)), call
            continue
        assert all(s is not None for s, r in zip(sums, spec) if r["kind"] == "adamw")
        worst = _check((name, call), tab, before, after, sums, 1.0)
        assert tuple(after["gate"]) == (0, 1) and not after["acc"].view(np.uint32).any()
        print(name, "call", call, "worst error / bound: %.3f (%s)" % worst)
        twin.set_grads(sums)
        t_before = twin.read()
        assert _state_bits_equal(before, t_before, keys=("steps", "scalars")) == []
        assert all(tt.same_bits(x[key], y[key]) for x, y in zip(before["rec"], t_before["rec"]) for key in "pmvt" if x[key] is not None)
        twin.ungated(1.0)
        t_after = twin.read()
        assert _state_bits_equal(t_after, after, keys=("steps", "scalars", "slots")) == []
        bad = [(i, key) for i, (x, y) in enumerate(zip(after["rec"], t_after["rec"])) for key in "pmvt"
               if x[key] is not None and not tt.same_bits(x[key], y[key])]
        assert bad == [], bad[:8]
        sums = [None] * len(spec)
        updates += 1
    assert updates == 2 and tuple(after["gate"]) == (1, 0)


# ---- 8: refusals that return before any launch -----------------------------------------------------------------------------------
def _entries(tab, table, n_steps=None, n_groups=4, decay=tt.DECAY, n_slots=None, acc=None, n_acc=None):
    t, host, aux, gt = len(table), table.ctypes.data, tab.aux, tab.group_table
    n_steps = tab.n_steps if n_steps is None else n_steps
    n_slots = tab.plan["slots"] if n_slots is None else n_slots
    acc = tab.acc.ptr("acc") if acc is None else acc
    n_acc = tab.n_acc if n_acc is None else n_acc
    slots, steps, scalars, gate, offs = aux.ptr("slots"), aux.ptr("steps"), aux.ptr("scalars"), tab.gate.ptr("gate"), tab.offs.data_ptr()
    return {"norm": ("geot_optim_tail_norm", t, host, slots, n_slots),
            "finish": ("geot_optim_tail_finish", t, host, 1, n_slots, slots, 1.0, steps, n_steps, scalars),
            "update": ("geot_optim_tail_update", t, host, n_groups, gt.ctypes.data, scalars, steps, n_steps, decay),
            "accumulate": ("geot_optim_tail_accumulate", t, host, acc, offs, n_acc, n_steps, slots, n_slots),
            "acc_finish": ("geot_optim_tail_acc_finish", t, host, 1, n_slots, slots, 1.0, steps, n_steps, scalars, gate, 2),
            "acc_update": ("geot_optim_tail_acc_update", t, host, n_groups, gt.ctypes.data, scalars, steps, n_steps, decay, acc, offs,
                           n_acc, gate)}


def _set(field, row, value):
    def change(tab, table):
        table[field][row] = value
        return {}
    return change


REFUSALS = {        # what is wrong -> (the change, the entry points that must refuse it)
    "a duplicate step index": (_set("step", 4, 1), ("finish", "acc_finish")),
    "a step index at n_steps": (_set("step", 0, 3), ("finish", "update", "accumulate", "acc_finish", "acc_update")),
    "a step index above n_steps": (_set("step", 4, 1000), ("finish", "update", "accumulate", "acc_finish", "acc_update")),
    "a group at n_groups": (lambda tab, table: {"n_groups": 3}, ("update", "acc_update")),
    "a group above every table": (_set("group", 2, 4), ("norm", "update", "accumulate", "acc_update")),
    "ema_decay 1.0": (lambda tab, table: {"decay": 1.0}, ("update", "acc_update")),
    "ema_decay NaN": (lambda tab, table: {"decay": float("nan")}, ("update", "acc_update")),
    "n_slots below the plan's": (lambda tab, table: {"n_slots": tab.plan["slots"] - 1}, ("norm", "accumulate")),
    "an accumulator off 16 bytes": (lambda tab, table: {"acc": tab.acc.ptr("acc") + 4}, ("accumulate", "acc_update")),
    "a record longer than n_acc": (lambda tab, table: {"n_acc": BLOCK}, ("accumulate", "acc_update")),
    "a null g in the un-gated form": (_set("g", 0, 0), ("norm", "update")),
}


@pytest.mark.parametrize("wrong", sorted(REFUSALS))
def test_a_refused_call_writes_nothing(wrong):
    """Host-side argument checks: each raises from call() before any launch, and everything is bit for bit as it was; the
    table as it stands then runs."""
    from geot_amd.ext._common import call
    tab = _table("refusals")
    assert tab.n_steps == 3 and tab.spec[2]["group"] == 3 and tab.spec[2]["n"] > BLOCK
    before = tab.read()
    change, refusing = REFUSALS[wrong]
    table = tab.table.copy()
    entries = _entries(tab, table, **change(tab, table))
    for entry in refusing:
        with pytest.raises(RuntimeError, match=entries[entry][0]):
            call(entries[entry][0], DEV, *entries[entry][1:])
    after = tab.read()
    assert after["guards_intact"], after["guard_faults"]
    assert _state_bits_equal(before, after, keys=("rec", "steps", "scalars", "slots", "gate", "acc")) == []
    tab.ungated(1.0)
    assert _check(wrong, tab, before, tab.read(), _grads(before), 1.0)[0] <= 1.0


# ---- 9: OptimTail over more parameters than one finish launch takes --------------------------------------------------------------
N_PARAMS = STEP_CAP + 4


class _Holder(torch.nn.Module):
    def __init__(self, params):
        super().__init__()
        for i, p in enumerate(params):
            self.register_parameter("p%d" % i, p)


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Rig:
    """N_PARAMS parameters of one to three elements in two AdamW optimizers (three groups), a teacher for every one, three
    in four clipped."""

    def __init__(self, accumulate):
        from geot_amd.optim_tail import OptimTail
        rng = np.random.default_rng(77)
        self.sizes = [1 + i % 3 for i in range(N_PARAMS)]
        self.params = [torch.nn.Parameter(_T(rng.standard_normal(n).astype(np.float32))) for n in self.sizes]
        self.teach = [torch.nn.Parameter(_T(rng.standard_normal(n).astype(np.float32)), requires_grad=False) for n in self.sizes]
        self.student, self.teacher = _Holder(self.params), _Holder(self.teach)
        self.groups = [tt.GROUPS[0], tt.GROUPS[1], tt.GROUPS[3]]
        member = lambda k: [p for i, p in enumerate(self.params) if i % 3 == k]      # noqa: E731
        self.opts = [torch.optim.AdamW([dict(self.groups[0], params=member(0)), dict(self.groups[1], params=member(1))], fused=True),
                     torch.optim.AdamW([dict(self.groups[2], params=member(2))], fused=True)]
        self.clip = [i % 4 != 3 for i in range(N_PARAMS)]
        self.tail = OptimTail(self.opts, clip_params=[p for p, c in zip(self.params, self.clip) if c], max_norm=1.0,
                              teacher=self.teacher, student=self.student, ema_decay=tt.DECAY, accumulate=accumulate)
        index = {id(p): i for i, p in enumerate(self.params)}
        self.order = [index[id(p)] for p, _, _ in self.tail.params]                 # the table's order: group by group

    def set_grads(self, call):
        rng = np.random.default_rng((78, call))
        grads = [rng.standard_normal(n).astype(np.float32) for n in self.sizes]
        for p, g in zip(self.params, grads):
            p.grad = _T(g)
        return grads

    def snapshot(self, grads):
        """The device state as the restatement's records, in the table's order, from a handful of transfers."""
        def flat(ts):
            return torch.cat([t.detach().reshape(-1) for t in ts]).cpu().numpy()
        state = [self.opts[0 if i % 3 < 2 else 1].state.get(p, {}) for i, p in enumerate(self.params)]
        zeros = [torch.zeros_like(p) for p in self.params]
        p, t = flat(self.params), flat(self.teach)
        m = flat([s["exp_avg"] if s else z for s, z in zip(state, zeros)])
        v = flat([s["exp_avg_sq"] if s else z for s, z in zip(state, zeros)])
        step = flat([s["step"] if s else z[:1].sum() for s, z in zip(state, zeros)])
        cut = np.cumsum([0] + self.sizes)
        recs = [dict(kind="adamw", p=p[cut[i]:cut[i + 1]], g=grads[i], m=m[cut[i]:cut[i + 1]], v=v[cut[i]:cut[i + 1]],
                     t=t[cut[i]:cut[i + 1]], group=i % 3, clipped=self.clip[i], step=int(step[i])) for i in range(N_PARAMS)]
        return [recs[i] for i in self.order]

    def check(self, what, before, grads_used):
        after = self.snapshot(grads_used)
        want, norm, coef = ref.tail(before, self.groups, 1.0, tt.DECAY, chain=ref.KERNEL_CHAIN)
        assert coef < 0.5
        worst = 0.0
        for i, (a, w) in enumerate(zip(after, want)):
            assert a["step"] == w["step"], (what, i)
            for key, e in (("p", "E_p"), ("m", "E_m"), ("v", "E_v"), ("t", "E_t")):
                x = ref.ratio(a[key], w[key], w[e])
                assert x <= 1.0, (what, i, key, x)
                worst = max(worst, x)
        total = float(self.tail.total_norm)
        assert abs(total - norm) <= E_NORM * norm and abs(float(self.tail.clip_coef) - coef) <= (E_NORM + 4 * ref.U) * coef
        print("OptimTail", what, "worst error / bound:", worst)

    def captured_kernels(self):
        """The kernel nodes of one captured step(): the launches that are really issued."""
        from geot_amd import streams
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with streams.capture(graph, DEV):
            self.tail.step()
        kinds = streams.node_types(graph)
        assert set(kinds) == {"kernel"}, kinds
        return kinds["kernel"]


def _plans_of_rig(rig):
    from geot_amd import optim_tail as ot
    counts = [rig.sizes[i] for i in rig.order]
    flags = [ot.CLIPPED if rig.clip[i] else 0 for i in rig.order]
    return ot.plan(counts, [1] * N_PARAMS, flags), ot.acc_plan(counts, [1] * N_PARAMS, flags)


def test_optimtail_over_more_parameters_than_one_finish_launch_takes():
    rig = _Rig(1)
    pl, ap = _plans_of_rig(rig)
    assert ap["finish_launches"] == 2 and pl["norm_launches"] == -(-sum(rig.clip) // CAP) < pl["update_launches"]
    for call in range(2):
        grads = rig.set_grads(call)
        before = rig.snapshot(grads)
        assert all(r["step"] == call for r in before)
        rig.tail.step()
        rig.check("step %d" % call, before, grads)
        assert rig.tail.launches == pl["norm_launches"] + ap["finish_launches"] + pl["update_launches"], rig.tail.launches
    assert rig.captured_kernels() == rig.tail.launches


def test_optimtail_window_over_more_parameters_than_one_finish_launch_takes():
    rig = _Rig(2)
    pl, ap = _plans_of_rig(rig)
    want_launches = ap["acc_launches"] + ap["finish_launches"] + ap["update_launches"]
    assert ap["finish_launches"] == 2 and ap["acc_launches"] == ap["update_launches"] == -(-N_PARAMS // CAP)
    g1 = rig.set_grads(0)
    start = rig.snapshot(g1)
    rig.tail.step()
    assert rig.tail.launches == want_launches and int(rig.tail.window) == 1
    g2 = rig.set_grads(1)
    sums = [(np.zeros_like(a) + a) + b for a, b in zip(g1, g2)]
    before = rig.snapshot(sums)
    for a, b in zip(start, before):                      # call 1 of the window: through both finish launches, nothing moved
        assert a["step"] == b["step"] == 0 and all(tt.same_bits(a[k], b[k]) for k in "pmvt")
    rig.tail.step()
    assert rig.tail.launches == want_launches and int(rig.tail.window) == 0
    rig.check("window of 2", before, sums)
    assert rig.captured_kernels() == want_launches
