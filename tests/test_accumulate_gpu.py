"""step_per_update on the GPU (OptimTail(accumulate=k), csrc/optim_tail.hip "ABI 27"): A. a k-call window of the gated tail
against the existing step() fed with the sequentially fp32-summed gradient, bit for bit, and against the fp64 restatement of
tests/_optim_tail_ref.py started from that sum; B. one captured call replayed through whole windows; C. the steps --
SupervisedStep(step_per_update=k) and FixMatchNTMStep with cfg step_per_update, fused and in torch ops, eager and replayed."""
import numpy as np
import pytest
import torch

import _optim_tail_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BLOCK = ref.BLOCK
DECAY = 0.9
# the record set: the issue's element counts, then the record whose gradient starts one element into its storage (scalar
# path), 42 small records (50 records with a gradient in every call: the accumulate sweep takes a second launch), one
# parameter that never gets a gradient (a member of the student: an EMA-only record), one that gets one in call 2 of every 3 only
COUNTS = (1, 3, 4, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 5)
MISALIGNED = len(COUNTS)
FILL = 42
NEVER = MISALIGNED + 1 + FILL
SOMETIMES = NEVER + 1
SIZES = COUNTS + (BLOCK + 1,) + tuple(2 + i for i in range(FILL)) + (5, BLOCK + 4)


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Holder(torch.nn.Module):
    def __init__(self, params, floats, ints):
        super().__init__()
        for name, p in params:
            self.register_parameter(name, p)
        for i, b in enumerate(floats):
            self.register_buffer("running%d" % i, b)
        for i, b in enumerate(ints):
            self.register_buffer("count%d" % i, b)


class Rig:
    """52 parameters in two AdamW optimizers (weight decay / none), a clipped subset (i % 3 != 2) and an unclipped one, a
    teacher for i % 4 != 3, one float32 and one int64 buffer with a teacher.  Fresh optimizer state."""

    def __init__(self, hp=ref.EXAGGERATED_HP, accumulate=None, max_norm=1.0, seed=5):
        from geot_amd.optim_tail import OptimTail
        rng = np.random.default_rng(seed)
        self.params = [torch.nn.Parameter(_T(rng.standard_normal(n).astype(np.float32))) for n in SIZES]
        self.group = [i % 2 for i in range(len(SIZES))]
        self.clip = [i % 3 != 2 for i in range(len(SIZES))]
        self.groups = ref.groups_of(hp)
        named = [("p%d" % i, p) for i, p in enumerate(self.params) if i % 4 != 3]
        assert "p%d" % NEVER in dict(named)
        fb, ib = rng.standard_normal(37).astype(np.float32), rng.integers(0, 2 ** 40, 5).astype(np.int64)
        self.student = _Holder(named, [_T(fb)], [_T(ib)])
        self.teacher = _Holder([(n, torch.nn.Parameter(_T(rng.standard_normal(p.numel()).astype(np.float32)), requires_grad=False))
                                for n, p in named], [_T(rng.standard_normal(37).astype(np.float32))], [_T(np.zeros(5, np.int64))])
        self.opts = [torch.optim.AdamW([dict(self.groups[k], params=[p for p, g in zip(self.params, self.group) if g == k])],
                                       fused=True) for k in (0, 1)]
        self.max_norm = max_norm
        kw = {} if accumulate is None else {"accumulate": accumulate}
        self.tail = OptimTail(self.opts, clip_params=[p for p, c in zip(self.params, self.clip) if c] if max_norm is not None else None,
                              max_norm=max_norm, teacher=self.teacher, student=self.student, ema_decay=DECAY, **kw)

    @staticmethod
    def gradient(call, i, inf_at=None):
        """The gradient of parameter i in call `call` (None: it has none), as an fp32 array."""
        if i == NEVER or (i == SOMETIMES and call % 3 != 1):
            return None
        g = np.random.default_rng((call, i, 3)).standard_normal(SIZES[i]).astype(np.float32) * np.float32(1e-3 if i == 5 else 1.0)
        if inf_at is not None and inf_at[0] == call and inf_at[1] == i:
            g[inf_at[2]] = np.inf
        return g

    def put(self, i, g):
        """p.grad = g (a device tensor or None); the MISALIGNED record's starts one element into its storage."""
        p = self.params[i]
        if g is None:
            p.grad = None
        elif i == MISALIGNED:
            store = torch.empty(p.numel() + 1, dtype=torch.float32, device=DEV)
            p.grad = store[1:]
            p.grad.copy_(g)
            assert p.grad.data_ptr() % 16 == 4
        else:
            p.grad = g.clone()

    def set_grads(self, call, inf_at=None):
        for i in range(len(SIZES)):
            g = self.gradient(call, i, inf_at)
            self.put(i, None if g is None else _T(g))

    def drop_grads(self):
        for opt in self.opts:
            opt.zero_grad(set_to_none=True)

    def state(self):
        """Everything a tail may write, as device clones."""
        torch.cuda.synchronize()
        out = {}
        for i, p in enumerate(self.params):
            out["p%d" % i] = p.detach().clone()
            st = self.opts[self.group[i]].state.get(p, {})
            for k in ("exp_avg", "exp_avg_sq", "step"):
                if k in st:
                    out["%s%d" % (k, i)] = st[k].detach().clone()
        out.update({"t." + k: v.detach().clone() for k, v in self.teacher.state_dict().items()})
        out["total_norm"], out["coef"] = self.tail.total_norm.clone(), self.tail.clip_coef.clone()
        return out

    def records(self, sums):
        """The device state as the restatement's records, sums[i] the gradient (None: none) of parameter i."""
        out = []
        t_of = dict(self.teacher.named_parameters())
        for i, p in enumerate(self.params):
            t = t_of["p%d" % i].detach().cpu().numpy() if "p%d" % i in t_of else None
            if sums[i] is None:
                if t is not None:
                    out.append(dict(kind="ema", p=p.detach().cpu().numpy(), t=t, i=i))
                continue
            st = self.opts[self.group[i]].state.get(p, {})
            n = p.numel()
            out.append(dict(kind="adamw", p=p.detach().cpu().numpy(), g=sums[i].cpu().numpy(), group=self.group[i], i=i,
                            clipped=self.clip[i], step=int(st["step"].item()) if st else 0, t=t,
                            m=st["exp_avg"].cpu().numpy() if st else np.zeros(n, np.float32),
                            v=st["exp_avg_sq"].cpu().numpy() if st else np.zeros(n, np.float32)))
        s_b, t_b = dict(self.student.named_buffers()), dict(self.teacher.named_buffers())
        for name in s_b:
            out.append(dict(kind="int" if s_b[name].dtype == torch.int64 else "ema", p=s_b[name].cpu().numpy(),
                            t=t_b[name].cpu().numpy(), name=name))
        return out

    def check(self, before, want, what):
        """The state against the restatement's results and bounds; -> the worst error / bound."""
        t_of, t_b = dict(self.teacher.named_parameters()), dict(self.teacher.named_buffers())
        worst = 0.0
        for r, w in zip(before, want):
            if "name" in r:
                got = t_b[r["name"]].cpu().numpy()
                if w["kind"] == "int":
                    assert np.array_equal(got, w["t"]), (what, r["name"])
                else:
                    x = ref.ratio(got, w["t"], w["E_t"])
                    assert x <= 1.0, (what, r["name"], x)
                    worst = max(worst, x)
                continue
            i = r["i"]
            p = self.params[i]
            if w["kind"] == "adamw":
                st = self.opts[self.group[i]].state[p]
                assert int(st["step"].item()) == w["step"], (what, i)
                for got, key, e in ((p, "p", "E_p"), (st["exp_avg"], "m", "E_m"), (st["exp_avg_sq"], "v", "E_v")):
                    x = ref.ratio(got.detach().cpu().numpy(), w[key], w[e])
                    assert x <= 1.0, (what, i, key, x)
                    worst = max(worst, x)
            if w.get("t") is not None:
                x = ref.ratio(t_of["p%d" % i].detach().cpu().numpy(), w["t"], w["E_t"])
                assert x <= 1.0, (what, i, "t", x)
                worst = max(worst, x)
        return worst


def _same(a, b, what):
    assert set(a) == set(b), (what, sorted(set(a) ^ set(b)))
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, (what, len(bad), bad[:8])


def _unchanged(before, after, what):
    """Nothing that existed before has other bits; what is new (optimizer state created for the window's records) is zero."""
    _same(before, {k: after[k] for k in before}, what)
    assert all(float(v.abs().sum()) == 0.0 for k, v in after.items() if k not in before), what


def _window_sums(calls, inf_at=None):
    """((0 + g1) + g2) + ... in fp32 on the device, per parameter: what in-place accumulation gives.  None: no gradient."""
    sums = []
    for i in range(len(SIZES)):
        s = None
        for c in calls:
            g = Rig.gradient(c, i, inf_at)
            if g is not None:
                s = (torch.zeros(SIZES[i], dtype=torch.float32, device=DEV) if s is None else s) + _T(g)
        sums.append(s)
    return sums


# ---- A. the tail alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3])
def test_a_window_equals_one_step_fed_with_the_fp32_sum_and_the_calls_between_change_nothing(k):
    acc, one = Rig(accumulate=k), Rig()
    comp = Rig(accumulate=k)
    assert acc.tail.accumulator.numel() >= sum(SIZES) and acc.tail.window.dtype == torch.int32
    launches = set()
    for call in range(2 * k + 1):
        before = acc.state()
        acc.set_grads(call)
        acc.tail.step()
        acc.drop_grads()
        launches.add(acc.tail.launches)
        comp.set_grads(call)
        if (call + 1) % k:
            assert comp.tail.composite() is None
            _unchanged(before, acc.state(), ("inside a window", call))
            assert int(acc.tail.window) == (call + 1) % k
            continue
        window = range(call + 1 - k, call + 1)
        sums = _window_sums(window)
        assert (sums[SOMETIMES] is not None) == any(c % 3 == 1 for c in window) and sums[NEVER] is None
        recs, recs_c = one.records(sums), comp.records(sums)
        comp.tail.composite()
        _unchanged(one.state(), before, ("before the update", call))
        for i, s in enumerate(sums):
            one.put(i, s)
        one.tail.step()
        one.drop_grads()
        _same(one.state(), acc.state(), ("update", call))
        assert int(acc.tail.window) == 0
        # the fp64 restatement started from the fp32 sum: its operation-count bounds, unchanged, hold tail and composite
        want, norm, coef = ref.tail(recs, acc.groups, acc.max_norm, DECAY)
        assert coef < 0.5
        want_c = ref.tail(recs_c, acc.groups, acc.max_norm, DECAY)[0]
        print("k", k, "call", call, "worst error / bound:", acc.check(recs, want, ("fused", call)),
              comp.check(recs_c, want_c, ("composite", call)))
        assert abs(float(acc.tail.total_norm) - norm) <= ref.norm_error(ref.KERNEL_CHAIN) * norm
        assert abs(float(acc.tail.clip_coef) - coef) <= (ref.norm_error(ref.KERNEL_CHAIN) + 4 * ref.U) * coef
        comp.drop_grads()
    # 50 or 51 records in the accumulate sweep: two launches of it, one finish, two of the update sweep -- on every call
    assert launches == {5}, launches
    assert int(acc.tail.window) == 1 and float(acc.tail.accumulator.abs().sum()) > 0       # the last window stays open
    assert one.opts[0].state[one.params[0]]["step"].item() == 2.0


def test_k_1_is_the_tail_built_without_the_argument():
    a, b = Rig(accumulate=1), Rig()
    for call in range(2):
        for rig in (a, b):
            rig.set_grads(call)
            rig.tail.step()
            rig.drop_grads()
        assert a.tail.launches == b.tail.launches
    _same(a.state(), b.state(), "k = 1")
    assert a.tail.accumulator is None and a.tail.window is None
    a.tail.restart()                   # (nothing to restart, nothing issued)


def test_two_runs_give_the_same_bits():
    runs = []
    for _ in range(2):
        rig = Rig(accumulate=2)
        for call in range(5):
            rig.set_grads(call)
            rig.tail.step()
            rig.drop_grads()
        runs.append(dict(rig.state(), acc=rig.tail.accumulator.clone()))
    _same(runs[0], runs[1], "two runs")


@pytest.mark.parametrize("drop", [False, True])
def test_restart_keeps_the_sum_and_drop_clears_it(drop):
    """Two calls of a window of three, restart(), a whole window: the update holds five gradients (the window an epoch cut
    off joins the next one), or with drop=True the last three."""
    acc, one = Rig(accumulate=3), Rig()
    for call in range(2):
        acc.set_grads(call)
        acc.tail.step()
        acc.drop_grads()
    assert int(acc.tail.window) == 2
    acc.tail.restart(drop=drop)
    assert int(acc.tail.window) == 0 and (float(acc.tail.accumulator.abs().sum()) == 0.0) == drop
    for call in range(2, 5):
        before = acc.state()
        acc.set_grads(call)
        acc.tail.step()
        acc.drop_grads()
        if call < 4:
            _unchanged(before, acc.state(), ("inside the window", call))
    for i, s in enumerate(_window_sums(range(2, 5) if drop else range(5))):
        one.put(i, s)
    one.tail.step()
    _same(one.state(), acc.state(), "restart(drop=%s)" % drop)
    assert float(acc.tail.accumulator.abs().sum()) == 0.0


def test_an_infinite_gradient_inside_a_window_gives_the_composites_pattern_at_the_update():
    pats = []
    for fused in (True, False):
        rig = Rig(ref.REFERENCE_HP, accumulate=2)
        for call in range(2):
            rig.set_grads(call, inf_at=(0, 6, 5000))
            norm = rig.tail.step() if fused else rig.tail.composite()
            if fused:
                rig.drop_grads()
        assert float(norm) == float("inf")
        st = rig.state()
        pats.append({k: torch.isnan(v) for k, v in st.items() if v.is_floating_point() and k not in ("total_norm", "coef")})
    _same(pats[0], pats[1], "non-finite pattern")
    assert any(bool(v.any()) for v in pats[0].values()) and not all(bool(v.all()) for v in pats[0].values() if v.numel())


def test_the_accumulator_is_exchanged_on_update_calls_only():
    """sync.exchange(flat accumulator) between the accumulate sweep and the gated update: once per update; an exchange
    that leaves the sum as it is leaves the bits of a run without one."""
    class Sync:
        collectives = 0

        def exchange(self, flat):
            assert flat is rig.tail.accumulator
            self.collectives += 1
    rig, plain, sync = Rig(accumulate=2), Rig(accumulate=2), Sync()
    for call in range(5):
        for r in (rig, plain):
            r.set_grads(call)
        rig.tail.step(sync=sync)
        plain.tail.step()
        assert sync.collectives == (call + 1) // 2
    _same(rig.state(), plain.state(), "an exchange that changes nothing")


# ---- B. capture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3])
def test_replays_of_one_captured_call_equal_eager_calls_and_the_graph_is_kernels_only(k):
    from geot_amd import streams

    def rig_with_state():
        rig = Rig(ref.REFERENCE_HP, accumulate=k)
        rig.set_grads(0)
        rig.put(SOMETIMES, _T(Rig.gradient(1, SOMETIMES)))      # (the captured set is fixed: it has a gradient in every call)
        rig.tail.step()              # creates the state, not under capture; call 1 of the first window
        return rig
    eager = rig_with_state()
    for _ in range(2 * k + 1):
        eager.tail.step()
    rig = rig_with_state()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with streams.capture(graph, DEV):
        rig.tail.step()
    kinds = streams.node_types(graph)
    assert set(kinds) == {"kernel"} and kinds["kernel"] == rig.tail.launches == 5, kinds
    for _ in range(2 * k + 1):
        graph.replay()
    a, b = eager.state(), rig.state()
    a.update(acc=eager.tail.accumulator.clone(), window=eager.tail.window.clone())
    b.update(acc=rig.tail.accumulator.clone(), window=rig.tail.window.clone())
    _same(a, b, "replayed against eager")
    assert int(rig.tail.window) == (2 * k + 2) % k and float(rig.opts[1].state[rig.params[1]]["step"]) == (2 * k + 2) // k


def test_a_capture_that_finds_another_set_than_the_open_window_raises(monkeypatch):
    """Refused on the host before anything is issued (so the test needs no capture: it says that one is in progress)."""
    rig = Rig(accumulate=3)
    rig.set_grads(1)                 # SOMETIMES has a gradient: it belongs to the open window's update
    rig.tail.step()
    rig.set_grads(2)                 # ... and has none now
    before = rig.state()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="captured call fixes the parameters"):
        rig.tail.step()
    monkeypatch.undo()
    _same(before, rig.state(), "a refused call")
    rig.tail.step()                  # eagerly the open window takes the call
    assert int(rig.tail.window) == 2


# ---- C. the steps --------------------------------------------------------------------------------------------------------------
from test_fixmatch_phase2_gpu import SMALL, _batch, _new_step, _state      # noqa: E402
from test_fixmatch_phase2_gpu import _same as _same_state                   # noqa: E402


def _supervised(**kw):
    from geot_amd.openpoints.models.backbone.transformer import PointTransformer_seg_T
    from geot_amd.train_step import SupervisedStep
    torch.manual_seed(5)
    net = PointTransformer_seg_T(**SMALL).to(DEV)
    return SupervisedStep(net, **kw)


def _sup_state(step):
    out = {"model." + k: v.detach().clone() for k, v in step.model.state_dict().items()}
    for j, p in enumerate(pp for g in step.optimizer.param_groups for pp in g["params"]):
        for k, v in step.optimizer.state.get(p, {}).items():
            if torch.is_tensor(v):
                out["opt.%d.%s" % (j, k)] = v.detach().clone()
    return out


def _sampled(step, grads, stride_to=65536):
    """test_optim_tail_gpu._sampled_records with the window's summed gradients `grads` (parameter -> tensor)."""
    recs, total = [], torch.zeros((), dtype=torch.float64, device=DEV)
    opt = step.optimizer
    for gi, group in enumerate(opt.param_groups):
        for p in group["params"]:
            g = grads.get(p)
            if g is None:
                continue
            total += g.double().pow(2).sum()
            pick = slice(None, None, max(1, p.numel() // stride_to))
            st = opt.state.get(p) or {}
            take = lambda t: t.detach().reshape(-1)[pick].cpu().numpy()      # noqa: E731
            n = len(take(p))
            recs.append(dict(kind="adamw", p=take(p), g=take(g), group=gi, clipped=True, t=None, param=p, pick=pick,
                             step=int(st["step"].item()) if st else 0,
                             m=take(st["exp_avg"]) if st else np.zeros(n, np.float32),
                             v=take(st["exp_avg_sq"]) if st else np.zeros(n, np.float32)))
    return recs, float(total.sqrt())


def test_supervised_step_with_the_fused_window_against_the_torch_form():
    """Five calls with step_per_update=2 and grad_norm_clip=1: updates behind calls 2 and 4, held as
    test_optim_tail_gpu.test_supervised_step_with_the_fused_tail_against_the_composite holds an iteration -- each run within
    the restatement's bound E_p of its OWN state and summed gradient, and the two runs within E_p(fused) + E_p(torch) +
    |R_fused - R_torch| of each other.  Calls 1, 3 and 5 change no parameter."""
    from geot_amd import train_step as ts
    data, _ = _batch(3)
    res = {}
    for fused in (False, True):
        step = _supervised(grad_norm_clip=1.0, fused_tail=fused, step_per_update=2)
        torch.manual_seed(11)
        updates = []
        for call in range(5):
            loss = step.forward_loss(data["pos"], data["cls"], data["y"])
            loss.backward()
            params = [p for g in step.optimizer.param_groups for p in g["params"] if p.grad is not None]
            if fused:
                off = dict(zip((id(p) for p, _, _ in step.tail.params), step.tail._acc_offsets.tolist()))
                grads = {p: step.tail.accumulator[off[id(p)]:off[id(p)] + p.numel()].view_as(p) + p.grad for p in params}
            else:
                grads = {p: p.grad.clone() for p in params}
            recs, norm = _sampled(step, grads)
            before = _sup_state(step)
            ts._window_update(step, step.clip, step.model, fused)
            if call % 2 == 0:
                after = _sup_state(step)
                assert all(torch.equal(before[k], after[k]) for k in before if "num_batches" not in k), call
                continue
            updates.append((recs, norm, [r["param"].detach().reshape(-1)[r["pick"]].cpu().numpy() for r in recs]))
        res[fused] = updates
        groups = [dict(ref.REFERENCE_HP, weight_decay=g["weight_decay"]) for g in step.optimizer.param_groups]
        if fused:
            assert float(step.tail.total_norm) > 0 and int(step.tail.window) == 1
    for it in range(2):
        outs = {}
        for fused in (False, True):
            recs, norm, after = res[fused][it]
            out, _, coef = ref.tail(recs, groups, 1.0, None, norm=norm)
            assert coef < 1.0 and len(out) == len(after) > 50
            worst = max(ref.ratio(a, w["p"], w["E_p"]) for a, w in zip(after, out))
            print("update", it, "fused" if fused else "torch", "worst error / bound:", worst, "coef", coef)
            assert worst <= 1.0, (it, fused, worst)
            outs[fused] = (after, out)
        (pa, oa), (pb, ob) = outs[False], outs[True]
        if it == 0:
            assert all(np.array_equal(x["p"], y["p"]) for x, y in zip(oa, ob))          # the same inputs: the same R
        cross = max(ref.ratio(b, a, x["E_p"] + y["E_p"] + np.abs(x["p"] - y["p"])) for a, b, x, y in zip(pa, pb, oa, ob))
        print("update", it, "fused against torch, worst difference / bound:", cross)
        assert cross <= 1.0, (it, cross)


@pytest.mark.parametrize("fused", [False, True])
def test_fixmatch_step_updates_and_moves_the_teacher_on_every_second_call(fused):
    """cfg step_per_update=2 with a clip and ema_teacher, five calls: calls 1, 3 and 5 leave student, optimizers and teacher
    alone; behind calls 2 and 4 the teacher is d t + (1 - d) s within the EMA's bound of _optim_tail_ref.py."""
    from geot_amd import train_step as ts
    cfg = dict(ts.NTM_CFG, threed_k=8, ema_teacher=True, fused_tail=fused, grad_norm_clip=1.0, step_per_update=2)
    step = _new_step(cfg)
    data, data_u = _batch(3)
    torch.manual_seed(11)
    d = cfg["ema_decay"]
    for call in range(5):
        t0 = {k: v.detach().clone() for k, v in step.model_t.state_dict().items()}
        s0 = _state(step)
        losses = step(data, data_u)
        torch.cuda.synchronize()
        assert ("grad_norm" in losses) == fused and all(torch.isfinite(v).all() for v in losses.values())
        s_sd, t_sd = step.model.state_dict(), step.model_t.state_dict()
        if call % 2 == 0:
            s1 = _state(step)
            # (BatchNorm's running statistics move with every forward; parameters and optimizer state do not)
            names = {n for n, _ in step.model.named_parameters()} | {n for n, _ in step.T_predictor.named_parameters()}
            same = [k for k in s0 if k.startswith("opt") or ("." in k and k.split(".", 1)[1] in names)]
            assert len(same) > 50 and all(torch.equal(s0[k], s1[k]) for k in same), call
            assert all(torch.equal(t_sd[k], t0[k]) for k in t_sd), call
            continue
        moved = 0
        for name, t in t_sd.items():
            s = s_sd[name]
            if t.dtype == torch.int64:
                assert torch.equal(t, s), name
                continue
            a, b, c = t0[name].double().cpu().numpy(), s.double().cpu().numpy(), t.double().cpu().numpy()
            want = d * a + (1 - d) * b
            bound = 2 * ref.U * d * np.abs(a) + 3 * ref.U * (1 - d) * (np.abs(b) + np.abs(a)) + ref.U * np.abs(want)
            assert ref.ratio(c, want, bound) <= 1.0, (call, name)
            moved += int(not torch.equal(t, t0[name]))
        assert moved > len(t_sd) // 2, (call, moved)
    if fused:
        assert int(step.tail.window) == 1


EPOCHS = [50, 50, 50, 51, 51, 51]      # warmup=1: each phase runs eagerly once, is captured and replayed; k = 2 windows span both


def test_graphed_fixmatch_equals_eager_across_the_switch_with_k_2():
    from geot_amd import train_step as ts, graph_step as gs
    cfg = dict(ts.NTM_CFG, threed_k=8, ema_teacher=True, fused_tail=True, grad_norm_clip=1.0, step_per_update=2)
    batches = [_batch(3), _batch(400)]
    runs = {}
    for mode in ("eager", "graph"):
        step = _new_step(cfg)
        call = gs.GraphedFixMatchStep(step, warmup=1) if mode == "graph" else step
        torch.manual_seed(11)
        out = []
        for i, epoch in enumerate(EPOCHS):
            call.set_epoch(epoch)
            cur, nxt = batches[i % 2], batches[(i + 1) % 2]
            res = call(cur[0], cur[1], next_batches=nxt)
            out.append({k: v.clone() for k, v in res.items()})
        torch.cuda.synchronize()
        if mode == "graph":
            # the graphs of k = 1: a P and an M per phase, kernel nodes only
            assert set(call.graphs) == {"P@e", "M@e", "P@2", "M@2"}, sorted(call.graphs)
            assert all(set(call.node_types[k]) == {"kernel"} for k in call.graphs), call.node_types
        state = _state(step)
        state.update({"teacher." + k: v.detach().clone() for k, v in step.model_t.state_dict().items()})
        state.update(acc=step.tail.accumulator.clone(), window=step.tail.window.clone())
        runs[mode] = (out, state)
    for i, (a, b) in enumerate(zip(runs["eager"][0], runs["graph"][0])):
        assert set(a) == set(b) and "grad_norm" in a
        for k in a:
            assert torch.equal(a[k], b[k]), (i, k, float(a[k]), float(b[k]))
    _same_state(runs["eager"][1], runs["graph"][1], "graph against eager")
    # calls 1 2 | 3 (epoch 51 restarts the count, the sum stays) 4 5 | 6: two updates, the second with three gradients
    assert int(runs["graph"][1]["window"]) == 1
    assert max(float(v) for k, v in runs["graph"][1].items() if k.endswith(".step")) == 2.0


def test_graphed_supervised_equals_eager_with_k_2():
    from geot_amd import graph_step as gs
    batches = [_batch(3)[0], _batch(400)[0]]
    runs = {}
    for mode in ("eager", "graph"):
        step = _supervised(grad_norm_clip=1.0, fused_tail=True, step_per_update=2)
        call = gs.GraphedSupervisedStep(step, warmup=1) if mode == "graph" else step
        torch.manual_seed(11)
        out = []
        for i, epoch in enumerate(EPOCHS):
            if i and epoch != EPOCHS[i - 1]:
                step.new_epoch()
            cur, nxt = batches[i % 2], batches[(i + 1) % 2]
            out.append(call(cur["pos"], cur["cls"], cur["y"], next_pos=nxt["pos"]).clone())
        torch.cuda.synchronize()
        if mode == "graph":
            assert all(set(call.node_types[k]) == {"kernel"} for k in call.graphs) and len(call.graphs) == 2, call.node_types
        runs[mode] = (out, dict(_sup_state(step), acc=step.tail.accumulator.clone(), window=step.tail.window.clone()))
    for i, (a, b) in enumerate(zip(runs["eager"][0], runs["graph"][0])):
        assert torch.equal(a, b), (i, float(a), float(b))
    _same_state(runs["eager"][1], runs["graph"][1], "graph against eager")
    assert int(runs["graph"][1]["window"]) == 1
    assert max(float(v) for k, v in runs["graph"][1].items() if k.endswith(".step")) == 2.0


def test_wrapping_a_k_2_step_without_the_fused_tail_raises():
    from geot_amd import train_step as ts, graph_step as gs
    with pytest.raises(RuntimeError, match="fused_tail"):
        gs.GraphedSupervisedStep(_supervised(step_per_update=2))
    with pytest.raises(RuntimeError, match="fused_tail"):
        gs.GraphedFixMatchStep(_new_step(dict(ts.NTM_CFG, threed_k=8, ema_teacher=True, step_per_update=2)))


def test_step_per_update_1_is_the_step_built_without_the_key():
    from geot_amd import train_step as ts
    batches = [_batch(3), _batch(400)]
    runs = []
    for with_key in (True, False):
        cfg = dict(ts.NTM_CFG, threed_k=8, grad_norm_clip=1.0, fused_tail=True)
        if not with_key:
            del cfg["step_per_update"]
        step = _new_step(cfg)
        assert step.step_per_update == 1 and step.tail.accumulator is None
        torch.manual_seed(11)
        for i in range(2):
            step.set_epoch(50 + i)
            step(*batches[i])
        torch.cuda.synchronize()
        runs.append(dict(_state(step), norm=step.tail.total_norm.clone()))
    _same_state(runs[0], runs[1], "step_per_update=1")
    sup = [_supervised(grad_norm_clip=1.0, fused_tail=True, **kw) for kw in ({"step_per_update": 1}, {})]
    for step in sup:
        torch.manual_seed(11)
        for i in range(2):
            step(batches[i][0]["pos"], batches[i][0]["cls"], batches[i][0]["y"])
            step.new_epoch()
        assert step.tail.accumulator is None
    _same_state(_sup_state(sup[0]), _sup_state(sup[1]), "SupervisedStep(step_per_update=1)")
