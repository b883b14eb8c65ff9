"""The fused tail of an iteration on the GPU (geot_amd/optim_tail.py, csrc/optim_tail.hip): A. the tail alone against the fp64
restatement of tests/_optim_tail_ref.py within its derived bounds; B. three replays of a captured tail against three eager
calls; C. the steps -- SupervisedStep(fused_tail=True), FixMatchNTMStep with cfg ema_teacher / fused_tail, eager and replayed
from hipGraphs across switch_ep, and the switches off against a step built without the keys."""
import copy

import numpy as np
import pytest
import torch

import _optim_tail_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HPS = {"reference": ref.REFERENCE_HP, "exaggerated": ref.EXAGGERATED_HP}
DECAY = 0.9
MISALIGNED = 6          # the record (BLOCK + 1 elements) whose gradient starts one element into its storage


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Holder(torch.nn.Module):
    """Named parameters and buffers, as a model holds them."""

    def __init__(self, params, floats, ints):
        super().__init__()
        for name, p in params:
            self.register_parameter(name, p)
        for i, b in enumerate(floats):
            self.register_buffer("running%d" % i, b)
        for i, b in enumerate(ints):
            self.register_buffer("count%d" % i, b)


class Rig:
    """The tensor set of the plan test on the device: two AdamW optimizers of two groups each (4 groups), records clipped or
    not, with weight decay or not, with a teacher (members of the student module) or none (free parameters, as T_predictor's
    are), three float buffers and an int64 one.  warm: the optimizers arrive with a state of three steps (adopted)."""

    def __init__(self, hp, seed=11, warm=True, max_norm=1.0, decay=DECAY, lr_tensor=False):
        from geot_amd.optim_tail import OptimTail
        self.recs = ref.make_records(seed, warm=warm)
        self.bufs = ref.make_buffers(seed)
        for i, r in enumerate(self.recs):
            r["group"] += 0 if i < 5 else 2
        self.groups = ref.groups_of(hp) + ref.groups_of(hp)
        self.params = [torch.nn.Parameter(_T(r["p"])) for r in self.recs]
        named = [("p%d" % i, p) for i, (p, r) in enumerate(zip(self.params, self.recs)) if r["t"] is not None]
        self.student = _Holder(named, [_T(b["p"]) for b in self.bufs if b["kind"] == "ema"],
                               [_T(b["p"]) for b in self.bufs if b["kind"] == "int"])
        self.teacher = _Holder([(n, torch.nn.Parameter(_T(self.recs[int(n[1:])]["t"]), requires_grad=False)) for n, _ in named],
                               [_T(b["t"]) for b in self.bufs if b["kind"] == "ema"],
                               [_T(b["t"]) for b in self.bufs if b["kind"] == "int"])
        self.lrs = []
        self.opts = []
        for lo in (0, 2):
            gs = []
            for k in (lo, lo + 1):
                g = dict(self.groups[k], params=[p for p, r in zip(self.params, self.recs) if r["group"] == k])
                if lr_tensor:
                    g["lr"] = torch.tensor(g["lr"], dtype=torch.float32, device=DEV)
                    self.lrs.append(g["lr"])
                gs.append(g)
            self.opts.append(torch.optim.AdamW(gs, fused=True))
        if warm:
            for p, r in zip(self.params, self.recs):
                opt = self.opts[0 if r["group"] < 2 else 1]
                opt.state[p] = {"step": torch.tensor(float(r["step"]), device=DEV), "exp_avg": _T(r["m"]), "exp_avg_sq": _T(r["v"])}
        self.clipped = [p for p, r in zip(self.params, self.recs) if r["clipped"]]
        self.max_norm, self.decay = max_norm, decay
        self.tail = OptimTail(self.opts, clip_params=self.clipped if max_norm is not None else None, max_norm=max_norm,
                              teacher=self.teacher, student=self.student, ema_decay=decay)

    def set_grads(self, seed, scale=1.0, inf_at=None):
        rng = np.random.default_rng((seed, 3))
        for i, (p, r) in enumerate(zip(self.params, self.recs)):
            g = (rng.standard_normal(p.numel()) * scale * (1e-3 if i == 5 else 1.0)).astype(np.float32)
            if inf_at is not None and i == inf_at[0]:
                g[inf_at[1]] = np.inf
            if i == MISALIGNED:
                store = torch.empty(p.numel() + 1, dtype=torch.float32, device=DEV)
                p.grad = store[1:]
                p.grad.copy_(_T(g))
                assert p.grad.data_ptr() % 16 == 4 and p.grad.is_contiguous()
            else:
                p.grad = _T(g)

    def snapshot(self):
        """The device state as the restatement's records."""
        out = []
        t_of = dict(self.teacher.named_parameters())
        for i, (p, r) in enumerate(zip(self.params, self.recs)):
            st = self.opts[0 if r["group"] < 2 else 1].state.get(p, {})
            n = p.numel()
            out.append(dict(kind="adamw", p=p.detach().cpu().numpy(), g=p.grad.cpu().numpy(), group=r["group"],
                            clipped=r["clipped"], step=int(st["step"].item()) if st else 0,
                            m=st["exp_avg"].cpu().numpy() if st else np.zeros(n, np.float32),
                            v=st["exp_avg_sq"].cpu().numpy() if st else np.zeros(n, np.float32),
                            t=t_of["p%d" % i].detach().cpu().numpy() if "p%d" % i in t_of else None))
        s_b, t_b = dict(self.student.named_buffers()), dict(self.teacher.named_buffers())
        for name in s_b:
            out.append(dict(kind="int" if s_b[name].dtype == torch.int64 else "ema", p=s_b[name].cpu().numpy(),
                            t=t_b[name].cpu().numpy()))
        return out

    def want(self, before, chain=ref.ANY_CHAIN):
        return ref.tail(before, self.groups, self.max_norm, self.decay, chain=chain)

    def check(self, want, what=""):
        """Everything the tail wrote, against the restatement's results and bounds."""
        after = self.snapshot()
        worst = 0.0
        for i, (a, w) in enumerate(zip(after, want)):
            if w["kind"] == "adamw":
                assert a["step"] == w["step"], (what, i, a["step"], w["step"])
                for key, e in (("p", "E_p"), ("m", "E_m"), ("v", "E_v")):
                    r = ref.ratio(a[key], w[key], w[e])
                    worst = max(worst, r)
                    assert r <= 1.0, (what, i, key, r)
            if w.get("t") is not None:
                if w["kind"] == "int":
                    assert np.array_equal(a["t"], w["t"]), (what, i)
                else:
                    r = ref.ratio(a["t"], w["t"], w["E_t"])
                    worst = max(worst, r)
                    assert r <= 1.0, (what, i, "t", r)
        return worst

    def bits(self):
        torch.cuda.synchronize()
        out = []
        for r in self.snapshot():
            out += [r[k] for k in ("p", "m", "v", "t") if r.get(k) is not None]
        return out


def _same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# ---- A. the tail alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hp", sorted(HPS))
def test_warm_step_against_fp64_with_the_norm_above_max_norm(hp):
    rig = Rig(HPS[hp])
    rig.set_grads(1)
    before = rig.snapshot()
    want, norm, coef = rig.want(before)
    assert coef < 0.5 and all(r["step"] == 3 for r in before if r["kind"] == "adamw")
    got = rig.tail.step()
    torch.cuda.synchronize()
    worst = rig.check(want, hp)
    print("worst error / bound:", worst)
    assert abs(float(got) - norm) <= ref.norm_error(ref.KERNEL_CHAIN) * norm           # the kernel's counted chain
    assert abs(float(rig.tail.clip_coef) - coef) <= (ref.norm_error(ref.KERNEL_CHAIN) + 4 * ref.U) * coef
    row = {id(rig.tail.params[k][0]): j for j, k in enumerate(rig.tail._active)}       # (the table is in group order)
    vector = [int(rig.tail.last_plan["vector"][row[id(p)]]) for p in rig.params]
    assert vector == [int(i != MISALIGNED) for i in range(8)]                           # the view took the scalar path, alone
    assert all(t.requires_grad is False for t in rig.teacher.parameters())


@pytest.mark.parametrize("hp", sorted(HPS))
def test_steps_one_to_three_from_a_fresh_state(hp):
    """The state is created as torch.optim.AdamW creates it; every step is held against the restatement started from the
    device's own state before it."""
    rig = Rig(HPS[hp], warm=False)
    for step in range(3):
        rig.set_grads(10 + step)
        before = rig.snapshot()
        assert all(r["step"] == step for r in before if r["kind"] == "adamw")
        want, _, _ = rig.want(before)
        rig.tail.step()
        rig.check(want, (hp, step))
    for p, r in zip(rig.params, rig.recs):
        st = rig.opts[0 if r["group"] < 2 else 1].state[p]
        assert st["step"].dim() == 0 and st["step"].dtype == torch.float32 and st["step"].device == p.device
        assert st["exp_avg"].shape == p.shape == st["exp_avg_sq"].shape


def test_a_norm_below_max_norm_equals_clip_off_bit_for_bit():
    runs = []
    for max_norm in (1e6, None):
        rig = Rig(ref.EXAGGERATED_HP, max_norm=max_norm)
        rig.set_grads(2)
        rig.tail.step()
        runs.append(rig.bits())
        assert float(rig.tail.clip_coef) == 1.0
    assert _same_bits(*runs)


def test_an_infinite_gradient_gives_the_composites_non_finite_pattern():
    pats = []
    for fused in (True, False):
        rig = Rig(ref.REFERENCE_HP)
        rig.set_grads(4, inf_at=(7, 5000))
        norm = rig.tail.step() if fused else rig.tail.composite()
        assert float(norm) == float("inf")
        pats.append([np.isnan(x) if x.dtype != np.int64 else x for x in rig.bits()])
    assert _same_bits(*pats)
    assert any(p.any() for p in pats[0] if p.dtype == bool) and not all(p.all() for p in pats[0] if p.dtype == bool and p.size)


def test_two_runs_and_an_lr_from_device_memory_give_the_same_bits():
    runs = []
    for lr_tensor in (False, False, True):
        rig = Rig(ref.EXAGGERATED_HP, warm=False, lr_tensor=lr_tensor)
        for step in range(2):
            rig.set_grads(20 + step)
            rig.tail.step()
        runs.append(rig.bits())
    assert _same_bits(runs[0], runs[1]) and _same_bits(runs[0], runs[2])
    # ... and the tensor is read on the device, call by call: another value, other bits, no rebuild
    rig.lrs[0].fill_(0.05)
    rig.set_grads(22)
    before = rig.snapshot()
    rig.groups[0]["lr"] = float(np.float32(0.05))
    want, _, _ = rig.want(before)
    rig.tail.step()
    rig.check(want, "lr refilled")


@pytest.mark.parametrize("hp", sorted(HPS))
def test_the_composite_lies_within_the_same_bound(hp):
    rig = Rig(HPS[hp])
    rig.set_grads(1)
    want, norm, _ = rig.want(rig.snapshot())
    got = rig.tail.composite()
    rig.check(want, hp)
    assert abs(float(got) - norm) <= ref.norm_error(ref.ANY_CHAIN) * norm


@pytest.mark.parametrize("first", ["fused", "torch"])
def test_state_round_trip_with_torch_adamw(first):
    """Two steps one way, state_dict() into fresh torch.optim.AdamW objects (a checkpoint: a deep copy), one more step each
    way: both continue from the same state, within the bound of the restatement."""
    a = Rig(ref.EXAGGERATED_HP, warm=False)
    for step in range(2):
        a.set_grads(30 + step)
        a.tail.step() if first == "fused" else a.tail.composite()
    b = Rig(ref.EXAGGERATED_HP, warm=False)
    with torch.no_grad():
        for x, y in zip(list(a.student.state_dict().values()) + list(a.teacher.state_dict().values()) + a.params,
                        list(b.student.state_dict().values()) + list(b.teacher.state_dict().values()) + b.params):
            y.copy_(x)
    for oa, ob in zip(a.opts, b.opts):
        ob.load_state_dict(copy.deepcopy(oa.state_dict()))
    for rig in (a, b):
        rig.set_grads(32)
    before = a.snapshot()
    assert all(r["step"] == 2 for r in before if r["kind"] == "adamw")
    assert _same_bits(a.bits(), b.bits())
    want, _, _ = a.want(before)
    # the loaded side runs the OTHER implementation: torch's after the fused steps, the fused one (adopting) after torch's
    if first == "fused":
        a.tail.step(), b.tail.composite()
    else:
        a.tail.composite(), b.tail.step()
    a.check(want, "continued")
    b.check(want, "loaded")


# ---- B. capture ------------------------------------------------------------------------------------------------------------------------
def test_three_replays_equal_three_eager_calls_and_the_graph_is_kernels_only():
    from geot_amd import streams

    def rig_with_state():
        rig = Rig(ref.REFERENCE_HP, warm=False)
        rig.set_grads(40)
        rig.tail.step()              # (creates the state: not under capture)
        return rig
    eager = rig_with_state()
    for _ in range(3):
        eager.tail.step()
    rig = rig_with_state()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with streams.capture(graph, DEV):
        rig.tail.step()
    kinds = streams.node_types(graph)
    assert set(kinds) == {"kernel"} and kinds["kernel"] == rig.tail.launches == 3, kinds
    for _ in range(3):
        graph.replay()
    assert _same_bits(eager.bits(), rig.bits())
    assert float(rig.opts[0].state[rig.params[1]]["step"]) == 4.0


# ---- C. the steps ----------------------------------------------------------------------------------------------------------------------
from test_fixmatch_phase2_gpu import SMALL, _batch, _same, _state      # noqa: E402


def _supervised(**kw):
    from geot_amd.openpoints.models.backbone.transformer import PointTransformer_seg_T
    from geot_amd.train_step import SupervisedStep
    torch.manual_seed(5)
    net = PointTransformer_seg_T(**SMALL).to(DEV)
    return SupervisedStep(net, **kw)


def _sampled_records(step, stride_to=65536):
    """The step's parameters, gradients and optimizer state right before its tail, as the restatement's records: every
    tensor's elements [::stride] (the bounds are per element), and the fp64 norm of ALL gradient elements."""
    recs, total = [], torch.zeros((), dtype=torch.float64, device=DEV)
    opt = step.optimizer
    for gi, group in enumerate(opt.param_groups):
        for p in group["params"]:
            if p.grad is None:
                continue
            total += p.grad.double().pow(2).sum()
            pick = slice(None, None, max(1, p.numel() // stride_to))
            st = opt.state.get(p) or {}
            take = lambda t: t.detach().reshape(-1)[pick].cpu().numpy()      # noqa: E731
            n = len(take(p))
            recs.append(dict(kind="adamw", p=take(p), g=take(p.grad), group=gi, clipped=True, t=None, key=id(p),
                             step=int(st["step"].item()) if st else 0,
                             m=take(st["exp_avg"]) if st else np.zeros(n, np.float32),
                             v=take(st["exp_avg_sq"]) if st else np.zeros(n, np.float32)))
    return recs, float(total.sqrt())


def _iterate(step, data):
    """SupervisedStep.iteration() in its pieces, with the records of its tail taken between backward and update."""
    from geot_amd import train_step as ts
    loss = step.forward_loss(data["pos"], data["cls"], data["y"])
    loss.backward()
    recs, norm = _sampled_records(step)
    params = {r["key"]: p for g in step.optimizer.param_groups for p in g["params"] for r in recs if r["key"] == id(p)}
    ts._update(step.grad_sync, step.clip, step.model, step.optimizers(), step.tail, step.tail is not None)
    after = [params[r["key"]].detach().reshape(-1)[slice(None, None, max(1, params[r["key"]].numel() // 65536))].cpu().numpy()
             for r in recs]
    return loss.detach().clone(), recs, norm, after


def test_supervised_step_with_the_fused_tail_against_the_composite():
    """Two iterations with grad_norm_clip=1.  The first loss is the default step's, bit for bit (nothing before the first
    update differs).  After each iteration the parameters of the fused run lie within the restatement's bound of the torch
    run's: |p_fused - p_torch| <= E_p(fused) + E_p(torch) + |R_fused - R_torch|, R the fp64 restatement of the iteration's
    tail on the run's OWN state and gradients.  In the first iteration both runs hold the same bits, R_fused = R_torch, and
    the bound is 2 E_p.  In the second their gradients differ, and no multiple of E_p can hold them together: a parameter
    whose gradient is rounding noise (a bias in front of a BatchNorm) takes a step of lr times the SIGN of that noise --
    measured: 6.1e5 times the two-iteration sum of E_p between the two runs, from inputs that agree to an ulp -- so the
    difference of the inputs enters exactly, through R, and each run is held to its one-step bound from where it stands."""
    data, _ = _batch(3)
    default = _supervised(grad_norm_clip=1.0)
    torch.manual_seed(11)
    first = default(data["pos"], data["cls"], data["y"]).clone()
    runs = {}
    for fused in (False, True):
        step = _supervised(grad_norm_clip=1.0, fused_tail=fused)
        torch.manual_seed(11)
        runs[fused] = [_iterate(step, data) for _ in range(2)], step
    assert torch.equal(first, runs[False][0][0][0]) and torch.equal(first, runs[True][0][0][0])
    groups = [dict(ref.REFERENCE_HP, weight_decay=g["weight_decay"]) for g in runs[True][1].optimizer.param_groups]
    for it in range(2):
        res = {}
        for fused in (False, True):
            _, recs, norm, after = runs[fused][0][it]
            out, _, coef = ref.tail(recs, groups, 1.0, None, norm=norm)
            assert coef < 1.0 and len(out) == len(after) > 50
            worst = max(ref.ratio(a, w["p"], w["E_p"]) for a, w in zip(after, out))
            print("iteration", it, "fused" if fused else "torch", "worst error / bound:", worst, "coef", coef)
            assert worst <= 1.0, (it, fused, worst)
            res[fused] = (after, out)
        (pa, oa), (pb, ob) = res[False], res[True]
        if it == 0:
            assert all(np.array_equal(x["p"], y["p"]) for x, y in zip(oa, ob))          # the same inputs: the same R
        cross = max(ref.ratio(b, a, x["E_p"] + y["E_p"] + np.abs(x["p"] - y["p"])) for a, b, x, y in zip(pa, pb, oa, ob))
        print("iteration", it, "fused against torch, worst difference / bound:", cross)
        assert cross <= 1.0, (it, cross)
    assert float(runs[True][1].tail.total_norm) > 0 and runs[False][1].tail is None


def _fixmatch(cfg):
    from geot_amd import train_step as ts
    torch.manual_seed(5)
    return ts.build_fixmatch(DEV, seg_cfg=SMALL, cfg=cfg, use_ddp=False)


@pytest.mark.parametrize("fused", [False, True])
def test_fixmatch_step_moves_the_teacher_towards_the_student(fused):
    from geot_amd import train_step as ts
    cfg = dict(ts.NTM_CFG, threed_k=8, ema_teacher=True, fused_tail=fused, grad_norm_clip=1.0)
    step = _fixmatch(cfg)
    t0 = {k: v.detach().clone() for k, v in step.model_t.state_dict().items()}
    data, data_u = _batch(3)
    torch.manual_seed(11)
    losses = step(data, data_u)
    torch.cuda.synchronize()
    assert ("grad_norm" in losses) == fused and all(torch.isfinite(v).all() for v in losses.values())
    d = cfg["ema_decay"]
    s_sd, t_sd = step.model.state_dict(), step.model_t.state_dict()
    moved = 0
    for name, t in t_sd.items():
        s = s_sd[name]
        if t.dtype == torch.int64:
            assert torch.equal(t, s), name
            continue
        a, b, c = t0[name].double().cpu().numpy(), s.double().cpu().numpy(), t.double().cpu().numpy()
        want = d * a + (1 - d) * b
        # E_t of _optim_tail_ref.py with E_p = 0: the student's value is read back exactly
        bound = 2 * ref.U * d * np.abs(a) + 3 * ref.U * (1 - d) * (np.abs(b) + np.abs(a)) + ref.U * np.abs(want)
        assert ref.ratio(c, want, bound) <= 1.0, name
        moved += int(not torch.equal(t, t0[name]))
    assert moved > len(t_sd) // 2, moved
    assert all(not p.requires_grad for p in step.model_t.parameters())


EPOCHS = [50, 50, 50, 51, 51, 51]      # warmup=1: P@e / M@e run eagerly once, are captured and replayed; then P@2 / M@2 likewise


def test_graphed_equals_eager_with_a_moving_teacher_across_the_switch():
    from geot_amd import train_step as ts, graph_step as gs
    cfg = dict(ts.NTM_CFG, threed_k=8, ema_teacher=True, fused_tail=True, grad_norm_clip=1.0)
    batches = [_batch(3), _batch(400)]
    runs = {}
    for mode in ("eager", "graph"):
        step = _fixmatch(cfg)
        call = gs.GraphedFixMatchStep(step, warmup=1) if mode == "graph" else step
        inside = []
        if mode == "graph":
            step.model_t.register_forward_hook(lambda *a: inside.append(tuple(call._where)))
            call._where = ["?"]
            run = call._run

            def traced(name, fn, pool_of=None, run=run, call=call):
                call._where = [name]
                try:
                    return run(name, fn, pool_of)
                finally:
                    call._where = ["-"]
            call._run = traced
        torch.manual_seed(11)
        out = []
        for i, epoch in enumerate(EPOCHS):
            call.set_epoch(epoch)
            cur, nxt = batches[i % 2], batches[(i + 1) % 2]
            res = call(cur[0], cur[1], next_batches=nxt)
            out.append({k: v.clone() for k, v in res.items()})
        torch.cuda.synchronize()
        if mode == "graph":
            assert {"P@e", "M@e", "P@2", "M@2"} <= set(call.graphs) and "P" not in call.graphs, sorted(call.graphs)
            assert all(set(call.node_types[k]) == {"kernel"} for k in call.graphs), call.node_types
            pre_e = call._pres["@e"]
            assert pre_e.pseudo is None and pre_e.feat_t is None and pre_e.geom_t is not None
            assert inside and all(w == ("M@e",) for w in inside), inside      # the teacher's forward: inside M, never inside P
        state = _state(step)
        state.update({"teacher." + k: v.detach().clone() for k, v in step.model_t.state_dict().items()})
        runs[mode] = (out, state)
    for i, (a, b) in enumerate(zip(runs["eager"][0], runs["graph"][0])):
        assert set(a) == set(b) and "grad_norm" in a
        for k in a:
            assert torch.equal(a[k], b[k]), (i, k, float(a[k]), float(b[k]))
    _same(runs["eager"][1], runs["graph"][1], "graph against eager")


def test_switches_off_is_the_step_built_without_the_keys():
    from geot_amd import train_step as ts
    new_keys = ("ema_teacher", "ema_decay", "fused_tail")
    batches = [_batch(3), _batch(400)]
    runs = []
    for with_keys in (True, False):
        cfg = dict(ts.NTM_CFG, threed_k=8, grad_norm_clip=1.0)
        if not with_keys:
            cfg = {k: v for k, v in cfg.items() if k not in new_keys}
        step = _fixmatch(cfg)
        assert step.tail is None
        if not with_keys:                       # (the step fills in defaults: take them out again)
            for k in new_keys:
                assert step.cfg[k] == ts.NTM_CFG[k]
        t0 = {k: v.detach().clone() for k, v in step.model_t.state_dict().items()}
        torch.manual_seed(11)
        for i in range(2):
            step(*batches[i])
        torch.cuda.synchronize()
        runs.append(_state(step))
        assert all(torch.equal(v, t0[k]) for k, v in step.model_t.state_dict().items())      # the frozen teacher stays frozen
    _same(runs[0], runs[1], "switches off")
