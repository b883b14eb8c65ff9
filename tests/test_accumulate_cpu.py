"""step_per_update (include/geot_hip.h "ABI 27", OptimTail(accumulate=k)) without a GPU: the cfg key and the steps' argument,
the new entry points in the header and in both bindings, the host-only plan of the gated tail's launches, malformed records,
and the torch form's gradient exchange -- one collective per update -- against DistributedDataParallel under no_sync()."""
import ctypes
import os
import re
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from geot_amd import _header, _lib, optim_tail as ot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1          # hipErrorInvalidValue
NEW = ("geot_optim_tail_accumulate", "geot_optim_tail_acc_finish", "geot_optim_tail_acc_update")


def _blocks(n):
    return -(-n // ot.BLOCK_ELEMS)


# ---- cfg and arguments ---------------------------------------------------------------------------------------------------------
BAD = (0, -1, 2.5, True, "2")


def test_cfg_key_default_and_checks():
    from geot_amd import train_step as ts
    assert ts.NTM_CFG["step_per_update"] == 1
    ts.check_cfg(dict(ts.NTM_CFG, step_per_update=4, fused_tail=True))
    ts.check_cfg({k: v for k, v in ts.NTM_CFG.items() if k != "step_per_update"})      # a cfg from before the key
    for bad in BAD:
        with pytest.raises((TypeError, ValueError)):
            ts.check_cfg(dict(ts.NTM_CFG, step_per_update=bad))
        with pytest.raises((TypeError, ValueError)):
            ts.FixMatchNTMStep(None, None, None, cfg=dict(ts.NTM_CFG, step_per_update=bad))      # before anything is touched


def test_supervised_step_argument_is_checked_before_anything_else():
    from geot_amd import train_step as ts
    for bad in BAD:
        with pytest.raises((TypeError, ValueError)):
            ts.SupervisedStep(None, step_per_update=bad)
    step = ts.SupervisedStep(torch.nn.Linear(2, 2), step_per_update=3)
    assert step.step_per_update == 3 and step.tail is None
    assert ts.SupervisedStep(torch.nn.Linear(2, 2)).step_per_update == 1
    step.new_epoch()                                       # the torch form: a count on the host, no device


def test_optim_tail_argument_is_checked():
    lin = torch.nn.Linear(3, 2)
    for bad in BAD:
        with pytest.raises((TypeError, ValueError)):
            ot.OptimTail([torch.optim.AdamW(lin.parameters())], accumulate=bad)


def test_the_wrappers_refuse_what_a_graph_cannot_gate():
    """k > 1 in the torch form: RuntimeError naming fused_tail; k > 1 with a gradient exchange of the step's own:
    NotImplementedError -- both before anything else of the wrapper runs."""
    from geot_amd import graph_step as gs
    plain = types.SimpleNamespace(step_per_update=2, tail=None, grad_sync=None)
    for cls in (gs.GraphedSupervisedStep, gs.GraphedFixMatchStep):
        with pytest.raises(RuntimeError, match="fused_tail"):
            cls(plain)
    fused = types.SimpleNamespace(step_per_update=2, tail=types.SimpleNamespace(accumulate=2), grad_sync=object())
    for cls in (gs.GraphedSupervisedStep, gs.GraphedFixMatchStep):
        with pytest.raises(NotImplementedError, match="step_per_update"):
            cls(fused)


# ---- header and bindings -------------------------------------------------------------------------------------------------------
def test_new_entries_are_in_the_header_and_bound_by_both_bindings():
    hdr = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    assert int(re.search(r"GEOT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 27
    lib = _lib.load()
    assert lib.geot_abi_version() == _lib.ABI_VERSION
    entries = {e.name: e for e in _header.parse()[0]}
    for name in NEW:
        assert entries[name].streamed and name in _lib.PROTOTYPES and hasattr(lib, name)
    assert "geot_optim_tail_acc_plan" in _lib.PLAIN and not entries["geot_optim_tail_acc_plan"].streamed
    # the record and the group did not grow, the ABI-25 entries are what they were
    assert ot.RECORD.itemsize == 64 and ot.GROUP.itemsize == 40
    assert len(_lib.PROTOTYPES["geot_optim_tail_update"]) == 9 and len(_lib.PROTOTYPES["geot_optim_tail_finish"]) == 10
    # the compiled dispatcher is generated from the same parse: its source forwards every new entry
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_dispatch", os.path.join(ROOT, "geot_amd", "csrc_torch", "gen_dispatch.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    source, names = gen.emit(_header.parse()[0])
    for name in NEW + ("geot_optim_tail_acc_plan",):
        assert name in names and 'm.def("%s"' % name in source, name


# ---- the host-only plan ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [ot.CAP - 1, ot.CAP, ot.CAP + 1, 2 * ot.CAP, 2 * ot.CAP + 1])
def test_acc_plan_record_counts_around_the_launch_capacity(t):
    counts = [(7 * i) % 9000 + 1 for i in range(t)]
    flags = [ot.CLIPPED] * t
    pl, old = ot.acc_plan(counts, [1] * t, flags), ot.plan(counts, [1] * t, flags)
    assert pl["acc_launches"] == pl["update_launches"] == old["update_launches"] == -(-t // ot.CAP)
    assert pl["finish_launches"] == 1
    assert pl["acc_blocks"] == pl["update_blocks"] == pl["slots"] == sum(_blocks(n) for n in counts) == old["slots"]
    # every second record a buffer: the accumulate sweep packs the AdamW records, the update sweep keeps the table's chunks
    flags = [ot.CLIPPED if i % 2 == 0 else ot.EMA_ONLY for i in range(t)]
    pl = ot.acc_plan(counts, [1] * t, flags)
    assert pl["update_launches"] == -(-t // ot.CAP) and pl["acc_launches"] == -(-((t + 1) // 2) // ot.CAP)
    assert pl["acc_blocks"] == pl["slots"] == sum(_blocks(n) for n in counts[::2])
    assert pl["update_blocks"] == sum(_blocks(n) for n in counts)
    # unclipped records are accumulated too, but hold no slot
    flags = [ot.CLIPPED if i % 2 == 0 else 0 for i in range(t)]
    pl = ot.acc_plan(counts, [1] * t, flags)
    assert pl["acc_launches"] == -(-t // ot.CAP) and pl["acc_blocks"] == sum(_blocks(n) for n in counts)
    assert pl["slots"] == sum(_blocks(n) for n in counts[::2])
    # a whole launch of empty records is not issued
    counts = [0] * ot.CAP + [1] * (t - ot.CAP) if t > ot.CAP else [0] * t
    pl = ot.acc_plan(counts, [1] * t, [0] * t)
    assert pl["acc_launches"] == pl["update_launches"] == (-(-t // ot.CAP) - 1 if t > ot.CAP else 0)


def test_acc_plan_element_counts_around_a_workgroup_and_the_finish_launches():
    counts = [1, 3, 4, ot.BLOCK_ELEMS - 1, ot.BLOCK_ELEMS, ot.BLOCK_ELEMS + 1, 2 * ot.BLOCK_ELEMS + 5, 0]
    t = len(counts)
    pl = ot.acc_plan(counts, [1] * t, [ot.CLIPPED] * t)
    assert pl["acc_blocks"] == pl["slots"] == 1 + 1 + 1 + 1 + 1 + 2 + 3
    assert pl["acc_launches"] == pl["update_launches"] == pl["finish_launches"] == 1
    flags = [ot.CLIPPED, 0, ot.CLIPPED | ot.EMA_ONLY, ot.INT64, ot.CLIPPED, 0, ot.CLIPPED, ot.EMA_ONLY]
    pl = ot.acc_plan(counts, [1] * t, flags)
    assert pl["slots"] == 1 + 1 + 3 and pl["acc_blocks"] == 1 + 1 + 1 + 2 + 3 and pl["update_blocks"] == 10
    # the step counters of the finish stage: one launch per STEP_CAP AdamW records, and one for none
    cap = _lib.OPTIM_TAIL_STEP_CAP
    for n, want in ((0, 1), (cap, 1), (cap + 1, 2), (2 * cap + 1, 3)):
        assert ot.acc_plan([1] * n, [1] * n, [0] * n)["finish_launches"] == want
    assert ot.acc_plan([1] * (cap + 1), [1] * (cap + 1), [ot.EMA_ONLY] * (cap + 1))["finish_launches"] == 1
    assert ot.acc_plan([], [], [])["acc_launches"] == 0
    with pytest.raises(RuntimeError):
        ot.acc_plan([4, -1], [1, 1], [0, 0])
    out = (ctypes.c_longlong * 6)(*([-7] * 6))
    one = (ctypes.c_longlong * 1)(4)
    ok = (ctypes.c_int * 1)(1)
    assert _lib.load().geot_optim_tail_acc_plan(1, one, ok, ok, out, 5) == 0 and list(out) == [-7] * 6      # no room


# ---- malformed records: hipErrorInvalidValue before any launch (no GPU is touched) -------------------------------------------------
def _table(**change):
    rec = np.zeros(1, dtype=ot.RECORD)
    rec[0] = (0x1000, 0x2000, 0x3000, 0x4000, 0, 8, 0, 0, ot.CLIPPED, 0)
    for k, v in change.items():
        rec[k] = v
    return rec


def test_malformed_sizes_and_records_are_invalid_value():
    lib = _lib.load()
    acc, offs, slots, gate, steps, scalars = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    group = np.zeros(1, dtype=ot.GROUP)
    group[0] = (0.9, 0.999, 1e-8, 0.0, 1e-3, 0, 0)

    def accumulate(rec, acc=acc, offs=offs, n_acc=64, n_steps=1, slots=slots, n_slots=4, t=1):
        return lib.geot_optim_tail_accumulate(t, rec.ctypes.data, acc, offs, n_acc, n_steps, slots, n_slots, None)

    def finish(rec, clip=1, n_slots=1, slots=slots, steps=steps, n_steps=1, scalars=scalars, gate=gate, k=2, t=1):
        return lib.geot_optim_tail_acc_finish(t, rec.ctypes.data, clip, n_slots, slots, 1.0, steps, n_steps, scalars, gate, k, None)

    def update(rec, n_groups=1, groups=group, scalars=scalars, steps=steps, n_steps=1, decay=0.9, acc=acc, offs=offs,
               n_acc=64, gate=gate, t=1):
        return lib.geot_optim_tail_acc_update(t, rec.ctypes.data, n_groups, groups.ctypes.data, scalars, steps, n_steps, decay,
                                              acc, offs, n_acc, gate, None)
    good = _table()
    for bad in (_table(n=-1), _table(p=0), _table(m=0), _table(v=0), _table(step=1), _table(step=-1), _table(group=-1),
                _table(group=ot.MAX_GROUPS), _table(n=65)):
        assert accumulate(bad) == INVALID, bad
    for kw in (dict(acc=None), dict(offs=None), dict(acc=acc + 4), dict(n_acc=-1), dict(n_acc=7), dict(n_steps=-1),
               dict(n_slots=0), dict(slots=None), dict(n_slots=-1), dict(t=-1)):
        assert accumulate(good, **kw) == INVALID, kw
    assert accumulate(_table(p=0, t=0x5000, flags=ot.EMA_ONLY)) == INVALID           # an EMA-only record without its teacher
    two = np.concatenate([good, good])
    for kw in (dict(scalars=None), dict(gate=None), dict(k=0), dict(k=-3), dict(n_steps=-1), dict(n_slots=-1), dict(slots=None),
               dict(steps=None), dict(t=-1)):
        assert finish(good, **kw) == INVALID, kw
    assert finish(two, t=2, n_steps=4) == INVALID                                    # two writers of one step counter
    assert finish(_table(step=1)) == INVALID and finish(_table(step=-1)) == INVALID
    for bad in (_table(n=-1), _table(p=0), _table(m=0), _table(step=1), _table(group=1), _table(n=65)):
        assert update(bad) == INVALID, bad
    for kw in (dict(n_groups=-1), dict(n_groups=ot.MAX_GROUPS + 1), dict(scalars=None), dict(steps=None), dict(decay=1.0),
               dict(decay=-0.1), dict(decay=float("nan")), dict(acc=None), dict(acc=acc + 8), dict(offs=None), dict(n_acc=-1),
               dict(gate=None), dict(t=-1)):
        assert update(good, **kw) == INVALID, kw


# ---- two ranks: one exchange per update, DistributedDataParallel's bits --------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _window_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank))
    from geot_amd import dist_utils, train_step as ts
    dist_utils.init("gloo")
    torch.manual_seed(100 + rank)

    def net():
        return torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.ReLU(), torch.nn.Linear(16, 16), torch.nn.ReLU(),
                                   torch.nn.Linear(16, 3))
    a, b = net(), net()
    b.load_state_dict(a.state_dict())
    ddp = torch.nn.parallel.DistributedDataParallel(a)
    sync = ts.GradSync([b], dist.group.WORLD)
    oa, ob = torch.optim.SGD(a.parameters(), lr=0.1), torch.optim.SGD(b.parameters(), lr=0.1)
    # what the steps hand _window_update / _accumulating: the torch form (no tail) with step_per_update = 2
    wrapped = types.SimpleNamespace(step_per_update=2, _window_calls=0, grad_sync=None, tail=None, optimizers=lambda: [oa],
                                    sync_modules=lambda: [ddp])
    bare = types.SimpleNamespace(step_per_update=2, _window_calls=0, grad_sync=sync, tail=None, optimizers=lambda: [ob],
                                 sync_modules=lambda: [b])
    g = torch.Generator().manual_seed(7 + rank)
    worst, inside, updates = 0.0, [], 0
    for call in range(5):
        x, y = torch.randn(5 + rank, 6, generator=g), torch.randn(5 + rank, 3, generator=g)
        for step, model in ((wrapped, ddp), (bare, b)):
            with ts._accumulating(step, False):
                inside.append(ddp.require_backward_grad_sync)
                torch.nn.functional.mse_loss(model(x), y).backward()
            ts._window_update(step, None, model, False)
        updates += call % 2
        before = [p.detach().clone() for p in b.parameters()]
        if call % 2 == 0:
            assert all(p.grad is not None for p in b.parameters())          # the sum stays in .grad
        for p1, p2 in zip(a.parameters(), b.parameters()):
            worst = max(worst, float((p1 - p2).abs().max()))
        del before
    gathered = [torch.zeros(3) for _ in range(world)]
    dist.all_gather(gathered, torch.cat([p.detach().reshape(-1) for p in b.parameters()])[:3].contiguous())
    q.put((rank, worst, sync.collectives, updates, inside[0::2], [g_.tolist() for g_ in gathered]))
    dist.destroy_process_group()


def test_two_ranks_exchange_once_per_update_and_equal_ddp_under_no_sync():
    """The torch form with step_per_update=2 over five calls: GradSync runs on the two update calls only, on the accumulated
    .grad; the DistributedDataParallel module runs calls 1, 3 and 5 under no_sync(); both leave the same parameter bits (as
    test_dist_cpu compares them at k = 1), the same on both ranks."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_window_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, worst, collectives, updates, ddp_syncs, gathered in res:
        assert worst == 0.0, (rank, worst)
        assert collectives == updates == 2
        assert ddp_syncs == [False, True, False, True, False]
        assert gathered[0] == gathered[1]
