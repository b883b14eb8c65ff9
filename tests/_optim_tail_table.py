"""A table-level harness for the optimizer tail (csrc/optim_tail.hip, include/geot_hip.h "ABI 25" / "ABI 27"): record tables
built by hand, every tensor laid into ONE guarded device arena per dtype, and the ABI sequences issued exactly as
OptimTail.step / OptimTail._step_window issue them -- so that a test chooses the order of the records, the alignment of every
pointer, the step-counter indirection and the launch boundaries, and sees a write past a tensor's end.

    spec      a list of records: rec(kind, n, group, clipped, teacher, step_index, step0, misalign)
    layout    (host, no torch) where every tensor and every guard element lies
    Table     (device) arena, RECORD / GROUP tables, steps / scalars / slots / gate / accumulator, each between guards;
              ungated() / gated() issue the sequences, read() brings everything back with a `guards_intact` verdict
    to_ref_records    the dicts tests/_optim_tail_ref.tail takes
    the cases the GPU file runs, by name (CASES): tests/test_optim_tail_table_cpu.py proves each on its branch through the
    library's own planners.

numpy only at import: torch and geot_amd are imported where a device or the library's constants are needed."""
import numpy as np

import _optim_tail_ref as ref

BLOCK = ref.BLOCK
CAP = 48              # GEOT_OPTIM_TAIL_CAP and GEOT_OPTIM_TAIL_STEP_CAP, restated: the CPU test asserts that the header agrees
STEP_CAP = 896
KEYS = ("p", "g", "m", "v", "t")
G = 8                 # guard elements before and after every tensor, at least
GUARD_F32_BITS = 0x4B1DC0DE                      # 10338526.0: finite, far outside every input
GUARD_I64 = 0x5AFEC0DE5AFEC0DE                   # above every integer input (< 2^42)
GUARD_I32 = 0x5AFEC0DE
UNUSED_STEP = 77.0                               # a counter no record points at
SCALARS0 = (-3.0, -5.0)                          # total_norm / coef before the first finish launch: values it never writes
STEP0S = (0, 3, 10)
DECAY = 0.9

# four groups, four hyper-parameter sets; the lr of LR_PTR_GROUP is read from device memory
GROUPS = [dict(ref.REFERENCE_HP),
          dict(ref.EXAGGERATED_HP),
          dict(ref.REFERENCE_HP, lr=3e-3, betas=(0.8, 0.99), weight_decay=0.0),
          dict(ref.EXAGGERATED_HP, lr=0.03, eps=1e-5, weight_decay=0.3)]
LR_PTR_GROUP = 2


def rec(kind="adamw", n=1, group=0, clipped=True, teacher=True, step_index=0, step0=0, misalign=()):
    assert kind in ("adamw", "ema", "int") and n >= 0 and set(misalign) <= set(KEYS)
    assert not (kind == "int" and misalign), "an int64 tensor cannot start 4 bytes off"
    if kind != "adamw":                               # as OptimTail builds them: a teacher, no group, no counter
        teacher, group, step_index, step0 = True, 0, 0, 0
    return dict(kind=kind, n=int(n), group=int(group), clipped=bool(clipped), teacher=bool(teacher),
                step_index=int(step_index), step0=int(step0), misalign=frozenset(misalign))


def keys_of(r):
    """The tensors a record has."""
    if r["kind"] == "adamw":
        return ("p", "g", "m", "v", "t") if r["teacher"] else ("p", "g", "m", "v")
    return ("p", "t")


def tensors_of(r):
    """The tensors a record holds in an arena (an empty record holds none: null pointers)."""
    return keys_of(r) if r["n"] else ()


def arena_of(r):
    return "i64" if r["kind"] == "int" else "f32"


def layout(spec):
    """-> dict: at[i][key] the element offset of record i's tensor in its arena (None: a null pointer), size[arena] in
    elements, guard[arena] a bool array (True: a guard element).  Every tensor starts on 16 bytes, or 4 bytes behind when
    its key is in `misalign` (the arena's base is 16-byte aligned: Table asserts it), and has at least G guard elements on
    either side."""
    end = {"f32": 0, "i64": 0}
    spans = {"f32": [], "i64": []}
    at = []
    for r in spec:
        arena = arena_of(r)
        quad = 4 if arena == "f32" else 2              # elements per 16 bytes
        row = dict.fromkeys(KEYS)
        for key in tensors_of(r):
            start = -(-(end[arena] + G) // quad) * quad + (1 if key in r["misalign"] else 0)
            row[key] = start
            spans[arena].append((start, start + r["n"]))
            end[arena] = start + r["n"]
        at.append(row)
    size, guard = {}, {}
    for arena in end:
        size[arena] = -(-(end[arena] + G) // 4) * 4
        guard[arena] = np.ones(size[arena], dtype=bool)
        for a, b in spans[arena]:
            guard[arena][a:b] = False
    return {"at": at, "size": size, "guard": guard, "spans": spans}


def requested_alignment(spec, g_null=()):
    """1 where every pointer of the record is to be 16-byte aligned (a null pointer is), from the spec alone."""
    out = []
    for i, r in enumerate(spec):
        held = set(tensors_of(r)) - ({"g"} if i in g_null else set())
        out.append(int(not (held & r["misalign"])))
    return out


def flags_of(spec):
    from geot_amd import optim_tail as ot
    kind = {"adamw": 0, "ema": ot.EMA_ONLY, "int": ot.INT64}
    return [kind[r["kind"]] | (ot.CLIPPED if r["clipped"] else 0) for r in spec]


def plans_of(spec, g_null=()):
    """(geot_optim_tail_plan, geot_optim_tail_acc_plan) for the spec, through the built library (host only)."""
    from geot_amd import optim_tail as ot
    counts, aligned, flags = [r["n"] for r in spec], requested_alignment(spec, g_null), flags_of(spec)
    return ot.plan(counts, aligned, flags), ot.acc_plan(counts, aligned, flags)


def in_norm(r):
    return r["kind"] == "adamw" and r["clipped"]


def n_steps_of(spec):
    return 1 + max([r["step_index"] for r in spec if r["kind"] == "adamw"], default=0)


def make_inputs(spec, seed, call=0, target_norm=4.0):
    """fp32 arrays per record.  Moments as if step0 steps had run (zeros at step0 = 0); every eleventh record's gradient is
    1e-3 of the others', so that eps carries weight somewhere; the gradients are then scaled so that the clipped ones have
    norm `target_norm`: coef < 0.5 at max_norm 1.  `call` varies the gradients only."""
    out = []
    for i, r in enumerate(spec):
        n = r["n"]
        rng = np.random.default_rng((seed, i))
        if r["kind"] == "int":
            out.append({"p": rng.integers(2 ** 40 + 1, 2 ** 41, n).astype(np.int64), "t": np.arange(n, dtype=np.int64)})
            continue
        a = {"p": rng.standard_normal(n).astype(np.float32)}
        a["t"] = (a["p"] + 0.1 * rng.standard_normal(n)).astype(np.float32) if r["teacher"] else None
        if r["kind"] == "adamw":
            g0 = rng.standard_normal(n).astype(np.float32) * np.float32(1e-3 if i % 11 == 5 else 1.0)
            if r["step0"]:
                a["m"] = (0.5 * g0 + 0.3 * rng.standard_normal(n) * np.abs(g0)).astype(np.float32)
                a["v"] = (g0.astype(np.float64) ** 2 * (0.5 + rng.random(n))).astype(np.float32)
            else:
                a["m"], a["v"] = np.zeros(n, np.float32), np.zeros(n, np.float32)
            a["g"] = (np.random.default_rng((seed, i, call, 3)).standard_normal(n).astype(np.float32)
                      * np.float32(1e-3 if i % 11 == 5 else 1.0))
        out.append(a)
    norm = ref.total_norm([a["g"] for a, r in zip(out, spec) if in_norm(r)])
    if norm > 0:
        scale = np.float32(target_norm / norm)
        for a, r in zip(out, spec):
            if r["kind"] == "adamw":
                a["g"] = (a["g"] * scale).astype(np.float32)
    return out


def expected_slots(spec, grads):
    """The fp64 sum of squares of every BLOCK-element stretch of every clipped AdamW record's gradient, in table order: what
    the norm sweep (and the accumulate sweep) owes slot by slot.  grads[i]: record i's gradient."""
    out = []
    for r, g in zip(spec, grads):
        if in_norm(r):
            g = np.asarray(g, dtype=np.float64)
            out += [float((g[b:b + BLOCK] ** 2).sum()) for b in range(0, r["n"], BLOCK)]
    return np.array(out, dtype=np.float64)


def acc_offsets(spec, n_steps):
    """The accumulator as OptimTail lays it out: one stretch per step index, in step-index order, each starting on 16 bytes
    -> (offsets (n_steps,), n_acc).  A counter no record points at has an empty stretch."""
    n_of = {r["step_index"]: r["n"] for r in spec if r["kind"] == "adamw"}
    offs, at = [], 0
    for s in range(n_steps):
        offs.append(at)
        at += -(-n_of.get(s, 0) // 4) * 4
    return np.array(offs, dtype=np.int64), max(at, 4)


def to_ref_records(spec, arrays, grads=None):
    """The dicts _optim_tail_ref.tail takes, from what read() returned (and `grads` in the place of the arena's g: the summed
    gradient of a window)."""
    out = []
    for i, (r, a) in enumerate(zip(spec, arrays["rec"])):
        if r["kind"] != "adamw":
            out.append(dict(kind=r["kind"], p=a["p"], t=a["t"]))
            continue
        out.append(dict(kind="adamw", p=a["p"], g=a["g"] if grads is None else grads[i], m=a["m"], v=a["v"], t=a["t"],
                        group=r["group"], clipped=r["clipped"], step=int(arrays["steps"][r["step_index"]])))
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


class _Guarded:
    """A device buffer of named stretches with G guard elements around each."""

    def __init__(self, torch, dev, dtype, guard, parts):
        self.guard_value = np.array([guard], dtype=_bits(np.zeros(1, dtype)).dtype).view(dtype)[0]      # (given as bits)
        self.where, at = {}, G
        for name, init in parts:
            init = np.asarray(init, dtype=dtype)
            self.where[name] = (at, at + init.size)
            at += init.size + G
        host = np.full(at, self.guard_value, dtype=dtype)
        self.mask = np.ones(at, dtype=bool)
        for (name, init) in parts:
            a, b = self.where[name]
            host[a:b] = init
            self.mask[a:b] = False
        self.dev = torch.from_numpy(host).to(dev)
        self.itemsize = host.itemsize
        assert self.dev.data_ptr() % 16 == 0

    def ptr(self, name):
        return self.dev.data_ptr() + self.where[name][0] * self.itemsize

    def read(self):
        host = self.dev.cpu().numpy()
        ok = bool(np.all(_bits(host[self.mask]) == _bits(np.array([self.guard_value]))[0]))
        return {name: host[a:b].copy() for name, (a, b) in self.where.items()}, ok


class Table:
    """The spec on the device.  inputs: make_inputs(spec, seed) by default; n_steps: the length of `steps` (counters no record
    points at hold UNUSED_STEP).  The slots buffer holds plan["slots"] slots and G guard slots on either side."""

    def __init__(self, spec, seed=0, inputs=None, n_steps=None, dev=None):
        import torch
        from geot_amd import optim_tail as ot
        self.torch, self.ot = torch, ot
        self.dev = dev if dev is not None else torch.device("cuda:0")
        self.spec = spec
        self.inputs = inputs if inputs is not None else make_inputs(spec, seed)
        self.lay = layout(spec)
        self.n_steps = n_steps if n_steps is not None else n_steps_of(spec)
        assert self.n_steps >= n_steps_of(spec)
        # the arenas: guard pattern everywhere, then the tensors
        host = {"f32": np.full(self.lay["size"]["f32"], GUARD_F32_BITS, dtype=np.uint32).view(np.float32),
                "i64": np.full(self.lay["size"]["i64"], GUARD_I64, dtype=np.int64)}
        for r, a, row in zip(spec, self.inputs, self.lay["at"]):
            for key in tensors_of(r):
                assert a[key].size == r["n"] and not np.any(_bits(a[key]) == _bits(host[arena_of(r)][:1])[0]), "an input holds the guard"
                host[arena_of(r)][row[key]:row[key] + r["n"]] = a[key]
        self.arena = {k: torch.from_numpy(v.copy()).to(self.dev) for k, v in host.items()}
        assert all(t.data_ptr() % 16 == 0 for t in self.arena.values())
        # the tables
        self.table = np.zeros(len(spec), dtype=ot.RECORD)
        flags = flags_of(spec)
        for i, (r, row) in enumerate(zip(spec, self.lay["at"])):
            base, size = self.arena[arena_of(r)].data_ptr(), 8 if r["kind"] == "int" else 4
            for key in KEYS:
                self.table[i][key] = 0 if row[key] is None else base + size * row[key]
            self.table[i]["n"], self.table[i]["group"], self.table[i]["flags"] = r["n"], r["group"], flags[i]
            self.table[i]["step"] = r["step_index"]
        self._g = self.table["g"].copy()
        self.groups = [dict(g) for g in GROUPS]
        self.lr = torch.tensor([GROUPS[LR_PTR_GROUP]["lr"]], dtype=torch.float32, device=self.dev)
        self.group_table = np.zeros(len(GROUPS), dtype=ot.GROUP)
        for k, g in enumerate(GROUPS):
            gt = self.group_table[k]
            gt["beta1"], gt["beta2"] = g["betas"]
            gt["eps"], gt["weight_decay"] = g["eps"], g["weight_decay"]
            gt["lr"], gt["lr_ptr"] = (0.0, self.lr.data_ptr()) if k == LR_PTR_GROUP else (g["lr"], 0)
        # steps, scalars and slots in one guarded buffer; the gate and the accumulator in their own
        self.plan = self.plan_now()
        steps = np.full(self.n_steps, UNUSED_STEP, dtype=np.float32)
        for r in spec:
            if r["kind"] == "adamw":
                steps[r["step_index"]] = r["step0"]
        guard_f32 = np.array([GUARD_F32_BITS], np.uint32).view(np.float32)[0]
        self.aux = _Guarded(torch, self.dev, np.float32, GUARD_F32_BITS,
                            [("steps", steps), ("scalars", SCALARS0), ("slots", np.full(self.plan["slots"], guard_f32))])
        self.gate = _Guarded(torch, self.dev, np.int32, GUARD_I32, [("gate", (0, 0))])
        self.offsets, self.n_acc = acc_offsets(spec, self.n_steps)
        self.offs = torch.from_numpy(self.offsets).to(self.dev)
        self.acc = _Guarded(torch, self.dev, np.float32, GUARD_F32_BITS, [("acc", np.zeros(self.n_acc, np.float32))])
        assert self.acc.ptr("acc") % 16 == 0

    # ---- plans from the table's own pointers ---------------------------------------------------------------------------------
    def aligned_now(self):
        aligned = np.ones(len(self.table), dtype=np.int32)
        for key in KEYS:
            aligned &= (self.table[key] % 16 == 0)
        return aligned

    def plan_now(self):
        return self.ot.plan(self.table["n"], self.aligned_now(), self.table["flags"])

    def acc_plan_now(self):
        return self.ot.acc_plan(self.table["n"], self.aligned_now(), self.table["flags"])

    # ---- writing -------------------------------------------------------------------------------------------------------------
    def set_grads(self, grads):
        """Other gradients for the next call (grads[i] None: record i keeps what it has)."""
        torch = self.torch
        host = self.arena["f32"].cpu().numpy()
        for r, g, row in zip(self.spec, grads, self.lay["at"]):
            if g is not None and r["kind"] == "adamw" and r["n"]:
                assert g.dtype == np.float32 and g.size == r["n"]
                host[row["g"]:row["g"] + r["n"]] = g
        self.arena["f32"].copy_(torch.from_numpy(host))

    def _call(self, name, *args):
        from geot_amd.ext._common import call
        call(name, self.dev, *args)

    def _with_g(self, g_null):
        self.table["g"] = self._g
        for i in g_null:
            self.table["g"][i] = 0

    # ---- the sequences, as OptimTail.step and OptimTail._step_window issue them ------------------------------------------------
    def norm(self):
        self._call("geot_optim_tail_norm", len(self.table), self.table.ctypes.data, self.aux.ptr("slots"), self.plan["slots"])

    def ungated(self, max_norm=1.0, decay=DECAY):
        self._with_g(())
        pl, t, host, clip = self.plan_now(), len(self.table), self.table.ctypes.data, max_norm is not None
        if clip:
            self._call("geot_optim_tail_norm", t, host, self.aux.ptr("slots"), pl["slots"])
        self._call("geot_optim_tail_finish", t, host, int(clip), pl["slots"] if clip else 0, self.aux.ptr("slots") if clip else None,
                   max_norm if clip else 0.0, self.aux.ptr("steps"), self.n_steps, self.aux.ptr("scalars"))
        self._call("geot_optim_tail_update", t, host, len(self.group_table), self.group_table.ctypes.data, self.aux.ptr("scalars"),
                   self.aux.ptr("steps"), self.n_steps, decay if decay is not None else 0.0)
        return pl

    def gated(self, k, max_norm=1.0, decay=DECAY, g_null=()):
        self._with_g(g_null)
        pl, t, host, clip = self.acc_plan_now(), len(self.table), self.table.ctypes.data, max_norm is not None
        self._call("geot_optim_tail_accumulate", t, host, self.acc.ptr("acc"), self.offs.data_ptr(), self.n_acc, self.n_steps,
                   self.aux.ptr("slots") if clip else None, pl["slots"] if clip else 0)
        self._call("geot_optim_tail_acc_finish", t, host, int(clip), pl["slots"] if clip else 0,
                   self.aux.ptr("slots") if clip else None, max_norm if clip else 0.0, self.aux.ptr("steps"), self.n_steps,
                   self.aux.ptr("scalars"), self.gate.ptr("gate"), k)
        self._call("geot_optim_tail_acc_update", t, host, len(self.group_table), self.group_table.ctypes.data,
                   self.aux.ptr("scalars"), self.aux.ptr("steps"), self.n_steps, decay if decay is not None else 0.0,
                   self.acc.ptr("acc"), self.offs.data_ptr(), self.n_acc, self.gate.ptr("gate"))
        return pl

    # ---- readback ------------------------------------------------------------------------------------------------------------
    def read(self):
        """Everything a sequence may write: rec[i][key] (None: the record has no such tensor), steps, scalars, slots (the
        plan's; their guard slots are part of guards_intact), gate, acc, and guards_intact / guard_faults."""
        self.torch.cuda.synchronize(self.dev)
        host = {k: v.cpu().numpy() for k, v in self.arena.items()}
        faults = []
        if not np.all(_bits(host["f32"][self.lay["guard"]["f32"]]) == GUARD_F32_BITS):
            faults.append("float32 arena at %s" % np.flatnonzero(self.lay["guard"]["f32"] & (_bits(host["f32"]) != GUARD_F32_BITS))[:8])
        if not np.all(host["i64"][self.lay["guard"]["i64"]] == GUARD_I64):
            faults.append("int64 arena at %s" % np.flatnonzero(self.lay["guard"]["i64"] & (host["i64"] != GUARD_I64))[:8])
        out = {"rec": []}
        for r, row in zip(self.spec, self.lay["at"]):
            h = host[arena_of(r)]
            out["rec"].append({key: (h[row[key]:row[key] + r["n"]].copy() if row[key] is not None else
                                     (np.zeros(0, h.dtype) if key in keys_of(r) else None)) for key in KEYS})
        for name, buf in (("aux", self.aux), ("gate", self.gate), ("acc", self.acc)):
            parts, ok = buf.read()
            out.update(parts)
            if not ok:
                faults.append("guards of " + name)
        out["guards_intact"], out["guard_faults"] = not faults, faults
        return out


def acc_expected(spec, offsets, n_acc, sums):
    """The accumulator that holds sums[i] (None: nothing) in record i's stretch and zeros elsewhere."""
    out = np.zeros(n_acc, dtype=np.float32)
    for r, s in zip(spec, sums):
        if r["kind"] == "adamw" and s is not None:
            out[offsets[r["step_index"]]:offsets[r["step_index"]] + r["n"]] = s
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _cycle(row):
    return dict(group=row % 4, step0=STEP0S[row % 3])


def case_norm_packing():
    """2 CAP + 1 records, even rows clipped AdamW (CAP + 1 of them: the norm sweep's second launch holds one record), odd
    rows unclipped AdamW / EMA-only / int64 in turn; three of the first CAP clipped records take more than one workgroup, so
    the second norm launch's first slot is not its first record's number.  One EMA-only record carries the CLIPPED flag (it is
    no part of the norm), one clipped record's gradient is misaligned."""
    t = 2 * CAP + 1
    big = {4: BLOCK + 1, 20: 2 * BLOCK, 60: 3 * BLOCK + 7}
    spec = []
    for row in range(t):
        n = big.get(row, 1 + row % 5)
        step_index = (row * 37 + 11) % t              # a fixed permutation of the rows (t = 97 is prime)
        if row % 2 == 0:
            spec.append(rec("adamw", n, clipped=True, teacher=row % 5 != 4, step_index=step_index,
                            misalign=("g",) if row == 8 else (), **_cycle(row)))
        elif row % 6 == 1:
            spec.append(rec("adamw", n, clipped=False, teacher=row % 5 != 4, step_index=step_index, **_cycle(row)))
        elif row % 6 == 3:
            spec.append(rec("ema", n, clipped=row == 9))
        else:
            spec.append(rec("int", n))
    return spec


def case_empty_records():
    """Records without elements wherever ot_find can meet them: row 0, three in a row in mid-launch, the last row of a launch,
    the first row of the next, the last rows of the table -- of every kind, and one of them in front of a record of more
    than one workgroup."""
    t = CAP + 12
    empty = {0: "adamw", 20: "adamw", 21: "ema", 22: "int", CAP - 1: "adamw", CAP: "adamw", t - 2: "ema", t - 1: "adamw"}
    spec = []
    for row in range(t):
        kind = empty.get(row, ("adamw", "adamw", "ema", "adamw", "int")[row % 5])
        n = 0 if row in empty else (BLOCK + 1 if row in (1, 23, CAP + 1) else 1 + row % 5)
        if row in (1, 23, CAP + 1):
            kind = "adamw"
        spec.append(rec(kind, n, clipped=row % 3 != 2, teacher=row % 4 != 3, step_index=(row * 7 + 3) % t, **_cycle(row)))
    return spec


def case_unissued_launch():
    """CAP records without elements, then one of 5: the first launch of every sweep is not issued."""
    spec = [rec("adamw", 0, clipped=True, step_index=CAP - row, **_cycle(row)) for row in range(CAP)]
    return spec + [rec("adamw", 5, clipped=True, step_index=0, step0=3, group=1)]


def case_many_counters():
    """STEP_CAP + 1 AdamW records: a second finish launch of one counter; step indices a fixed permutation into a `steps` of
    N_STEPS_MANY entries, six of which no record points at."""
    return [rec("adamw", 1 + row % 4, clipped=row % 2 == 0, teacher=row % 3 != 2, step_index=(row * 5 + 7) % N_STEPS_MANY,
                **_cycle(row)) for row in range(STEP_CAP + 1)]


N_STEPS_MANY = STEP_CAP + 7           # 903 = 3 * 7 * 43: 5 is coprime, row -> (5 row + 7) mod 903 is one to one


def case_misaligned():
    """Each pointer misaligned alone, and an aligned twin of every record."""
    spec, row = [], 0
    for key in KEYS:
        for mis in ((key,), ()):
            spec.append(rec("adamw", BLOCK + 1, clipped=row % 2 == 0, teacher=True, step_index=row, misalign=mis, **_cycle(row)))
            row += 1
    for key in ("p", "t"):
        for mis in ((key,), ()):
            spec.append(rec("ema", BLOCK + 3, misalign=mis))
    return spec


QUAD_TAIL_COUNTS = tuple(range(BLOCK - 3, BLOCK + 4)) + (2 * BLOCK + 1, 2 * BLOCK + 2, 2 * BLOCK + 3)


def case_quad_tails():
    """Aligned records on either side of a whole quad and a whole workgroup, with a teacher and without."""
    spec = []
    for row, n in enumerate(QUAD_TAIL_COUNTS):
        spec.append(rec("adamw", n, clipped=row % 3 != 2, teacher=row % 2 == 0, step_index=len(QUAD_TAIL_COUNTS) - 1 - row,
                        **_cycle(row)))
        spec.append(rec("ema", n))
    return spec


INT64_COUNTS = (BLOCK - 1, BLOCK, BLOCK + 3, 2 * BLOCK + 1)


def case_int64():
    """int64 records of more than one workgroup, the last one behind row CAP."""
    spec = [rec("int", n) for n in INT64_COUNTS[:3]]
    for row in range(3, CAP + 1):
        spec.append(rec("adamw", 1 + row % 3, clipped=row % 4 == 1, step_index=row, **_cycle(row)) if row % 2 else rec("ema", 2))
    return spec + [rec("int", INT64_COUNTS[3])]


SOMETIMES = 2 * CAP + 1               # case_window: the row whose gradient is there in call 1 of every three only


def case_window():
    """case_norm_packing plus one clipped record of two workgroups that has a gradient in one call of three."""
    spec = case_norm_packing()
    assert len(spec) == SOMETIMES
    return spec + [rec("adamw", BLOCK + 2, clipped=True, teacher=True, step_index=SOMETIMES, step0=3, group=1)]


def case_refusals():
    return [rec("adamw", 5, clipped=True, step_index=1, step0=3, group=1), rec("ema", 3),
            rec("adamw", BLOCK + 1, clipped=True, teacher=False, step_index=0, group=3), rec("int", 4),
            rec("adamw", 2, clipped=False, step_index=2, step0=10, group=2)]


CASES = {"norm_packing": case_norm_packing, "empty_records": case_empty_records, "unissued_launch": case_unissued_launch,
         "many_counters": case_many_counters, "misaligned": case_misaligned, "quad_tails": case_quad_tails,
         "int64": case_int64, "window": case_window, "refusals": case_refusals}
N_STEPS = {"many_counters": N_STEPS_MANY, "norm_packing": 2 * CAP + 4, "window": 2 * CAP + 5}
