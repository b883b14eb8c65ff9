"""What the run-time-C NTM tests share (csrc/ntm_generic.hip): the launch planner restated in Python, the query
geot_ntm_generic_plan as a dict, the branches of the kernels a (shape, class count, form) reaches, the case table of
tests/test_ntm_generic_kernels_gpu.py, and the searches that find its large shapes from the plan.

The planner, as the launchers read it (gen_sig_plan):
  * GEOT_NTM_GENERIC = m... | r... | w... forces the matrix-core, lane-per-point or wave-per-point form; unset: MFMA from c = 6.
  * MFMA needs 4 <= B N c^2 < 2^30 (the kernel's 32-bit offsets; its gradient loads are clamped to the last 4 elements),
    otherwise rows; rows needs B N c^2 < 4 (2^31 - 1), otherwise (or when forced) wave.
  * MFMA: CPAD = 8 | 16 | 32, NG = 32 / CPAD heads per row tile, nkt = ceil(c / NG) row tiles, ng = ceil(c / 8) groups of four K
    steps; ksplit = the first split from 1 whose weights fit 160 KB beside the 16 waves' tiles and whose last round of waves
    is >= 85 % full, or 4, or nkt when the loop runs out; nb = min(cus // ksplit, ceil(tiles / 16)) workgroups per range.
  * rows: CP = c rounded up to 8, 256 points per workgroup, at most 8 cus workgroups.
  * wave: 4 points per workgroup, (c + 1) c^2 floats of LDS, at most clamp(160 KB // (lds + 512), 1, 8) cus workgroups.
  * gen_correct_*: ceil(points / 4) workgroups, at most 2048."""
import ctypes

NONE, WAVE, ROWS, MFMA, C17, REFUSED = 0, 1, 2, 3, 4, -1
PLAN_FIELDS = ("form", "cp", "tails", "ksplit", "blocks", "lds", "correct_blocks")
GEN_MW, GEN_RS = 16, 36
LDS_MAX = 160 * 1024
ENVS = {None: None, "m": "mfma", "r": "rows", "w": "wave"}


def plan(lib, b, n, c, backward=0, cus=256):
    """geot_ntm_generic_plan as (form, dict or None)"""
    out = (ctypes.c_longlong * len(PLAN_FIELDS))(*([-7] * len(PLAN_FIELDS)))
    form = lib.geot_ntm_generic_plan(int(b), int(n), int(c), int(backward), int(cus), out, len(PLAN_FIELDS))
    if form == 0:
        assert list(out) == [-7] * len(PLAN_FIELDS)
        return 0, None
    d = dict(zip(PLAN_FIELDS, (int(v) for v in out)))
    assert d["form"] == form
    return form, d


def gen_blocks(pts):
    return max(1, min(2048, (pts + 3) // 4))


def mfma_geometry(c):
    cpad = 8 if c <= 8 else (16 if c <= 16 else 32)
    NG = 32 // cpad
    return cpad, NG, (c + NG - 1) // NG, (c + 7) // 8


def mfma_lds(c, ks):
    _, _, nkt, ng = mfma_geometry(c)
    per = (nkt + ks - 1) // ks
    return 4 * (per * ng * 256 + per * 32 + GEN_MW * 32 * GEN_RS)


def plan_ref(b, n, c, backward=0, cus=256, env=None):
    """the planner restated; env: the value of GEOT_NTM_GENERIC or None"""
    if b < 1 or n < 1 or c < 1 or c > 32:
        return 0, None
    pts = b * n
    d = dict(form=C17, cp=0, tails=0, ksplit=0, blocks=0, lds=0, correct_blocks=0)
    if c == 17:
        return C17, d
    d["correct_blocks"] = gen_blocks(pts)
    elems = pts * c * c
    k = env[0] if env else ""
    want_mfma = True if k == "m" else (False if k in ("r", "w") else c >= 6)
    if want_mfma and 4 <= elems < 2 ** 30:
        cpad, NG, nkt, ng = mfma_geometry(c)
        tiles = (pts + 31) // 32
        ks = 1
        while ks < nkt:
            if mfma_lds(c, ks) <= LDS_MAX:
                waves = cus // ks * GEN_MW
                if waves > 0:
                    rounds = (tiles + waves - 1) // waves
                    if tiles <= waves or tiles * 100 >= rounds * waves * 85 or ks >= 4:
                        break
            ks += 1
        d.update(form=MFMA, cp=cpad, tails=int(c % 4 != 0), ksplit=ks, lds=mfma_lds(c, ks))
        if d["lds"] > LDS_MAX or cus < ks:
            d["form"] = REFUSED
            return REFUSED, d
        d["blocks"] = min(cus // ks, (tiles + GEN_MW - 1) // GEN_MW) * ks
    elif k != "w" and elems < 0x7fffffff * 4:
        cp = (c + 7) // 8 * 8
        d.update(form=ROWS, cp=cp, ksplit=1, lds=4 * (((c * c + 3) & ~3) + 4 * 64 * (cp + 1)), blocks=min((pts + 255) // 256, 8 * cus))
    else:
        lds = 4 * (c + 1) * c * c
        per_cu = max(1, min(8, LDS_MAX // (lds + 512)))
        d.update(form=WAVE, ksplit=1, lds=lds, blocks=min((pts + 3) // 4, per_cu * cus))
    return d["form"], d


# ---- which branches of the kernels a case reaches ---------------------------------------------------------------------------
def tail_shift(c):
    """TAILS, backward: by how many elements the clamped 16-byte load of the last piece of the last point began early"""
    _, NG, nkt, _ = mfma_geometry(c)
    segk = min(NG, c - (nkt - 1) * NG) * c
    return (4 - segk % 4) % 4


def classes(b, n, c, env=None, cus=256):
    """the in-kernel branches geot_ntm_sig_t_mean[_grad_raw] takes at this shape, and those of the gen_correct kernels"""
    form, p = plan_ref(b, n, c, 0, cus, env)
    pts = b * n
    got = set()
    if form == MFMA:
        cpad, NG, nkt, ng = mfma_geometry(c)
        tiles = (pts + 31) // 32
        nb = p["blocks"] // p["ksplit"]
        got |= {"mfma", "mfma cpad %d" % cpad, "mfma ksplit %d" % min(p["ksplit"], 4), "mfma tails" if p["tails"] else "mfma whole (AHEAD)"}
        if p["tails"] and pts * c * c >= 4:
            got.add("mfma sh %d" % tail_shift(c))
        if c % NG:
            got.add("mfma partial last row tile")
        if cpad == 32:
            got.add("mfma ng %d" % ng)
            got.add("mfma fourth block skipped" if c <= 24 else "mfma fourth block live")
        if p["ksplit"] == nkt and nkt > 1:
            got.add("mfma ksplit = nkt")
        if p["ksplit"] > 1 and nkt % p["ksplit"]:
            got.add("mfma uneven ranges")
        if p["ksplit"] > 1 and mfma_lds(c, 1) > LDS_MAX:
            got.add("mfma ksplit from the LDS gate")
        if tiles > nb * GEN_MW:
            got.add("mfma second point tile")
        if pts % 32:
            got.add("mfma partial point tile")
        if b > 1 and n % 32:
            got.add("mfma batch boundary inside a tile")
    elif form == ROWS:
        got |= {"rows", "rows cp %d" % p["cp"], "rows dq 0" if 64 % c == 0 else "rows wrap"}
        if pts > p["blocks"] * 256:
            got.add("rows second trip")
        if pts % 64:
            got.add("rows partial tile")
        if b > 1 and n % 64:
            got.add("rows batch boundary inside a tile")
    elif form == WAVE:
        got |= {"wave", "wave odd c (dead half-wave)" if c % 2 else "wave even c"}
        if p["lds"] > 64 * 1024:
            got.add("wave big lds")
        if pts > p["blocks"] * 4:
            got.add("wave second trip")
    if c != 17 and pts > gen_blocks(pts) * 4:
        got.add("correct second trip")
    return got


# ---- the case table ---------------------------------------------------------------------------------------------------------
CLASS_COUNTS = [1, 2, 3, 5, 6, 7, 8, 9, 11, 12, 14, 16, 18, 20, 21, 23, 24, 25, 31, 32]
SMALL_SHAPES = [(1, 1), (5, 7), (1, 32), (1, 33), (1, 64), (1, 65), (2, 1001)]
# the seed of R.sig_inputs(b, n, c, amp=2.0) per (c, shape): the first of 0..2 whose inputs meet the region shares (>= 1 % each
# at 33 points and more) and the edge share (<= 1e-4); found by tests/test_ntm_generic_plan_cpu.py's own rule (seed_of below)
SEEDS = {(2, 2, 1001): 2, (5, 1, 64): 1, (12, 1, 33): 1, (14, 1, 32): 1, (16, 1, 64): 1, (24, 1, 33): 1, (31, 1, 33): 1, (32, 1, 64): 1}


def seed_of(c, b, n):
    return SEEDS.get((c, b, n), 0)


def forms_of(c):
    """the forms a class count is run under: (env, form) -- the default and every forced form that differs from it"""
    default = MFMA if c >= 6 else ROWS
    out = [(None, default)]
    for env, form in (("mfma", MFMA), ("rows", ROWS), ("wave", WAVE)):
        if form != default:
            out.append((env, form))
    return out


def small_form(b, n, c, env):
    """the form a small case must plan as: forced MFMA with fewer than four output elements goes to rows"""
    form = dict(forms_of(c))[env]
    return ROWS if form == MFMA and b * n * c * c < 4 else form


# what the table must reach (the census of tests/test_ntm_generic_plan_cpu.py)
REQUIRED_CLASSES = [
    "mfma cpad 8", "mfma cpad 16", "mfma cpad 32", "mfma tails", "mfma whole (AHEAD)", "mfma sh 0", "mfma sh 1", "mfma sh 2", "mfma sh 3",
    "mfma partial last row tile", "mfma ng 3", "mfma ng 4", "mfma fourth block skipped", "mfma fourth block live",
    "mfma ksplit 1", "mfma ksplit 2", "mfma ksplit 3", "mfma ksplit = nkt", "mfma uneven ranges", "mfma ksplit from the LDS gate",
    "mfma second point tile", "mfma partial point tile", "mfma batch boundary inside a tile",
    "rows cp 8", "rows cp 16", "rows cp 24", "rows cp 32", "rows dq 0", "rows wrap", "rows second trip", "rows partial tile",
    "rows batch boundary inside a tile",
    "wave", "wave odd c (dead half-wave)", "wave even c", "wave big lds", "wave second trip", "correct second trip"]


# ---- large shapes, searched from the planner at the device's CU count ------------------------------------------------------
def _smallest(pred, lo, hi, step=1):
    for pts in range(lo, hi, step):
        if pred(pts):
            return pts
    raise AssertionError("no point count in [%d, %d) has the property" % (lo, hi))


def large_mfma_second_tile(c, cus):
    """the smallest (3, n), 3 n no multiple of 32, at which a wave of the MFMA form walks two point tiles"""
    def ok(n):
        f, p = plan_ref(3, n, c, 0, cus)
        return f == MFMA and 3 * n % 32 and "mfma second point tile" in classes(3, n, c, None, cus)
    return 3, _smallest(ok, 1, 1 << 20, 2)


def large_mfma_ksplit3(c, cus):
    """the smallest (3, n) at which the planner picks ksplit = 3 with uneven ranges, or None on this CU count"""
    for n in range(1, 1 << 18, 2):
        f, p = plan_ref(3, n, c, 0, cus)
        if f == MFMA and p["ksplit"] == 3 and 3 * n % 32 and {"mfma uneven ranges"} <= classes(3, n, c, None, cus):
            return 3, n
    return None


def large_rows_second_trip(c, cus):
    pts = 8 * cus * 256 + 65                      # a second trip of block 0's first two waves, the second one partial
    assert "rows second trip" in classes(1, pts, c, "rows", cus) and pts % 64
    return 1, pts


def large_wave_second_trip(c, cus, b=3):
    def ok(n):
        return "wave second trip" in classes(b, n, c, "wave", cus) and (b * n) % 4
    return b, _smallest(ok, 1, 1 << 20, 2 if b > 1 else 1)


CORRECT_LARGE = (3, 2741)                         # 8223 points > 2048 workgroups x 4
