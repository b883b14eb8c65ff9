"""numpy float32 restatement of geot_view_draw's contract (include/geot_hip.h), written from the contract: of geot_amd only the
ATTRIBUTES of a ViewProgram's steps are read (the bounds a list was configured with).  Every arithmetic statement is one
float32 operation on float32 operands, so numpy rounds where the kernel rounds and the results agree bit for bit.

    uniform(w), uniform_open(w)                  (w >> 8) 2^-24 and ((w >> 8) + 1) 2^-24
    log_u24(n)                                   ln(n 2^-24), n in [1, 2^24]
    radius(w)                                    sqrt(-2 ln uniform_open(w))
    sincos_turns(t)                              (cos, sin) of t turns
    noise_rows(m, seed, draw, tag, std, clip)    (m, 3) finished jitter noise
    draw(program, m, seed, draw_id, view)        what ViewProgram.draw(m) returns: one dict per transform of the list
"""
import numpy as np

import _sample_draw_ref as sd

F = np.float32
Q_SCALE, Q_MIRROR, Q_SHIFT, Q_ROTATE, Q_FLIP, Q_DROP, Q_NOISE, Q_PERMASK = range(8)
ORDERS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
_BASE = {"PointCloudScaling_s": "PointCloudScaling", "PointCloudTranslation_s": "PointCloudTranslation",
         "PointCloudScaleAndTranslate_s": "PointCloudScaleAndTranslate", "PointCloudJitter_s": "PointCloudJitter",
         "PointCloudRotation_s": "PointCloudRotation"}


def tag(view, pos, quantity):
    return 0x40000000 | (view << 24) | (pos << 8) | quantity


def words(element, view, pos, quantity, seed, draw_id):
    """The four Philox words of (element, tag, d lo, d hi) under the key (seed lo, seed hi), as uint64 arrays < 2^32.
    element and draw_id broadcast; a draw id is taken mod 2^64."""
    seed = int(seed) & (2 ** 64 - 1)
    if not isinstance(draw_id, np.ndarray):
        draw_id = int(draw_id) & (2 ** 64 - 1)
    d = np.asarray(draw_id, dtype=np.uint64)
    return sd.philox4x32(np.asarray(element, dtype=np.uint64), tag(view, pos, quantity), d & sd.LOW, d >> sd.S32,
                         seed & 0xFFFFFFFF, seed >> 32)


def uniform(w):
    return (np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(F) * F(2.0 ** -24)


def uniform_open(w):
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(8)) + np.uint64(1)).astype(F) * F(2.0 ** -24)


def log_u24(n):
    n = np.asarray(n, dtype=np.int64)
    e = np.frexp(n.astype(np.float64))[1] - 1                 # the exponent of the integer: n = 2^e f, f in [1, 2)
    f = np.ldexp(n.astype(F), -e).astype(F)
    big = f > F(1.41421354)
    f = np.where(big, f * F(0.5), f)
    e = e + big
    s = (f - F(1)) / (f + F(1))
    w = s * s
    p = w * F(0.0909090936) + F(0.111111112)
    p = w * p + F(0.142857149)
    p = w * p + F(0.200000003)
    p = w * p + F(0.333333343)
    p = w * p
    lnf = (s + s * p) * F(2)
    return ((e - 24).astype(F) * F(0.693147182) + lnf).astype(F)


def radius(w):
    n = (np.asarray(w, dtype=np.uint64) >> np.uint64(8)) + np.uint64(1)
    return np.sqrt((F(0) - log_u24(n)) * F(2)).astype(F)


def sincos_turns(t):
    t = np.asarray(t, dtype=F)
    y = t * F(4)
    n = (y + F(12582912)) - F(12582912)
    r = y - n
    q = n.astype(np.int32) & 3
    a = r * F(1.57079637)
    w = a * a
    ps = w * F(2.75573188e-06) + F(-0.000198412701)
    ps = w * ps + F(0.00833333377)
    ps = w * ps + F(-0.166666672)
    ps = w * ps
    sn = a + a * ps
    pc = w * F(-2.75573188e-07) + F(2.48015876e-05)
    pc = w * pc + F(-0.00138888892)
    pc = w * pc + F(0.0416666679)
    pc = w * pc + F(-0.5)
    cs = w * pc + F(1)
    zero = F(0)
    c = np.select([q == 0, q == 1, q == 2], [cs, zero - sn, zero - cs], sn)
    s = np.select([q == 0, q == 1, q == 2], [sn, cs, zero - sn], zero - cs)
    return c.astype(F), s.astype(F)


def normals3(w0, w1, w2, w3):
    """(.., 3) standard normals of one generator call per point, before sigma and the clamp."""
    c0, s0 = sincos_turns(uniform(w1))
    c1, _ = sincos_turns(uniform(w3))
    r0, r1 = radius(w0), radius(w2)
    return np.stack([r0 * c0, r0 * s0, r1 * c1], axis=-1).astype(F)


def noise_rows(m, view, pos, seed, draw_id, std, clip):
    z = normals3(*words(np.arange(m), view, pos, Q_NOISE, seed, draw_id))
    v = z * F(std)
    lo = F(0) - F(clip)
    return np.minimum(np.maximum(v, lo), F(clip)).astype(F)


def scale(step, view, pos, seed, draw_id, form):
    ws = words(0, view, pos, Q_SCALE, seed, draw_id)
    wm = words(0, view, pos, Q_MIRROR, seed, draw_id)
    lo, span = F(step.scale_min), F(F(step.scale_max) - F(step.scale_min))
    mirror = np.asarray(step.mirror, dtype=F)
    out = np.empty(3, F)
    for k in range(3):
        v = F(F(uniform(ws[k if step.anisotropic else 0]) * span) + lo)
        if form:
            u = uniform(wm[k])
            if form == 1:
                mir = F(1) if u > mirror[k] else F(-1)
            else:
                mir = F(F((F(1) if u > F(0.5) else F(-1)) * mirror[k]) + F(F(1) - mirror[k]))
            v = F(v * mir)
        out[k] = v if step.scale_xyz[k if step.anisotropic else 0] else F(1)
    return out


def shift(step, view, pos, seed, draw_id, centred):
    w = words(0, view, pos, Q_SHIFT, seed, draw_id)
    amount = np.asarray(step.shift, dtype=F)
    u = np.array([uniform(w[k]) for k in range(3)], dtype=F)
    if centred:
        return (((u - F(0.5)) * F(2)) * amount).astype(F)
    return (u * amount).astype(F)


def matmul(a, b):
    o = np.empty((3, 3), F)
    for i in range(3):
        for j in range(3):
            o[i, j] = F(F(F(a[i, 0] * b[0, j]) + F(a[i, 1] * b[1, j])) + F(a[i, 2] * b[2, j]))
    return o


def rotation(angle_pi, view, pos, seed, draw_id):
    w = words(0, view, pos, Q_ROTATE, seed, draw_id)
    mats = []
    for ax in range(3):
        v = F(F(uniform(w[ax]) * F(2)) - F(1))
        c, s = sincos_turns(F(F(F(angle_pi[ax]) * v) * F(0.5)))
        c, s = F(c), F(s)
        ns = F(F(0) - s)
        mm = np.eye(3, dtype=F)
        if ax == 0:
            mm[1, 1], mm[1, 2], mm[2, 1], mm[2, 2] = c, ns, s, c
        elif ax == 1:
            mm[0, 0], mm[0, 2], mm[2, 0], mm[2, 2] = c, s, ns, c
        else:
            mm[0, 0], mm[0, 1], mm[1, 0], mm[1, 1] = c, ns, s, c
        mats.append(mm)
    order = ORDERS[((int(w[3]) >> 8) * 6) >> 24]
    return matmul(matmul(mats[order[0]], mats[order[1]]), mats[order[2]]), order


def flips(step, view, pos, seed, draw_id):
    w = words(0, view, pos, Q_FLIP, seed, draw_id)
    out = []
    if uniform(w[0]) < F(step.aug_prob):
        for k, ax in enumerate(step.horz_axes):
            if uniform(w[1 + k]) < F(0.5):
                out.append(ax)
    return out


def drop(step, view, pos, seed, draw_id):
    return bool(uniform(words(0, view, pos, Q_DROP, seed, draw_id)[0]) < F(step.color_drop))


def point_mask(step, m, view, pos, seed, draw_id):
    u = uniform(words(np.arange(m), view, pos, Q_PERMASK, seed, draw_id)[0])
    return (u > F(step.color_drop)).astype(F)


def draw(program, m, seed, draw_id, view=0):
    """What program.draw(m) returns, drawn as geot_view_draw draws it for a slot with this draw id and view."""
    out = []
    for pos, step in enumerate(program.steps):
        base = _BASE.get(step.name, step.name)
        a = (view, pos, seed, draw_id)
        if base == "PointCloudScaling":
            out.append({"scale": scale(step, *a, 1 if step.use_mirroring else 0)})
        elif base == "PointCloudTranslation":
            out.append({"t": shift(step, *a, False)})
        elif base == "PointCloudScaleAndTranslate":
            out.append({"scale": scale(step, *a, 1 if step.use_mirroring else 0), "t": shift(step, *a, True)})
        elif base == "PointCloudJitter":
            out.append({"noise": noise_rows(m, *a, step.noise_std, step.noise_clip)})
        elif base == "PointCloudScaleAndJitter":
            out.append({"scale": scale(step, *a, 2), "noise": noise_rows(m, *a, step.noise_std, step.noise_clip)})
        elif base == "PointCloudRotation":
            out.append({"R": rotation(step.angle_pi, *a)[0]})
        elif base == "RandomHorizontalFlip":
            out.append({"flip": flips(step, *a)})
        elif base == "ChromaticDropGPU":
            out.append({"drop": drop(step, *a)})
        elif base == "ChromaticPerDropGPU":
            out.append({"mask": point_mask(step, m, *a)})
        else:
            out.append({})
    return out
