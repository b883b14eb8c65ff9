"""The tests' own referee for the FixMatch views (geot_amd/openpoints/dataset/fixmatch_batch.py): the contract block
restated with numpy, once in fp64 (what the bounds are measured against) and once as the fp32 statements the kernel
executes, given its statistics.

With r (m, 3) the sampled, pc_norm-ed points of one scan, g the gravity column and (s, R, t) the view's parameters:

    q       = r * s                          one fp32 rounding per element
    x       = q                              the scaled, un-centred cloud
    heights = q[:, g:g+1] - min(q[:, g])
    c       = q - mean(q, axis=0)
    mx      = max_i sqrt(sum_k c[i,k]^2)
    pos     = c / mx
    pos     = pos @ R.T + t                  strong view only
"""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)      # 2^-23


def scaled(r, s):
    """q: the one fp32 multiply every implementation shares (identical inputs, one rounding: compared exactly)."""
    return (np.asarray(r, np.float32) * np.asarray(s, np.float32)).astype(np.float32)


def view_f64(r, s, R, t, g=1, rotate=True, translate=True):
    """fp64 restatement from the fp32 q on: dict(x, heights fp32 -- exact by construction -- and center, scale, pos_pre, pos
    in fp64).  pos_pre is pos before the rotation and shift."""
    q32 = scaled(r, s)
    q = q32.astype(np.float64)
    center = q.mean(axis=0)
    c = q - center
    with np.errstate(invalid="ignore", divide="ignore"):
        mx = np.sqrt((c * c).sum(axis=1)).max()
        pre = c / mx
    pos = pre
    if rotate:
        pos = pos @ np.asarray(R, np.float64).T
    if translate:
        pos = pos + np.asarray(t, np.float64)
    return {"x": q32, "heights": (q32[:, g:g + 1] - q32[:, g].min()).astype(np.float32), "center": center, "scale": mx,
            "pos_pre": pre, "pos": pos}


def pos_f32_given_stats(r, s, R, t, center, scale, rotate=True, translate=True):
    """The kernel's fp32 statements with ITS mean and maximum norm fed in: every step is one IEEE fp32 operation (numpy does
    not contract), so the result must carry the kernel's bits."""
    q = scaled(r, s)
    center = np.asarray(center, np.float32)
    scale = np.float32(scale)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = ((q - center) / scale).astype(np.float32)
    if rotate:
        R = np.asarray(R, np.float32)
        p = np.stack([(p[:, 0] * R[k, 0] + p[:, 1] * R[k, 1]) + p[:, 2] * R[k, 2] for k in range(3)], axis=1).astype(np.float32)
    if translate:
        p = (p + np.asarray(t, np.float32)).astype(np.float32)
    return p


def norm_f32(q, center):
    """mx as the kernel forms it: sqrtf((cx^2 + cy^2) + cz^2), maximised."""
    c = (np.asarray(q, np.float32) - np.asarray(center, np.float32)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]).max()


def mean_tree_f64(q, threads=512, wave=64):
    """The column means as the views kernels sum them (csrc/views.h), before the one rounding to fp32: thread t adds its
    points t, t + 512, ... in index order onto 0 in fp64, a butterfly over each 64-lane wave (v += v[lane ^ d], d = 32 .. 1),
    the wave sums added in wave order onto 0, one division by m.  Every step is one fp64 add, so numpy repeats it exactly."""
    q = np.asarray(q, np.float32).astype(np.float64)
    m = q.shape[0]
    part = np.zeros((threads, 3))
    for k0 in range(0, m, threads):
        chunk = q[k0:k0 + threads]
        part[:len(chunk)] = part[:len(chunk)] + chunk
    v, lane = part.reshape(threads // wave, wave, 3), np.arange(wave)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ d]
    tot = np.zeros(3)
    for w in range(threads // wave):
        tot = tot + v[w, 0]
    return tot / m


def rotate_f64(pre, R, t):
    """fp64 rotation and shift of a given pre-rotation pos."""
    return np.asarray(pre, np.float64) @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
