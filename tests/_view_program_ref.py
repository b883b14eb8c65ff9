"""The tests' own referee for transform lists as view programs (geot_amd/openpoints/dataset/view_program.py,
csrc/view_program.hip), extending tests/_views_ref.py: the reference's transform classes restated with numpy, working from
the class NAMES, the kwargs and one view's recorded draws -- not from the compiler's ops, so that a wrong aliasing decision
of the compiler shows.  The aliasing is literal: data['x'] and data['pos'] start as ONE array, in-place statements change
both, rebinding statements separate them.

    run(raw, names, kwargs, params, np.float64)            what the bounds are measured against
    run(raw, names, kwargs, params, np.float32, stats=...)  the fp32 statements the kernel executes (numpy does not contract),
                                                            with ITS mean / maximum norm fed in: must carry the kernel's bits
"""
import numpy as np

_BASE = {"PointCloudScaling_s": "PointCloudScaling", "PointCloudTranslation_s": "PointCloudTranslation",
         "PointCloudScaleAndTranslate_s": "PointCloudScaleAndTranslate", "PointCloudJitter_s": "PointCloudJitter",
         "PointCloudRotation_s": "PointCloudRotation"}


def _mean(pos, dtype):
    """fp64 column means, rounded once to the working type (the kernel: fp64 sums, one division, one rounding)."""
    return pos.astype(np.float64).mean(axis=0).astype(dtype)


def _max_norm(pos):
    with np.errstate(invalid="ignore"):
        return np.sqrt((pos[:, 0] * pos[:, 0] + pos[:, 1] * pos[:, 1]) + pos[:, 2] * pos[:, 2]).max()


def run(raw, names, kwargs, params, dtype=np.float64, stats=None):
    """One view -> dict(pos (m, 3), x (m, 3), heights (m, 1) or None, x_is_pos, center, scale).  params: one dict per name
    (ViewProgram.draw's layout: scale, t, noise, R, flip, drop, mask).  stats: (center (3,), scale) to use instead of the
    computed mean / maximum norm in every centring transform (a list with one of them)."""
    data = {"pos": np.array(raw, dtype=dtype)}
    data["x"] = data["pos"]
    center, scale = np.zeros(3, dtype), dtype(1)
    f = lambda v: np.asarray(v, dtype=np.float32).astype(dtype)     # noqa: E731 -- a drawn fp32 value in the working type
    for name, p in zip(names, params):
        base = _BASE.get(name, name)
        if base in ("PointsToTensor", "PointCloudToTensor"):
            continue
        if base == "PointCloudScaling":
            data["pos"] *= f(p["scale"])
        elif base == "PointCloudCenterAndNormalize":
            g = int(kwargs.get("gravity_dim", 2))
            height = data["pos"][:, g:g + 1]
            data["heights"] = height - height.min()
            center, scale = np.zeros(3, dtype), dtype(1)
            if kwargs.get("centering", True):
                center = _mean(data["pos"], dtype) if stats is None else np.asarray(stats[0], dtype)
                data["pos"] = data["pos"] - center
            if kwargs.get("normalize", True):
                scale = _max_norm(data["pos"]) if stats is None else dtype(stats[1])
                with np.errstate(invalid="ignore", divide="ignore"):
                    data["pos"] = data["pos"] / scale
        elif base == "PointCloudXYZAlign":
            g = int(kwargs.get("gravity_dim", 2))
            center, scale = (_mean(data["pos"], dtype) if stats is None else np.asarray(stats[0], dtype)), dtype(1)
            data["pos"] -= center
            data["pos"][:, g] -= data["pos"][:, g].min()
        elif base == "PointCloudTranslation":
            data["pos"] += f(p["t"])
        elif base == "PointCloudScaleAndTranslate":
            data["pos"] = data["pos"] * f(p["scale"]) + f(p["t"])
        elif base == "PointCloudJitter":
            data["pos"] += f(p["noise"])
        elif base == "PointCloudScaleAndJitter":
            data["pos"] = data["pos"] * f(p["scale"]) + f(p["noise"])
        elif base == "PointCloudRotation":
            R, q = f(p["R"]), data["pos"]
            if dtype == np.float32:         # the kernel's order: ((p0 R[k][0] + p1 R[k][1]) + p2 R[k][2])
                data["pos"] = np.stack([(q[:, 0] * R[k, 0] + q[:, 1] * R[k, 1]) + q[:, 2] * R[k, 2] for k in range(3)], axis=1)
            else:
                data["pos"] = q @ R.T
        elif base == "RandomHorizontalFlip":
            for ax in p["flip"]:
                data["pos"][:, ax] = data["pos"].max() - data["pos"][:, ax]
        elif base == "ChromaticDropGPU":
            if p["drop"]:
                data["x"][:, :3] = 0
        elif base == "ChromaticPerDropGPU":
            data["x"][:, :3] *= f(p["mask"]).reshape(-1, 1)
        else:
            raise ValueError(name)
        assert data["pos"].dtype == dtype and data["x"].dtype == dtype
    return {"pos": data["pos"], "x": data["x"], "heights": data.get("heights"), "x_is_pos": data["x"] is data["pos"],
            "center": center, "scale": scale}


def fixture_params(fx, case, i):
    """Item i's recorded draws in ViewProgram.draw's layout."""
    names = [str(n) for n in fx[case + "_names"]]
    params = []
    for k in range(len(names)):
        p = {what: fx["%s_t%d_%s" % (case, k, what)][i] for what in ("scale", "t", "R", "noise", "mask") if "%s_t%d_%s" % (case, k, what) in fx.files}
        if "%s_t%d_flip" % (case, k) in fx.files:
            p["flip"] = [ax for ax in range(3) if fx["%s_t%d_flip" % (case, k)][i][ax]]
        if "%s_t%d_drop" % (case, k) in fx.files:
            p["drop"] = bool(fx["%s_t%d_drop" % (case, k)][i])
        params.append(p)
    return params
