"""Regenerate tests/golden/fixmatch_views_ref.npz (build container only: the reference tree does not exist on the GPU box).

    python tests/golden/make_views_golden.py

What runs is the reference's own code, as make_ntm_golden.py runs it: the transform classes
(openpoints/transforms/point_transformer_gpu.py, PointsToTensor of point_transform_cpu.py) and the two training datasets
(openpoints/dataset/tooth_semi/tooth_dataset.py TeethSegSemiLDataset / TeethSegSemiUDataset, constructor and __getitem__)
are taken out of their files with ``ast`` and executed in place on the CPU.  The transform lists and their keyword
arguments are read from cfgs/tooth_semi/transformer_finetune_fixmatch_ntm.yaml.  Stubs: ``IO.get`` hands over the
synthetic scans, the registry decorators are dropped and the lists are composed by a plain loop;
``collections.Iterable`` (gone from this Python) is ``collections.abc.Iterable`` in the executing namespace, the classes
are not edited.  In that namespace ``torch.rand``, ``np.random.uniform``, ``np.random.shuffle`` and ``np.random.choice``
are wrapped so that every draw is recorded; the scale, rotation matrix and translation the transforms form from them are
local variables of their ``__call__``: they are read from the frame when it returns.  Items are collated with torch's
default collation and x / x_w / x_s are transposed as examples/segmentation/train.py:445, 467, 485-486 do.

The fixture holds data only.  Per case ("cfg": the yaml's kwargs, R = I; "rot": the same plus angle_s = [1, 1, 1]):

    seed                       numpy and torch are seeded with it, then the 3 labelled and the 3 unlabelled items are made
    l_* / u_*                  every key of the collated labelled / unlabelled batch
    l_raw_pos                  the labelled items' sampled pc_norm-ed points (the reference's pc_norm on the recorded indices)
    l_sel / u_sel              the recorded np.random.choice results
    l_s, u_s_s, u_R_s, u_t_s   the recorded view parameters; u_theta (3, 3), u_perm (3, 3) the angles and the shuffle
    next_np / next_torch       the next draws of both generators after the last item
    eref_<key>                 max |reference fp32 - fp64 restatement (tests/_views_ref.py) on the recorded parameters|
and once: the synthetic scans (scan_l<i> / scan_u<i>, lab_* mapped to class ids, cls_*), num_points, kwargs, versions,
provenance.
"""
import collections
import collections.abc
import json
import os
import sys
import tempfile
import types
from copy import deepcopy

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from make_ntm_golden import PROVENANCE, REF, ref_defs  # noqa: E402
import _views_ref as vr  # noqa: E402

TRANSFORMS = "openpoints/transforms/point_transformer_gpu.py"
TRANSFORMS_CPU = "openpoints/transforms/point_transform_cpu.py"
DATASET = "openpoints/dataset/tooth_semi/tooth_dataset.py"
YAML = "cfgs/tooth_semi/transformer_finetune_fixmatch_ntm.yaml"
OUT = os.path.join(HERE, "fixmatch_views_ref.npz")
NUM_POINTS = 768
SIZES_L, SIZES_U = (1500, 1201, 1800), (1650, 500, 2000)      # 500 < NUM_POINTS: np.random.choice(replace=True)
CASES = (("cfg", 20240, None), ("rot", 20241, [1, 1, 1]))
FDI = [0] + [10 * q + t for q in (1, 2, 3, 4) for t in range(1, 9)]


class _Proxy:
    """A module look-alike: attribute reads fall through to the real module unless overridden."""

    def __init__(self, real, **over):
        self.__dict__["_real"], self.__dict__["_over"] = real, over

    def __getattr__(self, name):
        over = self.__dict__["_over"]
        return over[name] if name in over else getattr(self.__dict__["_real"], name)


class Recorder:
    def __init__(self):
        self.rand, self.uniform, self.perm, self.choice, self.frames = [], [], [], [], []

    def torch_rand(self, *a, **k):
        out = torch.rand(*a, **k)
        self.rand.append(out.clone().numpy())
        return out

    def np_uniform(self, *a, **k):
        out = np.random.uniform(*a, **k)
        self.uniform.append(out)
        return out

    def np_shuffle(self, seq):
        before = list(seq)
        np.random.shuffle(seq)
        self.perm.append([next(i for i, b in enumerate(before) if b is a) for a in seq])

    def np_choice(self, *a, **k):
        out = np.random.choice(*a, **k)
        self.choice.append(np.array(out))
        return out

    def trace(self, frame, event, arg):
        """sys.settrace hook: the locals of every transform __call__ of the reference file, at its return."""
        if event == "call" and frame.f_code.co_name == "__call__" and frame.f_code.co_filename.endswith(TRANSFORMS):
            def local(fr, ev, _):
                if ev == "return":
                    keep = {k: (v.clone().numpy() if torch.is_tensor(v) else v) for k, v in fr.f_locals.items()
                            if k in ("scale", "rot_mat", "translation")}
                    self.frames.append((type(fr.f_locals["self"]).__name__, keep))
                return local
            return local
        return None


def namespace(rec):
    from scipy.linalg import expm, norm
    coll = types.ModuleType("collections")
    coll.__dict__.update(collections.__dict__)
    coll.Iterable = collections.abc.Iterable                  # removed in Python 3.10; the classes still spell it this way
    scans = {}
    ns = {"torch": _Proxy(torch, rand=rec.torch_rand),
          "np": _Proxy(np, random=_Proxy(np.random, uniform=rec.np_uniform, shuffle=rec.np_shuffle, choice=rec.np_choice)),
          "collections": coll, "expm": expm, "norm": norm, "deepcopy": deepcopy, "os": os, "json": json,
          "data": torch.utils.data, "IO": types.SimpleNamespace(get=lambda path: scans[path]), "_scans": scans}
    ref_defs(TRANSFORMS, ["PointCloudCenterAndNormalize", "PointCloudScaling", "PointCloudScaling_s", "PointCloudRotation_s",
                          "PointCloudTranslation_s"], ns)
    ref_defs(TRANSFORMS_CPU, ["PointsToTensor"], ns)
    ref_defs(DATASET, ["TeethSegSemiLDataset", "TeethSegSemiUDataset"], ns)
    return ns


def compose(ns, names, kwargs):
    """transforms_factory's Compose over the registry, as a loop: every class is built with the whole kwargs dict."""
    ops = [ns[n](**kwargs) for n in names]

    def run(data):
        for op in ops:
            data = op(data)
        return data
    return run


def synthetic_scan(rng, n):
    """A jaw-like arch far from the origin (millimetres), teeth as runs of FDI labels along the vertex order."""
    u = np.sort(rng.random(n)) * np.pi
    pts = np.stack([28 * np.cos(u), 9 * rng.random(n), 22 * np.sin(u)], axis=1) + rng.normal(0, 1.5, (n, 3))
    pts = (pts + np.array([14.0, -37.0, 61.0])).astype(np.float32)
    cuts = np.sort(rng.integers(0, n, 13))
    run = rng.choice(FDI, 14)
    labels = np.repeat(run, np.diff(np.concatenate([[0], cuts, [n]])))
    return pts, labels


def make_data_root(tmp, ns, scans_l, scans_u):
    """data.json + the two split lists the constructors read; the 'files' are keys of the IO stub."""
    table = {"scans": {}, "gt": {}}
    for split, scans in (("l", scans_l), ("u", scans_u)):
        names = []
        for i, (pts, labels, jaw) in enumerate(scans):
            name = "%s%03d_%s.obj" % (split, i, "lower" if jaw == 0 else "upper")
            names.append(name)
            table["scans"][name], table["gt"][name] = name + "#points", name + "#gt"
            ns["_scans"][name + "#points"] = pts
            ns["_scans"][name + "#gt"] = {"labels": [int(v) for v in labels]}
        with open(os.path.join(tmp, "semi_%s_train_0.2.txt" % split), "w") as fh:
            fh.write("\n".join(names) + "\n")
    with open(os.path.join(tmp, "data.json"), "w") as fh:
        json.dump(table, fh)


def run_case(tag, seed, angle_s, cfg, scans_l, scans_u, out):
    rec = Recorder()
    ns = namespace(rec)
    kwargs = dict(cfg["kwargs"])
    if angle_s is not None:
        kwargs["angle_s"] = angle_s
    with tempfile.TemporaryDirectory() as tmp:
        make_data_root(tmp, ns, scans_l, scans_u)
        ds_l = ns["TeethSegSemiLDataset"](data_root=tmp, num_points=NUM_POINTS, split="train",
                                          transform=compose(ns, cfg["train"], kwargs))
        ds_u = ns["TeethSegSemiUDataset"](data_root=tmp, num_points=NUM_POINTS, split="train",
                                          transform_w=compose(ns, cfg["train_w"], kwargs),
                                          transform_s=compose(ns, cfg["train_s"], kwargs))
    np.random.seed(seed)
    torch.manual_seed(seed)
    sys.settrace(rec.trace)
    try:
        items_l = [ds_l[i] for i in range(len(scans_l))]
        items_u = [ds_u[i] for i in range(len(scans_u))]
    finally:
        sys.settrace(None)
    nxt_np, nxt_torch = np.random.random_sample(4), torch.rand(4).numpy()
    batch_l = torch.utils.data.default_collate(items_l)
    batch_u = torch.utils.data.default_collate(items_u)
    batch_l["x"] = batch_l["x"].transpose(1, 2).contiguous()                       # train.py:445 / 485
    for k in ("x_w", "x_s"):
        batch_u[k] = batch_u[k].transpose(1, 2).contiguous()                       # train.py:467, 486
    bl, bu = len(scans_l), len(scans_u)
    assert len(rec.choice) == bl + bu and len(rec.uniform) == 3 * bu and len(rec.perm) == bu
    frames = {}
    for name, keep in rec.frames:
        frames.setdefault(name, []).append(keep)
    p = tag + "_"
    out[p + "seed"] = np.int64(seed)
    out[p + "l_sel"], out[p + "u_sel"] = np.stack(rec.choice[:bl]), np.stack(rec.choice[bl:])
    out[p + "l_s"] = np.stack([f["scale"] for f in frames["PointCloudScaling"]])
    out[p + "u_s_s"] = np.stack([f["scale"] for f in frames["PointCloudScaling_s"]])
    out[p + "u_R_s"] = np.stack([f["rot_mat"] for f in frames["PointCloudRotation_s"]])
    out[p + "u_t_s"] = np.stack([f["translation"] for f in frames["PointCloudTranslation_s"]])
    out[p + "u_theta"] = np.array(rec.uniform, dtype=np.float64).reshape(bu, 3)
    out[p + "u_perm"] = np.array(rec.perm, dtype=np.int64)
    out[p + "rand_raw"] = np.stack(rec.rand)
    out[p + "next_np"], out[p + "next_torch"] = nxt_np, nxt_torch
    # the labelled items' untransformed sample: the reference's own pc_norm on the recorded indices
    out[p + "l_raw_pos"] = np.stack([ds_l.pc_norm(scans_l[i][0])[0][out[p + "l_sel"][i]].astype(np.float32) for i in range(bl)])
    for side, batch in (("l_", batch_l), ("u_", batch_u)):
        for k, v in batch.items():
            out[p + side + k] = v.numpy()
    # e_ref: the reference's fp32 outputs against the fp64 restatement on the recorded parameters
    g = int(kwargs["gravity_dim"])
    eye, zero, one = np.eye(3, dtype=np.float32), np.zeros(3, np.float32), np.ones(3, np.float32)
    err = collections.defaultdict(float)

    def measure(suffix, side, raw, i, s, R, t, strong):
        ref = vr.view_f64(raw, s, R, t, g, rotate=strong, translate=strong)
        for key, want in (("pos", ref["pos"]), ("x", ref["x"].T), ("heights", ref["heights"])):
            got = out[p + side + key + suffix][i].astype(np.float64)
            err[side + key + suffix] = max(err[side + key + suffix], float(np.abs(got - want).max()))
    for i in range(bl):
        measure("", "l_", out[p + "l_raw_pos"][i], i, out[p + "l_s"][i], eye, zero, False)
    for i in range(bu):
        raw = out[p + "u_raw_pos"][i]
        measure("_w", "u_", raw, i, one, eye, zero, False)
        measure("_s", "u_", raw, i, out[p + "u_s_s"][i], out[p + "u_R_s"][i], out[p + "u_t_s"][i], True)
    for k, v in err.items():
        out[p + "eref_" + k] = np.float64(v)
    return kwargs


def main():
    import yaml
    with open(os.path.join(REF, YAML)) as fh:
        cfg = yaml.safe_load(fh)["datatransforms"]
    from geot_amd.openpoints.dataset.fixmatch_batch import TOOTH_VIEW_KWARGS
    for k, v in TOOTH_VIEW_KWARGS.items():
        assert cfg["kwargs"][k] == v, "TOOTH_VIEW_KWARGS[%r] differs from the yaml" % k
    assert "angle_s" not in cfg["kwargs"]
    rng = np.random.default_rng(7)
    scans_l = [synthetic_scan(rng, n) + (i % 2,) for i, n in enumerate(SIZES_L)]
    scans_u = [synthetic_scan(rng, n) + ((i + 1) % 2,) for i, n in enumerate(SIZES_U)]
    out = {"num_points": np.int64(NUM_POINTS), "num_classes": np.int64(17), "cases": np.array([c[0] for c in CASES])}
    label2id = None
    for tag, seed, angle_s in CASES:
        kwargs = run_case(tag, seed, angle_s, cfg, scans_l, scans_u, out)
        out[tag + "_kwargs"] = np.array(json.dumps(kwargs, sort_keys=True))
    ns = namespace(Recorder())
    with tempfile.TemporaryDirectory() as tmp:
        make_data_root(tmp, ns, scans_l, scans_u)
        label2id = ns["TeethSegSemiUDataset"](data_root=tmp, num_points=NUM_POINTS, split="train").label2id
    for split, scans in (("l", scans_l), ("u", scans_u)):
        for i, (pts, labels, jaw) in enumerate(scans):
            out["scan_%s%d" % (split, i)] = pts
            out["lab_%s%d" % (split, i)] = np.array([label2id[int(v)] for v in labels], dtype=np.int32)
        out["cls_" + split] = np.array([s[2] for s in scans], dtype=np.int64)
    import scipy
    out["meta"] = np.array(json.dumps({
        "generator": "tests/golden/make_views_golden.py", "numpy": np.__version__, "torch": torch.__version__,
        "scipy": scipy.__version__, "python": sys.version.split()[0], "provenance": dict(PROVENANCE),
        "lists": {k: cfg[k] for k in ("train", "train_w", "train_s")},
        "note": "x, x_w, x_s are stored transposed (B, 3, m) as train.py does after collation; labels are class ids "
                "(label2id applied); e_ref = max |reference fp32 - tests/_views_ref.py fp64| per key"}, sort_keys=True))
    np.savez_compressed(OUT, **out)
    print("%8.1f KB  %s" % (os.path.getsize(OUT) / 1024, os.path.basename(OUT)))
    for k in sorted(out):
        if "eref_" in k:
            print("  %-24s %.3e" % (k, float(out[k])))


if __name__ == "__main__":
    assert os.path.isdir(REF), "run in the build container"
    main()
