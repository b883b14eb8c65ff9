"""Regenerate tests/golden/view_program_ref.npz (build container only: the reference tree does not exist on the GPU box).

    python tests/golden/make_view_program_golden.py

What runs is the reference's own code, as make_views_golden.py runs it: the transform classes
(openpoints/transforms/point_transformer_gpu.py, PointsToTensor of point_transform_cpu.py) and the labelled training dataset
(openpoints/dataset/tooth_semi/tooth_dataset.py TeethSegSemiLDataset, constructor and __getitem__) are taken out of their
files with ``ast`` and executed in place on the CPU; ``IO.get`` hands over synthetic scans, the registry decorators are
dropped, the lists are composed by a plain loop in which every class receives the whole kwargs dict.  In the executing
namespace ``torch.rand`` / ``torch.randn_like``, ``np.random.uniform`` / ``shuffle`` / ``choice`` and ``random.random`` are
wrapped so that every draw is seen; what the transforms form from them (scale, translation, rot_mat, noise, colors_drop) are
locals of their ``__call__`` and are read from the frame when it returns.  Items are collated with torch's default collation
and x is transposed as examples/segmentation/train.py:445 does.

Four transform lists (CASES): a = the `train` list and kwargs of cfgs/tooth_semi/default.yaml, b / c / d = lists that
exercise every other supported transform.  The fixture holds data only.  Per case <c>:

    <c>_names, <c>_kwargs      the list and the kwargs (json)
    <c>_seed                   numpy, torch and python `random` are seeded with it, then the items are made in order
    <c>_b_<key>                every key of the collated batch (x transposed to (B, 3, m))
    <c>_raw_pos, <c>_sel       the items' sampled pc_norm-ed points (the reference's pc_norm on the recorded indices), the
                               recorded np.random.choice results
    <c>_t<k>_<what>            the draws of transform k of the list, stacked over the items: scale, t, noise, R, mask as the
                               transform formed them; flip (B, 3) 0/1 per axis; drop (B,) 0/1
    <c>_x_is_pos, <c>_has_heights   whether data['x'] was still data['pos'] after the list / the batch has heights
    <c>_next_np / _next_torch / _next_py   the next draws of the three generators after the last item
    <c>_eref_<key>             max |reference fp32 - fp64 restatement (tests/_view_program_ref.py) on the recorded draws|
and once: the synthetic scans (scan<i>, lab<i> mapped to class ids, cls), num_points, versions, provenance.
"""
import collections
import collections.abc
import json
import os
import random
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
from make_views_golden import _Proxy, make_data_root, synthetic_scan  # noqa: E402
import _view_program_ref as vpr  # noqa: E402

TRANSFORMS = "openpoints/transforms/point_transformer_gpu.py"
TRANSFORMS_CPU = "openpoints/transforms/point_transform_cpu.py"
DATASET = "openpoints/dataset/tooth_semi/tooth_dataset.py"
YAML = "cfgs/tooth_semi/default.yaml"
OUT = os.path.join(HERE, "view_program_ref.npz")
NUM_POINTS = 256
SIZES = (700, 200, 450)                  # 200 < NUM_POINTS: np.random.choice(replace=True)
CLASSES = ["PointCloudToTensor", "PointCloudCenterAndNormalize", "PointCloudXYZAlign", "RandomHorizontalFlip", "PointCloudScaling",
           "PointCloudScaling_s", "PointCloudTranslation", "PointCloudTranslation_s", "PointCloudScaleAndTranslate",
           "PointCloudScaleAndTranslate_s", "PointCloudJitter", "PointCloudJitter_s", "PointCloudScaleAndJitter",
           "PointCloudRotation", "PointCloudRotation_s", "ChromaticDropGPU", "ChromaticPerDropGPU"]
# case -> (seed, list or None = the yaml's `train`, kwargs on top of the yaml's)
CASES = {
    "a": (20250, None, {}),
    "b": (20251, ["PointsToTensor", "PointCloudScaleAndTranslate_s", "PointCloudCenterAndNormalize", "PointCloudJitter_s",
                  "PointCloudRotation_s", "PointCloudTranslation_s"], {"angle_s": [1, 1, 1]}),
    "c": (20252, ["PointsToTensor", "PointCloudJitter", "PointCloudScaling", "RandomHorizontalFlip", "PointCloudXYZAlign",
                  "ChromaticPerDropGPU"], {"mirror": [0.5, 0.5, 0.5], "upright_axis": "y"}),
    "d": (20253, ["PointsToTensor", "PointCloudScaleAndJitter", "PointCloudCenterAndNormalize", "PointCloudTranslation"],
          {"centering": False, "mirror": [1, 0, 1]}),
}
KEEP = {"scale": "scale", "translation": "t", "rot_mat": "R", "noise": "noise", "colors_drop": "mask"}


class Recorder:
    def __init__(self):
        self.rand, self.choice, self.py, self.frames = [], [], [], []

    def torch_rand(self, *a, **k):
        out = torch.rand(*a, **k)
        self.rand.append(out.clone().numpy())
        return out

    def np_choice(self, *a, **k):
        out = np.random.choice(*a, **k)
        self.choice.append(np.array(out))
        return out

    def py_random(self):
        out = random.random()
        self.py.append(out)
        return out

    def trace(self, frame, event, arg):
        """sys.settrace hook: the locals of every transform __call__ of the reference file, at its return."""
        if event == "call" and frame.f_code.co_name == "__call__" and frame.f_code.co_filename.endswith(TRANSFORMS):
            start = (len(self.rand), len(self.py))

            def local(fr, ev, _):
                if ev == "return":
                    keep = {KEEP[k]: v.clone().numpy() for k, v in fr.f_locals.items() if k in KEEP and torch.is_tensor(v)}
                    keep["_rand"], keep["_py"] = self.rand[start[0]:], self.py[start[1]:]
                    keep["_x_is_pos"] = fr.f_locals["data"]["x"] is fr.f_locals["data"]["pos"]
                    self.frames.append((type(fr.f_locals["self"]).__name__, fr.f_locals["self"], keep))
                return local
            return local
        return None


def namespace(rec):
    from scipy.linalg import expm, norm
    coll = types.ModuleType("collections")
    coll.__dict__.update(collections.__dict__)
    coll.Iterable = collections.abc.Iterable                  # removed in Python 3.10; the classes still spell it this way
    scans = {}
    ns = {"torch": _Proxy(torch, rand=rec.torch_rand), "np": _Proxy(np, random=_Proxy(np.random, choice=rec.np_choice)),
          "random": _Proxy(random, random=rec.py_random), "collections": coll, "expm": expm, "norm": norm,
          "deepcopy": deepcopy, "os": os, "json": json, "data": torch.utils.data,
          "IO": types.SimpleNamespace(get=lambda path: scans[path]), "_scans": scans}
    ref_defs(TRANSFORMS, CLASSES, ns)
    ref_defs(TRANSFORMS_CPU, ["PointsToTensor"], ns)
    ref_defs(DATASET, ["TeethSegSemiLDataset"], ns)
    return ns


def compose(ns, names, kwargs):
    """transforms_factory's Compose over the registry, as a loop: every class is built with the whole kwargs dict."""
    ops = [ns[n](**kwargs) for n in names]

    def run(data):
        for op in ops:
            data = op(data)
        return data
    return run


def item_params(names, frames):
    """One item's frames (the list's transforms but PointsToTensor, in order) -> ViewProgram.draw's layout."""
    params, frames = [], list(frames)
    for name in names:
        if name == "PointsToTensor":
            params.append({})
            continue
        cls, obj, keep = frames.pop(0)
        assert cls == name, (cls, name)
        p = {k: v for k, v in keep.items() if not k.startswith("_")}
        if name == "RandomHorizontalFlip":      # the class's own tests on the recorded python draws
            draws, flips = list(keep["_py"]), []
            if draws.pop(0) < obj.aug_prob:
                for ax in obj.horz_axes:
                    if draws.pop(0) < 0.5:
                        flips.append(ax)
            assert not draws
            p = {"flip": flips}
        elif name == "ChromaticDropGPU":
            assert len(keep["_rand"]) == 1 and keep["_rand"][0].shape == (1,)
            p = {"drop": bool(keep["_rand"][0][0] < obj.color_drop)}
        elif name == "ChromaticPerDropGPU":
            p = {"mask": p["mask"].reshape(-1)}
        elif name in ("PointCloudJitter", "PointCloudJitter_s"):
            p = {"noise": p["noise"]}
        elif name == "PointCloudScaleAndJitter":
            p = {"scale": p["scale"], "noise": p["noise"]}
        elif name in ("PointCloudCenterAndNormalize", "PointCloudXYZAlign"):
            p = {}
        if "scale" in p:
            p["scale"] = np.broadcast_to(p["scale"], (3,)).copy()
        p["_x_is_pos"] = keep["_x_is_pos"]
        params.append(p)
    assert not frames
    return params


def run_case(tag, seed, names, kwargs, scans, out):
    rec = Recorder()
    ns = namespace(rec)
    with tempfile.TemporaryDirectory() as tmp:
        make_data_root(tmp, ns, scans, scans)
        ds = ns["TeethSegSemiLDataset"](data_root=tmp, num_points=NUM_POINTS, split="train", transform=compose(ns, names, kwargs))
    np.random.seed(seed)
    torch.manual_seed(seed)
    random.seed(seed)
    items, params = [], []
    for i in range(len(scans)):
        first = len(rec.frames)
        sys.settrace(rec.trace)
        try:
            items.append(ds[i])
        finally:
            sys.settrace(None)
        params.append(item_params(names, rec.frames[first:]))
    nxt = np.random.random_sample(4), torch.rand(4).numpy(), np.array([random.random() for _ in range(4)])
    batch = torch.utils.data.default_collate(items)
    batch["x"] = batch["x"].transpose(1, 2).contiguous()                           # train.py:445
    b, p = len(scans), tag + "_"
    assert len(rec.choice) == b
    out[p + "names"], out[p + "kwargs"] = np.array(names), np.array(json.dumps(kwargs, sort_keys=True))
    out[p + "seed"], out[p + "sel"] = np.int64(seed), np.stack(rec.choice)
    out[p + "next_np"], out[p + "next_torch"], out[p + "next_py"] = nxt
    out[p + "raw_pos"] = np.stack([ds.pc_norm(scans[i][0])[0][out[p + "sel"][i]].astype(np.float32) for i in range(b)])
    for k, v in batch.items():
        out[p + "b_" + k] = v.numpy()
    x_is_pos = {params[i][-1]["_x_is_pos"] for i in range(b)}
    assert len(x_is_pos) == 1
    out[p + "x_is_pos"], out[p + "has_heights"] = np.int64(x_is_pos.pop()), np.int64("heights" in batch)
    for k, name in enumerate(names):
        for what in ("scale", "t", "R", "noise", "mask"):
            if what in params[0][k]:
                out["%st%d_%s" % (p, k, what)] = np.stack([params[i][k][what] for i in range(b)]).astype(np.float32)
        if "flip" in params[0][k]:
            out["%st%d_flip" % (p, k)] = np.array([[int(ax in params[i][k]["flip"]) for ax in range(3)] for i in range(b)], np.int64)
        if "drop" in params[0][k]:
            out["%st%d_drop" % (p, k)] = np.array([int(params[i][k]["drop"]) for i in range(b)], np.int64)
    # e_ref: the reference's fp32 outputs against the fp64 restatement on the recorded draws
    err = collections.defaultdict(float)
    for i in range(b):
        ref = vpr.run(out[p + "raw_pos"][i], names, kwargs, params[i], np.float64)
        assert ref["x_is_pos"] == bool(out[p + "x_is_pos"]) and (ref["heights"] is not None) == bool(out[p + "has_heights"])
        for key, want in (("pos", ref["pos"]), ("x", ref["x"].T), ("heights", ref["heights"])):
            if want is not None:
                err[key] = max(err[key], float(np.abs(out[p + "b_" + key][i].astype(np.float64) - want).max()))
    for k, v in err.items():
        out[p + "eref_" + k] = np.float64(v)
    return params


def check_branches(tag, names, params, out):
    """Both branches of every data-dependent decision must occur: change the SEED if one is missing, not this check."""
    if tag == "a":
        k = names.index("ChromaticDropGPU")
        fired = [p[k]["drop"] for p in params]
        assert any(fired) and not all(fired), "case a: ChromaticDropGPU must fire for one item and not for another: %s" % fired
        for i, f in enumerate(fired):
            assert (not out["a_b_x"][i].any()) == f
    if tag == "c":
        k = names.index("RandomHorizontalFlip")
        flips = out["c_t%d_flip" % k][:, [0, 2]]
        assert flips.any() and not flips.all(), "case c: one flipped and one unflipped horizontal axis: %s" % flips
        signs = np.sign(out["c_t%d_scale" % names.index("PointCloudScaling")])
        assert (signs < 0).any() and (signs > 0).any(), "case c: one mirrored and one unmirrored component: %s" % signs
        kept = out["c_t%d_mask" % names.index("ChromaticPerDropGPU")].sum(axis=1)
        assert ((kept >= 1) & (kept <= NUM_POINTS - 1)).all(), "case c: between 1 and m - 1 dropped points per item: %s" % kept
        assert np.array_equal(out["c_b_x"].transpose(0, 2, 1), out["c_b_pos"]) and not out["c_has_heights"]
        dropped = out["c_t%d_mask" % names.index("ChromaticPerDropGPU")] == 0
        assert not out["c_b_pos"][dropped].any()        # the dropped points are zero in pos too


def main():
    import yaml
    with open(os.path.join(REF, YAML)) as fh:
        cfg = yaml.safe_load(fh)["datatransforms"]
    from geot_amd.openpoints.dataset.supervised_batch import DEFAULT_TRAIN, DEFAULT_TRAIN_KWARGS
    assert cfg["train"] == DEFAULT_TRAIN and cfg["kwargs"] == DEFAULT_TRAIN_KWARGS, "DEFAULT_TRAIN(_KWARGS) differ from the yaml"
    rng = np.random.default_rng(11)
    scans = [synthetic_scan(rng, n) + (i % 2,) for i, n in enumerate(SIZES)]
    out = {"num_points": np.int64(NUM_POINTS), "num_classes": np.int64(17), "cases": np.array(sorted(CASES))}
    for tag in sorted(CASES):
        seed, names, extra = CASES[tag]
        names, kwargs = (cfg["train"] if names is None else names), dict(cfg["kwargs"], **extra)
        params = run_case(tag, seed, names, kwargs, scans, out)
        check_branches(tag, names, params, out)
    ns = namespace(Recorder())
    with tempfile.TemporaryDirectory() as tmp:
        make_data_root(tmp, ns, scans, scans)
        label2id = ns["TeethSegSemiLDataset"](data_root=tmp, num_points=NUM_POINTS, split="train").label2id
    for i, (pts, labels, jaw) in enumerate(scans):
        out["scan%d" % i] = pts
        out["lab%d" % i] = np.array([label2id[int(v)] for v in labels], dtype=np.int32)
    out["cls"] = np.array([s[2] for s in scans], dtype=np.int64)
    import scipy
    out["meta"] = np.array(json.dumps({
        "generator": "tests/golden/make_view_program_golden.py", "numpy": np.__version__, "torch": torch.__version__,
        "scipy": scipy.__version__, "python": sys.version.split()[0], "provenance": dict(PROVENANCE),
        "note": "x is stored transposed (B, 3, m) as train.py does after collation; labels are class ids (label2id applied); "
                "e_ref = max |reference fp32 - tests/_view_program_ref.py fp64| per key"}, sort_keys=True))
    np.savez_compressed(OUT, **out)
    print("%8.1f KB  %s" % (os.path.getsize(OUT) / 1024, os.path.basename(OUT)))
    for k in sorted(out):
        if "eref_" in k:
            print("  %-24s %.3e" % (k, float(out[k])))


if __name__ == "__main__":
    assert os.path.isdir(REF), "run in the build container"
    main()
