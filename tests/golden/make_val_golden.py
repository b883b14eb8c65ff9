"""Regenerate tests/golden/val_batches_ref.npz (build container only: the reference tree does not exist on the GPU box).

    python tests/golden/make_val_golden.py

What runs is the reference's own code, as make_views_golden.py runs it: TeethSegSemiLDataset (constructor and __getitem__
of openpoints/dataset/tooth_semi/tooth_dataset.py) with split='val', the `val` transform list of
cfgs/tooth_semi/transformer_finetune_fixmatch_ntm.yaml (PointsToTensor, PointCloudCenterAndNormalize) and collate_fn_val
(openpoints/dataset/build.py) are taken out of their files with ``ast`` and executed in place on the CPU over small
synthetic scans, one of them with fewer vertices than num_points.  Stubs and recorded draws as in make_views_golden.py.
Items are taken in the sequential sampler's order, collated in batches of BATCH scans, and x is transposed as
examples/segmentation/train.py:738 does.

The fixture holds data only:

    seed                  numpy and torch are seeded with it, then the items are made in order
    b<k>_pos / x / y / cls / center / scale     the collated batch k (center / scale: the lists, stacked)
    b<k>_ids, b<k>_sel    the scans of batch k and the recorded np.random.choice results
    next_np / next_torch  the next draws of both generators after the last item; n_torch_rand: torch.rand calls seen (0)
    scan<i> / lab<i> (class ids) / cls      the synthetic scans
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from make_ntm_golden import PROVENANCE, REF, ref_defs  # noqa: E402
from make_views_golden import YAML, Recorder, compose, namespace, synthetic_scan  # noqa: E402

OUT = os.path.join(HERE, "val_batches_ref.npz")
NUM_POINTS = 768
SIZES = (1500, 500, 2000, 1201)           # 500 < NUM_POINTS: np.random.choice(replace=True)
JAWS = (0, 1, 1, 0)
BATCH = 2
SEED = 20242


def make_data_root(tmp, ns, scans):
    """data.json + testing.txt, the list every split but 'train' reads; the 'files' are keys of the IO stub."""
    table, names = {"scans": {}, "gt": {}}, []
    for i, (pts, labels, jaw) in enumerate(scans):
        name = "v%03d_%s.obj" % (i, "lower" if jaw == 0 else "upper")
        names.append(name)
        table["scans"][name], table["gt"][name] = name + "#points", name + "#gt"
        ns["_scans"][name + "#points"] = pts
        ns["_scans"][name + "#gt"] = {"labels": [int(v) for v in labels]}
    with open(os.path.join(tmp, "testing.txt"), "w") as fh:
        fh.write("\n".join(names) + "\n")
    with open(os.path.join(tmp, "data.json"), "w") as fh:
        json.dump(table, fh)


def main():
    import yaml
    with open(os.path.join(REF, YAML)) as fh:
        cfg = yaml.safe_load(fh)["datatransforms"]
    assert cfg["val"] == cfg["train_w"], "the val list is no longer the weak view's list"
    rng = np.random.default_rng(11)
    scans = [synthetic_scan(rng, n) + (jaw,) for n, jaw in zip(SIZES, JAWS)]
    rec = Recorder()
    ns = namespace(rec)
    ref_defs("openpoints/dataset/build.py", ["collate_fn_val"], ns)
    with tempfile.TemporaryDirectory() as tmp:
        make_data_root(tmp, ns, scans)
        ds = ns["TeethSegSemiLDataset"](data_root=tmp, num_points=NUM_POINTS, split="val",
                                        transform=compose(ns, cfg["val"], dict(cfg["kwargs"])))
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    items = [ds[i] for i in range(len(scans))]
    nxt_np, nxt_torch = np.random.random_sample(4), torch.rand(4).numpy()
    assert len(rec.choice) == len(scans) and not rec.uniform and not rec.perm
    out = {"num_points": np.int64(NUM_POINTS), "num_classes": np.int64(17), "seed": np.int64(SEED), "batch_size": np.int64(BATCH),
           "next_np": nxt_np, "next_torch": nxt_torch, "n_torch_rand": np.int64(len(rec.rand)),
           "cls": np.array(JAWS, dtype=np.int64)}
    for k, at in enumerate(range(0, len(items), BATCH)):
        data = ns["collate_fn_val"](items[at:at + BATCH])
        data["x"] = data["x"].transpose(1, 2).contiguous()                               # train.py:738
        p = "b%d_" % k
        for key in ("pos", "x", "y"):
            out[p + key] = data[key].numpy()
        out[p + "cls"] = np.asarray(data["cls"])
        out[p + "center"] = torch.stack(data["center"]).numpy()
        out[p + "scale"] = torch.stack(data["scale"]).numpy()
        out[p + "ids"] = np.arange(at, min(at + BATCH, len(items)), dtype=np.int64)
        out[p + "sel"] = np.stack(rec.choice[at:at + BATCH])
        for j, i in enumerate(out[p + "ids"]):                                          # the lists carry the whole scans
            assert np.array_equal(data["points"][j].numpy(), scans[i][0])
            assert np.array_equal(data["labels"][j].numpy(), [ds.label2id[int(v)] for v in scans[i][1]])
    out["batches"] = np.int64(k + 1)
    for i, (pts, labels, _) in enumerate(scans):
        out["scan%d" % i] = pts
        out["lab%d" % i] = np.array([ds.label2id[int(v)] for v in labels], dtype=np.int32)
    out["meta"] = np.array(json.dumps({
        "generator": "tests/golden/make_val_golden.py", "numpy": np.__version__, "torch": torch.__version__,
        "python": sys.version.split()[0], "provenance": dict(PROVENANCE), "list": cfg["val"],
        "note": "x is stored transposed (B, 3, m) as train.py:738 does after collation; labels are class ids (label2id applied)"},
        sort_keys=True))
    np.savez_compressed(OUT, **out)
    print("%8.1f KB  %s" % (os.path.getsize(OUT) / 1024, os.path.basename(OUT)))
    for key in sorted(out):
        print("  %-14s %s %s" % (key, out[key].dtype, out[key].shape))


if __name__ == "__main__":
    assert os.path.isdir(REF), "run in the build container"
    main()
