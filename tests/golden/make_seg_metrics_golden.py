"""Regenerate tests/golden/seg_metrics_ref.npz (build container only: the reference tree does not exist on the GPU box).

    python tests/golden/make_seg_metrics_golden.py

What runs is the reference's own code, as make_ntm_golden.py runs it: ``get_seg_metrics`` and ``validate``
(examples/segmentation/train.py:802-832, 716-779) are taken out of the file with ``ast`` and executed in place on the CPU,
``Tensor.cuda`` being the identity.  ``tqdm``, ``get_pred_whole`` and the model are stubs: the model hands over the batch's
stored predictions as its "logits" and the get_pred_whole stub returns them, so what runs is the reference's counting, its
per-class loop, its numpy means and validate's jaw split and aggregation.  validate's jaw means are local variables: they
are read from its frame when it returns.  The fixture holds data only: per-scan predictions / labels, the jaw classes,
every value the reference computed with its dtype, the numpy / torch versions and the provenance.

    e0    one epoch of 10 scans (1 ... 20 000 vertices, 5 batches of 2, both jaws): a background-only scan (NaN mIoU / DSC,
          the float64 promotion), a class present and never predicted, a class predicted and never present
    e1    one epoch of 3 scans, all maxillary: the mandible means are empty means (NaN)
    gsm   get_seg_metrics alone on 3 scans with predictions -1, 17 and 255
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_ntm_golden import PROVENANCE, REF, TRAIN, on_cpu, ref_defs  # noqa: E402

C = 17
OUT = os.path.join(HERE, "seg_metrics_ref.npz")


def _scan(rng, m, kind):
    """Labels in runs along the vertex order (a mesh lists a tooth's vertices together), predictions = labels with 12 %
    replaced at random."""
    runs = max(1, m // 700)
    cuts = np.sort(rng.integers(0, m, runs - 1))
    run_labels = rng.integers(1, C, runs)
    run_labels[rng.random(runs) < 0.35] = 0
    labels = np.repeat(run_labels, np.diff(np.concatenate([[0], cuts, [m]])))
    if kind == "background":
        labels[:] = 0
    elif kind == "never_predicted":
        labels[m // 3: m // 3 + 900] = 15
    elif kind == "never_present":
        labels[labels == 16] = 1
    elif kind == "single":
        labels[:] = 5
    preds = labels.copy()
    flip = rng.random(m) < 0.12
    preds[flip] = rng.integers(0, C, int(flip.sum()))
    if kind == "never_predicted":
        preds[preds == 15] = 14
    elif kind == "never_present":
        preds[m // 2: m // 2 + 400] = 16
    elif kind == "out_of_range":
        preds[rng.random(m) < 0.05] = -1
        preds[rng.random(m) < 0.05] = 17
        preds[rng.random(m) < 0.05] = 255
    return preds.astype(np.int16), labels.astype(np.int8)


CASES = {
    "e0": dict(sizes=[1, 20000, 4097, 64, 777, 15000, 3, 12000, 2500, 9001], cls=[0, 1, 1, 0, 0, 0, 1, 1, 0, 1],
               kinds={0: "single", 4: "background", 5: "never_predicted", 7: "never_present"}, batches=[2, 2, 2, 2, 2]),
    "e1": dict(sizes=[5000, 1500, 8000], cls=[1, 1, 1], kinds={}, batches=[2, 1]),
    "gsm": dict(sizes=[3000, 1, 2048], cls=[0, 0, 0], kinds={0: "out_of_range", 2: "out_of_range"}, batches=[3]),
}


class _StoredPredictions:
    """The model: its "logits" are the batch's stored predictions (the get_pred_whole stub passes them through)."""

    def eval(self):
        return self

    def __call__(self, data):
        return data["preds"], None, None


def _batch(preds, labels, cls):
    b = len(preds)
    return {"pos": torch.zeros(b, 8, 3), "cls": torch.tensor(cls, dtype=torch.int64).reshape(b, 1),
            "x": torch.zeros(b, 8, 3), "y": torch.zeros(b, 8, dtype=torch.int64),
            "points": [torch.zeros(len(lab), 3) for lab in labels],
            "labels": [torch.from_numpy(lab.astype(np.int64)) for lab in labels],
            "center": [torch.zeros(1, 3) for _ in labels], "scale": [torch.ones(()) for _ in labels],
            "preds": [torch.from_numpy(p.astype(np.int64))[None] for p in preds]}


def _per_scan(out, tag, results):
    acc, miou, mdsc = ([], [], [])
    for a, i, d in results:
        acc += [float(x) for x in a]
        assert all(torch.is_tensor(x) and x.dtype == torch.float32 and x.dim() == 0 for x in a)
        miou += list(i)
        mdsc += list(d)
    out[tag + "_acc"] = np.array(acc, np.float32)
    out[tag + "_miou"] = np.array([float(x) for x in miou], np.float64)
    out[tag + "_miou_dtype"] = np.array([type(x).__name__ for x in miou])
    out[tag + "_mdsc"] = np.array([float(x) for x in mdsc], np.float64)
    out[tag + "_mdsc_dtype"] = np.array([type(x).__name__ for x in mdsc])


def main():
    assert os.path.isdir(REF), "run where the reference tree exists"
    rng = np.random.default_rng(20241016)
    ns = dict(torch=torch, np=np, logging=SimpleNamespace(info=lambda *a, **k: None),
              tqdm=lambda it, total=None: it, get_pred_whole=lambda logits, points, points_whole, center, scale: logits)
    ref_defs(TRAIN, ["get_seg_metrics", "validate"], ns)
    reference_gsm = ns["get_seg_metrics"]
    results = []
    ns["get_seg_metrics"] = lambda p, l: results.append(reference_gsm(p, l)) or results[-1]
    out = {}
    for tag, case in CASES.items():
        scans = [_scan(rng, m, case["kinds"].get(i, "plain")) for i, m in enumerate(case["sizes"])]
        out[tag + "_preds"] = np.concatenate([p for p, _ in scans])
        out[tag + "_labels"] = np.concatenate([lab for _, lab in scans])
        out[tag + "_sizes"] = np.array(case["sizes"], np.int64)
        out[tag + "_cls"] = np.array(case["cls"], np.int64)
        out[tag + "_batches"] = np.array(case["batches"], np.int64)
        del results[:]
        with on_cpu(torch.float32):
            if tag == "gsm":
                results.append(reference_gsm([torch.from_numpy(p.astype(np.int64))[None] for p, _ in scans],
                                             [torch.from_numpy(lab.astype(np.int64)) for _, lab in scans]))
            else:
                loader, at = [], 0
                for b in case["batches"]:
                    part = scans[at:at + b]
                    loader.append(_batch([p for p, _ in part], [lab for _, lab in part], case["cls"][at:at + b]))
                    at += b
                frame = {}
                code = ns["validate"].__code__

                def keep_locals(f, event, arg):
                    if event == "return" and f.f_code is code:
                        frame.update(f.f_locals)
                sys.setprofile(keep_locals)
                try:
                    ret = ns["validate"](_StoredPredictions(), loader, SimpleNamespace(epoch=1, epochs=2))
                finally:
                    sys.setprofile(None)
                names = [jaw + "_" + m for jaw in ("mandible", "maxillary", "whole") for m in ("macc", "miou", "mdsc")]
                for name in names:
                    out["%s_%s" % (tag, name)] = np.asarray(frame[name])
                assert all(np.asarray(r).dtype == np.asarray(frame[n]).dtype for r, n in zip(ret, names[6:]))
        _per_scan(out, tag, results)
    rows = ["%s lines %s" % kv for kv in sorted(PROVENANCE.items()) if "train.py::" in kv[0]]
    meta = ("executed from the reference checkout on the CPU (Tensor.cuda = identity; tqdm, get_pred_whole and the model "
            "stubbed: the model returns the stored predictions): %s. Per-scan values are in scan order; *_dtype is the "
            "type of each miou / mdsc value; the jaw / whole values keep their dtype." % "; ".join(rows))
    np.savez_compressed(OUT, meta=np.array(meta), numpy_version=np.array(np.__version__),
                        torch_version=np.array(torch.__version__), **out)
    print("%.1f KB  %s" % (os.path.getsize(OUT) / 1024, OUT))
    for tag in ("e0", "e1"):
        print(tag, [(k[len(tag) + 1:], out[k][()], out[k].dtype) for k in sorted(out) if k.startswith(tag + "_") and
                    out[k].ndim == 0])


if __name__ == "__main__":
    main()
