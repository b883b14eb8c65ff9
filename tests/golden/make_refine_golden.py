"""Regenerate tests/golden/part_seg_refinement_ref.npz: the reference's part_seg_refinement executed in place (BUILD container
only: /root/reference does not exist on the GPU box).

    python tests/golden/make_refine_golden.py

What runs is the reference's own code: batched_bincount and part_seg_refinement (examples/segmentation/train.py),
torch_grouping_operation (openpoints/models/layers/group.py) taken out of their files with ``ast`` as make_ntm_golden.py does,
knn_point loaded by file path.  No reference source text is written anywhere: the fixture holds seeded inputs and the labels
the reference returned.

The reference reads ``pred.cpu().data.numpy()`` once and goes on writing ``pred``.  For the CUDA tensor it is written for that
is a snapshot; for a plain CPU tensor it is a view that follows every write, and the labels differ.  The rule is the CUDA
one, so ``pred`` is handed over as a Tensor subclass whose ``cpu()`` returns a clone (``meta`` says so).

Inputs: four unit-ball-normalised clouds of N points with region labels and islands: classes of 1, 3, 7, 9 (= n - 1: refined)
and 10 (= n: kept) members, a class the jaw does not allow that holds most of a scan (its inner vertices vote all-zero -> 0),
two small classes next to each other with the later one first in the scan, a scan of two classes, a scan of one class.
Seeds are tried until, for EVERY query, the fp64 gap between the (n + 1)-th and (n + 2)-th squared distance is at least 32
fp32 ulp of the largest squared vertex norm -- there torch.cdist + topk and the (d2, index) order pick the same n + 1 vertices,
so no query is left out of any comparison.
"""
import os
import sys
from collections import Counter

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _scan_refine_ref as rref  # noqa: E402
from make_ntm_golden import PROVENANCE, REF, _load_by_path, ref_defs  # noqa: E402

N_POINTS, N_REFINE, C = 400, 10, 17
CLS2PARTS = [[0, 1, 2, 3, 4, 5, 6, 7, 8], [0, 9, 10, 11, 12, 13, 14, 15, 16]]
CLS = [0, 1, 0, 1]
MIN_GAP_ULP = 32.0


class SnapshotTensor(torch.Tensor):
    """cpu() is a copy, as it is for a CUDA tensor."""

    def cpu(self, *args, **kwargs):
        return torch.Tensor.cpu(self.as_subclass(torch.Tensor)).clone()


def _cloud(rng, m):
    x = rng.normal(size=(m, 3)) * np.array([1.0, 0.7, 0.4])
    x -= x.mean(0)
    return (x / np.sqrt((x ** 2).sum(1)).max()).astype(np.float32)


def _island(rng, pts, pred, label, members, at=None):
    """`members` vertices around a random vertex (or around vertex `at`) get `label`."""
    at = int(rng.integers(len(pts))) if at is None else at
    near = np.argsort(((pts - pts[at]) ** 2).sum(1), kind="stable")[:members]
    pred[near] = label
    return near


def make_inputs(seed):
    rng = np.random.default_rng(seed)
    pos = np.stack([_cloud(rng, N_POINTS) for _ in CLS])
    pred = np.zeros((len(CLS), N_POINTS), np.int64)
    # scan 0 (mandible: 0..8 allowed): three regions along x, islands of 1, 3, 7, 9 and 10 members, one disallowed island of 12
    order = np.argsort(pos[0][:, 0])
    pred[0, order[:150]], pred[0, order[150:280]], pred[0, order[280:]] = 1, 2, 3
    for label, members in ((4, 1), (5, 3), (6, 7), (7, 9), (8, 10), (12, 12)):
        _island(rng, pos[0], pred[0], label, members)
    # scan 1 (maxillary: 0, 9..16 allowed): class 3 is not allowed and holds most of the scan; two small classes side by side,
    # 11 around vertex 5 and 10 around its neighbour, with vertex 0 forced into class 10: 10 comes first although 11 sits lower
    pred[1, :] = 3
    order = np.argsort(pos[1][:, 1])
    pred[1, order[:90]] = 9
    a = _island(rng, pos[1], pred[1], 11, 5, at=5)
    far = [v for v in np.argsort(((pos[1] - pos[1][5]) ** 2).sum(1), kind="stable") if v not in set(a)][:4]
    pred[1, far] = 10
    pos[1][0] = pos[1][far[0]] + np.float32(1e-3)
    pred[1, 0] = 10
    # scan 2: two classes, the smaller one below n; scan 3: one class
    pred[2, :] = 2
    _island(rng, pos[2], pred[2], 5, 6)
    pred[3, :] = 13
    return pos, pred


def queries_and_gap(pos, pred):
    gaps, nq = [], 0
    for s in range(len(CLS)):
        count = Counter(pred[s].tolist())
        if len(count) < 2:
            continue
        q = np.flatnonzero([count[int(l)] < N_REFINE or int(l) not in CLS2PARTS[CLS[s]] for l in pred[s]])
        nq += q.size
        gaps.append(rref.knn_gap(pos[s], q, N_REFINE))
    return nq, min(gaps)


if __name__ == "__main__":
    assert os.path.isdir(REF), "run in the build container"
    knn_mod = _load_by_path(os.path.join(REF, "openpoints/models/layers/knn.py"), "geot_ref_knn")
    PROVENANCE["openpoints/models/layers/knn.py::knn_point"] = "imported by file path"
    ns = dict(torch=torch, np=np, Counter=Counter, knn_point=knn_mod.knn_point)
    ref_defs("examples/segmentation/train.py", ["batched_bincount", "part_seg_refinement"], ns)
    ref_defs("openpoints/models/layers/group.py", ["torch_grouping_operation"], ns)
    for seed in range(1000):
        pos, pred = make_inputs(seed)
        nq, gap = queries_and_gap(pos, pred)
        if gap >= MIN_GAP_ULP:
            break
    else:
        raise AssertionError("no seed with a gap of %g ulp" % MIN_GAP_ULP)
    assert gap >= MIN_GAP_ULP
    run = lambda t: ns["part_seg_refinement"](t, torch.from_numpy(pos), CLS, CLS2PARTS, n=N_REFINE)    # noqa: E731
    out = run(torch.from_numpy(pred.copy()).as_subclass(SnapshotTensor)).as_subclass(torch.Tensor).numpy().copy()
    aliased = run(torch.from_numpy(pred.copy())).numpy().copy()
    want, stats = rref.refine_scans(list(pred), list(pos), C, N_REFINE, [CLS2PARTS[j] for j in CLS])
    assert np.array_equal(np.stack(want), out), "the restatement differs from the reference at %d vertices" % int((np.stack(want) != out).sum())
    assert int(stats[:, 1].sum()) == nq
    alias_want = [rref.refine_scan(p, x, C, N_REFINE, CLS2PARTS[j], alias=True)[0] for p, x, j in zip(pred, pos, CLS)]
    assert np.array_equal(np.stack(alias_want), aliased)
    assert not np.array_equal(out, aliased), "the inputs do not tell the snapshot rule from the aliasing form"
    rows = "; ".join("%s lines %s" % kv for kv in sorted(PROVENANCE.items()) if "refinement" in kv[0] or "bincount" in kv[0]
                     or "knn_point" in kv[0] or "grouping" in kv[0])
    meta = ("executed from /root/reference (torch %s, CPU): %s. pred was a Tensor subclass whose cpu() returns a clone (the "
            "snapshot rule of a CUDA tensor); `aliased` is the same call on a plain CPU tensor. seed %d, n %d, %d queries, "
            "%d labels changed, smallest fp64 gap between the (n+1)-th and (n+2)-th squared distance %.1f fp32 ulp of the "
            "largest squared norm (required %g); no query excluded."
            % (torch.__version__, rows, seed, N_REFINE, nq, int((out != pred).sum()), gap, MIN_GAP_ULP))
    path = os.path.join(HERE, "part_seg_refinement_ref.npz")
    np.savez_compressed(path, meta=np.array(meta), pos=pos, pred=pred.astype(np.int16), out=out.astype(np.int16),
                        aliased=aliased.astype(np.int16), cls=np.array(CLS, np.int64), n=np.int64(N_REFINE),
                        cls2parts=np.array(CLS2PARTS, np.int64), stats=stats, seed=np.int64(seed), min_gap_ulp=np.float64(gap))
    print(meta)
    print("%8.1f KB  %s" % (os.path.getsize(path) / 1024, os.path.basename(path)))
