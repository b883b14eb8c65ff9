"""Regenerate tests/golden/pseudo_label_refine_ref.npz: the reference's pseudo-label refinements executed in place (BUILD
container only: /root/reference does not exist on the GPU box).

    python tests/golden/make_pseudo_refine_golden.py

What runs is the reference's own code: get_neigbor_tensors, pseudo_label_refine, pseudo_label_refine_margin and
pseudo_label_refine_margin_v1 taken out of utils/pseudo_mask.py with ``ast`` as make_ntm_golden.py does, on CPU tensors:
``Tensor.cuda`` is a no-op for the duration, ``pointops.knn`` is stood in by a brute-force search in (fp64 squared distance,
index) order that returns the point itself in slot 0 (tests/_pseudo_refine_ref.py neighbours_fp64), and ``torch.exp`` is
watched so that the bits of the ``beta`` the reference computed are kept.  No reference source text is written anywhere: the
fixture holds seeded inputs, the masks and margins the reference returned, and a provenance string.

Inputs: B = 2 clouds of N = 300 points, C = 17; the probabilities are the soft-max of logits with a few confident regions
(around random centres) and noisy borders (the logit scale follows the distance to the region's border).  th = 0.9 for the
confidence, 0.5 for the margins.  Every mode runs at (n, k) = (4, 1), the configured sizes, and at (6, 3).

Seeds are tried until, for EVERY point and case: all points are distinct; the fp64 gap between the (n + 1)-th and (n + 2)-th
squared distance is at least 32 fp32 ulp of the largest squared norm (any fp32 search then picks the same neighbours); the
value is at least 1e-4 away from th -- so no point is left out of any comparison.  (pseudo_label_refine returns its mask
only: its value is the restatement's, whose mask is asserted equal to the reference's.)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _pseudo_refine_ref as pref  # noqa: E402
from make_ntm_golden import PROVENANCE, REF, ref_defs  # noqa: E402

B, N_POINTS, C = 2, 300, 17
CASES = [(mode, n, k) for n, k in ((4, 1), (6, 3)) for mode in pref.MODES]
TH = {"max": 0.9, "margin": 0.5, "margin_v1": 0.5}
MIN_GAP_ULP, MIN_TH_DIST = 32.0, 1e-4


def make_inputs(seed):
    rng = np.random.default_rng(seed)
    pos = (rng.normal(size=(B, N_POINTS, 3)) * np.array([1.0, 0.7, 0.4])).astype(np.float32)
    logits = np.empty((B, C, N_POINTS), np.float32)
    for b in range(B):
        centres = pos[b][rng.choice(N_POINTS, 6, replace=False)].astype(np.float64)
        labels = rng.choice(C, 6, replace=False)
        d = np.sqrt(((pos[b][:, None, :].astype(np.float64) - centres[None]) ** 2).sum(-1))
        near = np.sort(d, axis=1)
        inside = near[:, 1] - near[:, 0]                         # 0 at a border between two regions
        scale = 1.0 + 14.0 * np.clip(inside / 0.5, 0.0, 1.0)
        z = rng.normal(size=(N_POINTS, C)) * 1.5
        z[np.arange(N_POINTS), labels[d.argmin(1)]] += scale
        logits[b] = z.T.astype(np.float32)
    prob = torch.softmax(torch.from_numpy(logits), dim=1).numpy()
    return pos, prob


class _Pointops:
    """pointops.knn(pos, pos, k) on CPU tensors -> (ids (B, N, k) int64 with the point itself first, distances)."""

    @staticmethod
    def knn(x, src, k):
        assert x is src or torch.equal(x, src)
        ids, _ = pref.neighbours_fp64(x.numpy(), k - 1)
        own = np.broadcast_to(np.arange(x.shape[1])[None, :, None], ids.shape[:2] + (1,))
        ids = torch.from_numpy(np.concatenate([own, ids], 2).astype(np.int64))
        dist = torch.gather(torch.cdist(x.double(), x.double()), 2, ids).float()
        return ids, dist


def run_reference(ns, pos, prob):
    """Every case through the reference's functions -> ({case: (mask, margin or None)}, the betas torch.exp returned)."""
    betas, real_exp, real_cuda = [], torch.exp, torch.Tensor.cuda

    def watched_exp(t, *a, **kw):
        out = real_exp(t, *a, **kw)
        if out.dim() == 0:
            betas.append(out.clone())
        return out
    torch.exp, torch.Tensor.cuda = watched_exp, lambda self, *a, **kw: self
    try:
        out = {}
        pred, p = torch.from_numpy(prob), torch.from_numpy(pos)
        for mode, n, k in CASES:
            if mode == "max":
                res = (ns["pseudo_label_refine"](pred.clone(), TH[mode], p, neigborhood_size=n, n_neigbors=k), None)
            elif mode == "margin":
                res = ns["pseudo_label_refine_margin"](pred.clone(), TH[mode], p, neigborhood_size=n, n_neigbors=k)
            else:
                res = ns["pseudo_label_refine_margin_v1"](pred.clone(), TH[mode], 0, p, neigborhood_size=n, n_neigbors=k)[:2]
            out[(mode, n, k)] = res
    finally:
        torch.exp, torch.Tensor.cuda = real_exp, real_cuda
    return out, betas


def beta_bits():
    return int(torch.exp(torch.tensor(-1 / 2)).view(torch.int32))


if __name__ == "__main__":
    assert os.path.isdir(REF), "run in the build container"
    from geot_amd.utils.pseudo_mask import E_JOINT
    ns = dict(torch=torch, np=np, pointops=_Pointops)
    ref_defs("utils/pseudo_mask.py", ["get_neigbor_tensors", "pseudo_label_refine", "pseudo_label_refine_margin",
                                      "pseudo_label_refine_margin_v1"], ns)
    beta = np.array(beta_bits(), np.uint32).view(np.float32)
    for seed in range(2000):
        pos, prob = make_inputs(seed)
        if len(np.unique(pos.reshape(-1, 3), axis=0)) != B * N_POINTS:
            continue
        nbrs, gaps = {}, {}
        for n in sorted({n for _, n, _ in CASES}):
            nbrs[n], g = pref.neighbours_fp64(pos, n)
            gaps[n] = float(g.min())
        if min(gaps.values()) < MIN_GAP_ULP:
            continue
        mine = {(m, n, k): pref.refine(prob, nbrs[n], k, m, TH[m], beta, E_JOINT) for m, n, k in CASES}
        dist = {case: float(np.abs(v.astype(np.float64) - TH[case[0]]).min()) for case, (_, v) in mine.items()}
        if min(dist.values()) >= MIN_TH_DIST:
            break
    else:
        raise AssertionError("no seed meets the conditions")
    ref, betas = run_reference(ns, pos, prob)
    assert betas and all(int(t.view(torch.int32)) == beta_bits() for t in betas), "the reference computed another beta"
    arrays = {}
    plain = torch.from_numpy(prob).max(1)[0]
    for case in CASES:
        mode, n, k = case
        mask, margin = ref[case]
        keep, value = mine[case]
        mask = mask.numpy().astype(np.uint8)
        assert mask.shape == (B, N_POINTS) and np.array_equal(mask, keep), "%s: the restatement's mask differs at %d points" % (
            case, int((mask != keep).sum()))
        assert set(np.unique(mask)) == {0, 1}, "%s: a trivial mask" % (case,)
        assert (mask != plain.ge(TH[mode]).numpy()).any(), "%s: the refinement changes nothing" % (case,)
        tag = "%s_n%d_k%d" % case
        arrays["mask_" + tag] = mask
        if margin is not None:
            margin = margin.numpy()
            assert margin.dtype == np.float32 and np.array_equal(margin.view(np.uint32), value.view(np.uint32)), \
                "%s: the restatement's margin differs" % (case,)
            arrays["margin_" + tag] = margin
    rows = "; ".join("%s lines %s" % kv for kv in sorted(PROVENANCE.items()) if "pseudo_mask" in kv[0])
    meta = ("executed from /root/reference (torch %s, CPU; Tensor.cuda a no-op, pointops.knn a brute-force fp64-ordered search "
            "with the point itself in slot 0): %s. seed %d; all %d points distinct; smallest fp64 gap between the (n+1)-th and "
            "(n+2)-th squared distance, in fp32 ulp of the largest squared norm (required %g): %s; smallest |value - th| "
            "(required %g): %s; kept points: %s; beta bits 0x%08x; th %s; no point excluded."
            % (torch.__version__, rows, seed, B * N_POINTS, MIN_GAP_ULP,
               ", ".join("n=%d %.1f" % kv for kv in sorted(gaps.items())), MIN_TH_DIST,
               ", ".join("%s/%d/%d %.2e" % (c + (dist[c],)) for c in CASES),
               ", ".join("%s/%d/%d %d" % (c + (int(mine[c][0].sum()),)) for c in CASES), beta_bits(), TH))
    path = os.path.join(HERE, "pseudo_label_refine_ref.npz")
    np.savez_compressed(path, meta=np.array(meta), pos=pos, prob=prob, seed=np.int64(seed), beta_bits=np.uint32(beta_bits()),
                        cases=np.array(["%s_n%d_k%d" % c for c in CASES]), th=np.array([TH[c[0]] for c in CASES], np.float64),
                        min_gap_ulp=np.array([gaps[n] for n in sorted(gaps)]), th_dist=np.array([dist[c] for c in CASES]),
                        **{"nbr_n%d" % n: v.astype(np.int16) for n, v in nbrs.items()}, **arrays)
    print(meta)
    print("%8.1f KB  %s" % (os.path.getsize(path) / 1024, os.path.basename(path)))
