"""kNN-based pseudo-label refinement -- mirror of utils/pseudo_mask.py (get_neigbor_tensors :5-35,
pseudo_label_refine :38-53, pseudo_label_refine_margin :55-90, pseudo_label_refine_margin_v1 :92-170,
neigh_acc_count :174-196; the configured run keeps ``pseudo_refine: False``, yaml:75).

The neighbours come from ``pointops.knn`` (heap-order semantics kept, grid-accelerated) and the per-neighbour
``index_select`` loop is one grouping launch: (B,C,N) gathered at (B,N,n) -> (B,C,N,n).  Same signatures, same
returned tensors (sic: the reference's spellings are kept).  Everything runs under ``no_grad`` as there; the class
counters of ``neigh_acc_count`` stay on the device until ``acc_array`` is read (the reference adds 2 x num_class device
scalars to a numpy array per update = 34 host syncs).

``pseudo_refine_mask`` is the three refinements as ONE launch behind the neighbour search (csrc/pseudo_refine.hip
geot_pseudo_refine): the gather, the top-k, the blend passes and the class maximum / margin per point in registers, no
(B, C, N, n) tensor; ``neighbours`` is the table it reads.  The functions above stay what they were: the composite the fused
entry point is tested against.
"""
import numpy as np
import torch

from .. import _lib
from ..ext._common import call, need, ptr
from ..pointops.functions import pointops
from ..pointnet2 import pointnet2_utils as pt_utils

E_JOINT = [0.9698153347167245, 0.9595924029774019, 0.9596092881209647, 0.9617471101196512, 0.9662687092798028,
           0.9684095068416779, 0.9766432433032493, 0.9754884408811396, 0.9629032258064516, 0.9596091749248413,
           0.9584221215955251, 0.9619788870996601, 0.9666700999073025, 0.968204136476084, 0.9760611218051148,
           0.9746949382049295, 0.966996699669967]     # pseudo_mask.py:56-61


def get_neigbor_tensors(X, n, pos):
    """X (B,C,N), pos (B,N,3) -> (list of n tensors (B,C,N): X at each point's ii-th nearest OTHER point,
    top_dist (B,N,n))."""
    B, C, N = X.shape
    top_dist_index, top_dist = pointops.knn(pos, pos, n + 1)             # (B,N,n+1); slot 0 = the point itself
    top_dist = top_dist[:, :, 1:]
    idx = top_dist_index[:, :, 1:].to(torch.int32).contiguous()          # local ids within each cloud
    grouped = pt_utils.grouping_operation(X.contiguous().float(), idx)   # (B,C,N,n) in one launch
    return [grouped[..., ii].contiguous() for ii in range(n)], top_dist


def _blend(pred_t, pos, neigborhood_size, n_neigbors):
    neighbors, _ = get_neigbor_tensors(pred_t, n=neigborhood_size, pos=pos)
    k_neighbors, _ = torch.topk(torch.stack(neighbors), k=n_neigbors, dim=0)          # (n_neigbors,B,C,N)
    beta = float(np.exp(-0.5))
    for neighbor in k_neighbors:
        pred_t = pred_t + beta * neighbor - (pred_t * neighbor) * beta
    return pred_t


@torch.no_grad()
def pseudo_label_refine(pred_t, th, pos, neigborhood_size=4, n_neigbors=1):
    pred_t = _blend(pred_t, pos, neigborhood_size, n_neigbors)
    logits_u_aug, _ = torch.max(pred_t.detach(), dim=1)
    return logits_u_aug.ge(th).bool()


@torch.no_grad()
def pseudo_label_refine_margin(pred_t, th, pos, neigborhood_size=4, n_neigbors=1):
    pred_t = _blend(pred_t, pos, neigborhood_size, n_neigbors)
    _topk, _ = torch.topk(pred_t.detach(), 2, dim=1)
    _margin = _topk[:, 0, :] - _topk[:, 1, :]
    return _margin.ge(th).bool(), _margin


@torch.no_grad()
def pseudo_label_refine_margin_v1(pred_t, th, drop_percent, pos, neigborhood_size=4, n_neigbors=1):
    B, C, N = pred_t.shape
    E = torch.tensor(E_JOINT[:C], device=pred_t.device, dtype=pred_t.dtype).view(1, C, 1)
    neighbors, _ = get_neigbor_tensors(pred_t, n=neigborhood_size, pos=pos)
    k_neighbors, _ = torch.topk(torch.stack(neighbors), k=n_neigbors, dim=0)
    for neighbor in k_neighbors:
        upper_bound = E * pred_t / neighbor
        pred_t = pred_t + neighbor - (pred_t * upper_bound)
    _topk, _ = torch.topk(pred_t.detach(), 2, dim=1)
    _margin = _topk[:, 0, :] - _topk[:, 1, :]
    return _margin.ge(th).bool(), _margin, th


def neighbours(pos, n):
    """pos (B, N, 3) -> (B, N, n) int32: every point's n nearest OTHER points, local ids -- slots 1 .. n of
    pointops.knn(pos, pos, n + 1), slot 0 dropped as get_neigbor_tensors drops it.  Depends on the coordinates alone."""
    need(torch.is_tensor(pos) and pos.dim() == 3 and pos.shape[2] == 3, "neighbours: pos must be (B, N, 3)")
    need(isinstance(n, int) and not isinstance(n, bool) and 1 <= n <= _lib.PSEUDO_REFINE_MAX_N,
         "neighbours: n must be an int in 1..%d, got %r" % (_lib.PSEUDO_REFINE_MAX_N, n))
    need(pos.shape[1] >= n + 1, "neighbours: %d points have no %d nearest other points" % (pos.shape[1], n))
    idx, _ = pointops.knn(pos, pos, n + 1)
    return idx[:, :, 1:].to(torch.int32).contiguous()


_CONSTANTS = {}


def _beta():
    """The reference's torch.exp(torch.tensor(-1/2)) (pseudo_mask.py:47), computed once on the host in fp32."""
    if "beta" not in _CONSTANTS:
        _CONSTANTS["beta"] = float(torch.exp(torch.tensor(-1 / 2)))
    return _CONSTANTS["beta"]


def _e_joint(device, c):
    key = (str(device), c)
    if key not in _CONSTANTS:
        _CONSTANTS[key] = torch.tensor(E_JOINT[:c], dtype=torch.float32).to(device)
    return _CONSTANTS[key]


@torch.no_grad()
def pseudo_refine_mask(pred_t, th, pos, neigborhood_size=4, n_neigbors=1, mode="max", nbr=None, return_value=False):
    """pseudo_label_refine (mode "max"), pseudo_label_refine_margin ("margin") or pseudo_label_refine_margin_v1 ("margin_v1")
    in one launch: pred_t (B, C, N) fp32 probabilities, pos (B, N, 3) -> keep (B, N) uint8, the hard mask the fused criteria
    take; with return_value=True (keep, value (B, N) fp32): the refined confidence, or the top-1 minus top-2 margin.
    nbr: neighbours(pos, neigborhood_size) computed earlier (pos is then not read); otherwise it is computed here."""
    need(mode in _lib.PSEUDO_MODES, "pseudo_refine_mask: mode must be one of %s, got %r" % (sorted(_lib.PSEUDO_MODES), mode))
    need(torch.is_tensor(pred_t) and pred_t.dim() == 3 and pred_t.dtype == torch.float32,
         "pseudo_refine_mask: pred_t must be a (B, C, N) fp32 tensor")
    b, c, npts = pred_t.shape
    n, k = neigborhood_size, n_neigbors
    need(all(isinstance(v, int) and not isinstance(v, bool) for v in (n, k)) and 1 <= k <= n <= _lib.PSEUDO_REFINE_MAX_N,
         "pseudo_refine_mask: 1 <= n_neigbors <= neigborhood_size <= %d, got %r / %r" % (_lib.PSEUDO_REFINE_MAX_N, k, n))
    need(npts >= n + 1, "pseudo_refine_mask: %d points have no %d nearest other points" % (npts, n))
    need(1 <= c <= (len(E_JOINT) if mode == "margin_v1" else 32) and (c >= 2 or mode == "max"),
         "pseudo_refine_mask: %d classes (1..32; 2..%d for margin_v1, at least 2 for margin)" % (c, len(E_JOINT)))
    need(pred_t.is_cuda, "pseudo_refine_mask: CPU not supported (pred_t must live on the GPU)")
    if nbr is None:
        need(torch.is_tensor(pos) and tuple(pos.shape) == (b, npts, 3), "pseudo_refine_mask: pos must be (B, N, 3)")
        nbr = neighbours(pos, n)
    need(torch.is_tensor(nbr) and nbr.dtype == torch.int32 and tuple(nbr.shape) == (b, npts, n) and nbr.device == pred_t.device,
         "pseudo_refine_mask: nbr must be the (B, N, %d) int32 table of neighbours(pos, %d) on %s" % (n, n, pred_t.device))
    dev = pred_t.device
    prob, nbr = pred_t.detach().contiguous(), nbr.contiguous()
    keep = torch.empty((b, npts), dtype=torch.uint8, device=dev)
    value = torch.empty((b, npts), dtype=torch.float32, device=dev) if return_value else None
    e = _e_joint(dev, c) if mode == "margin_v1" else None
    call("geot_pseudo_refine", dev, b, c, npts, n, k, _lib.PSEUDO_MODES[mode], float(th), _beta(), ptr(prob), ptr(nbr), ptr(e),
         ptr(keep), ptr(value))
    return (keep, value) if return_value else keep


class neigh_acc_count:
    """Per-class agreement between a point's predicted label and its nearest neighbour's (first cloud of the batch
    only, as the reference: pseudo_mask.py:184-189)."""

    def __init__(self, num_class=17):
        self.num_class = num_class
        self._acc = None

    @torch.no_grad()
    def update(self, pred, pos, neigborhood_size=4, n_neigbors=1):
        top_dist_index, _ = pointops.knn(pos, pos, 2)
        nn_idx = top_dist_index[0, :, 1].long()
        p = pred[0]
        agree = (p == p[nn_idx])
        counts = torch.bincount(p, minlength=self.num_class)[:self.num_class]
        hits = torch.bincount(p[agree], minlength=self.num_class)[:self.num_class]
        upd = torch.stack([counts, hits], 1).to(torch.float64)
        self._acc = upd if self._acc is None else self._acc + upd

    @property
    def acc_array(self):
        return np.zeros((self.num_class, 2)) if self._acc is None else self._acc.cpu().numpy()
