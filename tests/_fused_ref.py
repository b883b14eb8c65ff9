"""Shared by the fused row-op tests (geot_amd/fused_norm.py over csrc/bnrelu.hip and csrc/layernorm.hip): the error bound
of an fp32 sum from the depth of its summation tree, the first-maximum rule of torch.max, storage at an offset, a
backward that hands its gradient over at an offset, and a recorder of the kernels a call launched."""
import numpy as np
import torch

U32 = 2.0 ** -24                 # unit roundoff of fp32 (round to nearest)


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): |fl(sum) - sum| <= gamma_k * sum|terms| for a summation tree of depth k
    (every term passes through at most k roundings), whatever the order inside the tree"""
    return k * U32 / (1.0 - k * U32)


def first_argmax(x):
    """(..., n) -> int64 (...): torch.max's slot, spelled out -- the first NaN if the row has one, else the first maximum
    (-0.0 and +0.0 tie: the earlier slot wins; an all -inf row gives 0)"""
    a = x.detach().cpu().numpy()
    return torch.from_numpy(np.argmax(a, axis=-1).astype(np.int64))   # numpy: NaN is the largest, ties go to the first


def at_offset(t, k):
    """a contiguous copy of t whose first element sits k elements past the start of fresh storage (k = 1, 2, 3: 4, 8 and 12
    bytes off the 16-byte boundary)"""
    buf = torch.empty(k + t.numel(), dtype=t.dtype, device=t.device)
    v = buf[k:].view(t.shape)
    v.copy_(t)
    return v


def backward_at_offset(outs, ups, k):
    """sum(out * up) backward for every (out, up), with the outputs' gradients handed over as contiguous slices of one
    buffer, the first at a k-element offset: what autograd does when the outputs meet again in a torch.cat"""
    pad = outs[0].new_zeros(k)
    y = torch.cat([pad] + [o.reshape(-1) for o in outs])
    w = torch.cat([pad] + [u.reshape(-1).to(y.dtype) for u in ups])
    (y * w).sum().backward()


class Launches:
    """records the C-ABI entry points fused_norm launched (monkeypatched over fused_norm.call)"""

    def __init__(self, monkeypatch):
        from geot_amd import fused_norm
        self.names = []
        real = fused_norm.call

        def rec(name, dev, *args):
            self.names.append(name)
            return real(name, dev, *args)
        monkeypatch.setattr(fused_norm, "call", rec)

    def take(self):
        names, self.names = self.names, []
        return names
