"""Run by tests/test_knn_large_k_gpu.py in a child process with GEOT_DISTANCE=fma: the long-list kNN paths of the
contracted-distance library (literal heap, pointops.knn's certified path, sorted selection) against the oracle twin
built with the same GEOT_DISTANCE_MODE, bit for bit."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geot_amd import _lib  # noqa: E402
from geot_amd.synth import make_batch  # noqa: E402
from geot_amd.ext import pointops_cuda  # noqa: E402
from geot_amd.pointops.functions import pointops  # noqa: E402
from geot_amd.knn_cuda import knn_sorted  # noqa: E402
from oracle import capi  # noqa: E402

mode = os.environ["GEOT_DISTANCE"]
assert _lib.DISTANCE == mode and capi.DISTANCE == mode and _lib.load().geot_distance_mode() == {"fma": 1, "fma_xy": 2}[mode]
dev = torch.device("cuda:0")
B, N, K = 2, 4000, 300
xyz = make_batch(B, N, start_index=33, dup_frac=0.02)[0]
x = torch.from_numpy(xyz).to(dev)
q = xyz[:, ::10].copy()
M = q.shape[1]
off = (np.arange(1, B + 1) * N).astype(np.int32)
noff = (np.arange(1, B + 1) * M).astype(np.int32)

# literal heap, ragged-capable entry point
idx = torch.zeros((B * M, K), dtype=torch.int32, device=dev)
d2 = torch.zeros((B * M, K), dtype=torch.float32, device=dev)
pointops_cuda.knnquery_cuda(B * M, K, x.reshape(-1, 3).contiguous(), torch.from_numpy(q.reshape(-1, 3)).to(dev),
                            torch.from_numpy(off).to(dev), torch.from_numpy(noff).to(dev), idx, d2)
wi, wd = capi.knnquery_heap(K, xyz.reshape(-1, 3), q.reshape(-1, 3), off, noff)
assert np.array_equal(idx.cpu().numpy(), wi) and np.array_equal(d2.cpu().numpy(), wd)
# pointops.knn: selection + certification, the heap for the rest
pi, pd = pointops.knn(torch.from_numpy(q).to(dev), x, K)
assert np.array_equal(pi.cpu().numpy().reshape(-1, K) + np.repeat(np.arange(B) * N, M)[:, None], wi)
# sorted selection
d2, ki = knn_sorted(torch.from_numpy(q).to(dev), x, K)
wi, wd = capi.knn_sorted(q, xyz, K)
assert np.array_equal(ki.cpu().numpy(), wi) and np.array_equal(d2.cpu().numpy(), wd)
print("long-list contracted parity ok: %s" % mode)
