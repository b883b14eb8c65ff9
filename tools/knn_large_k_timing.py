"""Long-list kNN timing (GPU only): the selection kernel behind knn_sorted / knn_cuda.KNN / knn_point for k > 64,
pointops.knn's certified path and the literal heap of knnquery_cuda, against the reference's formulation on the same
inputs (chunked torch.cdist + topk, as openpoints/models/layers/knn.py does it) and, at k = 128 / 256, against the
one-lane insertion kernel (GEOT_NN_IMPL=basic).

    python tools/knn_large_k_timing.py [--out FILE] [--iters 10]

Times are device events around each call, after a warm-up call, median over --iters calls (the cdist + topk
formulation: median over 3).  Every sorted result is checked bit for bit against the numpy restatement
(oracle/np_ref.py) on a sample of queries."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from geot_amd import _lib  # noqa: E402
from geot_amd.synth import make_batch  # noqa: E402
from geot_amd.knn_cuda import knn_sorted  # noqa: E402
from geot_amd.ext import pointops_cuda  # noqa: E402
from geot_amd.pointops.functions import pointops  # noqa: E402
from oracle import np_ref  # noqa: E402

DEV = torch.device("cuda:0")
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def cdist_topk(q, r, k, chunk=2048):
    outs = []
    for s in range(0, q.shape[1], chunk):
        outs.append(torch.cdist(q[:, s:s + chunk], r).topk(k=k, dim=-1, largest=False, sorted=True).indices)
    return torch.cat(outs, 1)


def cloud(b, n, start):
    return torch.from_numpy(make_batch(b, n, start_index=start)[0]).to(DEV)


def basic(fn):
    os.environ["GEOT_NN_IMPL"] = "basic"
    try:
        return fn()
    finally:
        del os.environ["GEOT_NN_IMPL"]


def check_sample(q, r, k, d2, idx, n=64):
    """ids and squared distances of n sampled queries of the first cloud equal the numpy restatement's, bit for bit
    (cdist + topk cannot serve here: its matmul-form distances round differently and reorder near-ties)"""
    pick = np.arange(0, q.shape[1], max(1, q.shape[1] // n))[:n]
    wi, wd = np_ref.knn_sorted(q[:1, pick].cpu().numpy(), r[:1].cpu().numpy(), k)
    return bool(np.array_equal(idx[:1, pick].cpu().numpy(), wi) and np.array_equal(d2[:1, pick].cpu().numpy(), wd)), len(pick)


def sorted_shape(b, nq, nr, k, iters):
    r = cloud(b, nr, 1)
    q = r if nq == nr else r[:, :nq].contiguous()
    t_new = timed(lambda: knn_sorted(q, r, k), iters)
    good, n_ok = check_sample(q, r, k, *knn_sorted(q, r, k))
    try:
        t_ref = "%.2f ms" % timed(lambda: cdist_topk(q, r, k), 3)
    except RuntimeError as e:                   # (out of memory, ...)
        t_ref = "failed: %s" % str(e).splitlines()[0][:80]
    old = ""
    if k in (128, 256):
        try:
            old = ", one-lane kernel (GEOT_NN_IMPL=basic) %.2f ms" % basic(lambda: timed(lambda: knn_sorted(q, r, k), iters))
        except RuntimeError as e:
            old = ", one-lane kernel: %s" % str(e).splitlines()[0][:100]
    say("sorted  b=%d nq=%5d nr=%5d k=%4d : new %8.2f ms | cdist+topk %s%s | bit-exact vs numpy on %d sampled queries: %s"
        % (b, nq, nr, k, t_new, t_ref, old, n_ok, good))


def certified_share(b, n, k):
    x = cloud(b, n, 3)
    flat = x.reshape(-1, 3).contiguous()
    off = torch.arange(1, b + 1, device=DEV, dtype=torch.int32) * n
    nbytes = int(_lib.load().geot_knnquery_heap_ws_bytes(b, n, n, k))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    idx = torch.empty((b * n, k), dtype=torch.int32, device=DEV)
    d2 = torch.empty((b * n, k), dtype=torch.float32, device=DEV)
    err = _lib.load().geot_knnquery_heap_ws(b, n, n, k, flat.data_ptr(), flat.data_ptr(), off.data_ptr(), off.data_ptr(),
                                            idx.data_ptr(), d2.data_ptr(), ws.data_ptr(), nbytes,
                                            torch.cuda.current_stream().cuda_stream)
    _lib.check(err, "geot_knnquery_heap_ws")
    torch.cuda.synchronize()
    uncertified = int(ws[4 * b * n:4 * b * n + 4].view(torch.int32).item())
    return 1.0 - uncertified / float(b * n)


def pointops_shape(b, n, k, iters):
    x = cloud(b, n, 3)
    flat = x.reshape(-1, 3).contiguous()
    off = torch.arange(1, b + 1, device=DEV, dtype=torch.int32) * n
    idx = torch.empty((b * n, k), dtype=torch.int32, device=DEV)
    d2 = torch.empty((b * n, k), dtype=torch.float32, device=DEV)
    t_new = timed(lambda: pointops.knn(x, x, k), iters)
    t_heap = timed(lambda: pointops_cuda.knnquery_cuda(b * n, k, flat, flat, off, off, idx, d2), max(3, iters // 3))
    t_ref = timed(lambda: cdist_topk(x, x, k), 3)
    say("pointops.knn b=%d n=%d k=%4d : new %8.2f ms | literal heap (knnquery_cuda) %8.2f ms | cdist+topk %8.2f ms | "
        "certified share %.4f" % (b, n, k, t_new, t_heap, t_ref, certified_share(b, n, k)))


def ragged_heap(sizes, nsample, iters):
    clouds = [make_batch(1, s, start_index=5 + i)[0][0] for i, s in enumerate(sizes)]
    xyz = torch.from_numpy(np.concatenate(clouds)).to(DEV)
    q = torch.from_numpy(np.concatenate([c[::4] for c in clouds])).to(DEV)
    off = torch.from_numpy(np.cumsum(sizes).astype(np.int32)).to(DEV)
    noff = torch.from_numpy(np.cumsum([(s + 3) // 4 for s in sizes]).astype(np.int32)).to(DEV)
    m = q.shape[0]
    idx = torch.empty((m, nsample), dtype=torch.int32, device=DEV)
    d2 = torch.empty((m, nsample), dtype=torch.float32, device=DEV)
    t = timed(lambda: pointops_cuda.knnquery_cuda(m, nsample, xyz, q, off, noff, idx, d2), iters)
    ref = []
    for i, s in enumerate(sizes):   # the reference's formulation per segment
        a = int(off[i - 1]) if i else 0
        qa = int(noff[i - 1]) if i else 0
        ref.append((xyz[None, a:a + s], q[None, qa:int(noff[i])]))
    t_ref = timed(lambda: [cdist_topk(qq, rr, nsample) for rr, qq in ref], 3)
    say("knnquery_cuda ragged segments=%s queries=%d nsample=%d : literal heap %8.2f ms | cdist+topk per segment %8.2f ms"
        % (sizes, m, nsample, t, t_ref))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_large_k_timing: no GPU")
    say("# %s, %s, KMAX_HEAP=%d KMAX_SORTED=%d" % (torch.cuda.get_device_name(0), _lib.LIB_PATH.split("/")[-1],
                                                     _lib.KNN_KMAX_HEAP, _lib.KNN_KMAX_SORTED))
    for k in (128, 256, 512, 1000, 4096):
        sorted_shape(8, 24000, 24000, k, a.iters)
    sorted_shape(8, 8192, 24000, 1000, a.iters)
    for k in (128, 1000):
        pointops_shape(2, 24000, k, a.iters)
    ragged_heap([24000, 16000, 8000], 1000, a.iters)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
