"""Long neighbour lists: the heap-ordered kNN up to GEOT_KNN_KMAX_HEAP and the sorted kNN up to GEOT_KNN_KMAX_SORTED,
bit for bit (ids and squared distances) against the CPU oracle / its numpy restatement, through every public entry
point that reaches them: knnquery_cuda, pointops.knn, knn_sorted, knn_cuda.KNN and the 3-D knn_point."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from geot_amd.synth import make_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def _ragged(sizes, start):
    """Segments of the given sizes (5 % duplicated points), every 3rd point of each a query."""
    clouds = [make_batch(1, n, start_index=start + i, dup_frac=0.05)[0][0] for i, n in enumerate(sizes)]
    qs = [c[::3] for c in clouds]
    off = np.cumsum(sizes).astype(np.int32)
    noff = np.cumsum([q.shape[0] for q in qs]).astype(np.int32)
    return np.concatenate(clouds), np.concatenate(qs), off, noff


def _heap(pops, xyz, q, off, noff, nsample):
    idx = torch.full((q.shape[0], nsample), -7, dtype=torch.int32, device=DEV)
    d2 = torch.full((q.shape[0], nsample), -1.0, device=DEV)
    pops.knnquery_cuda(q.shape[0], nsample, xyz, q, off, noff, idx, d2)
    return idx, d2


@pytest.fixture(scope="module")
def pops():
    from geot_amd import _lib
    from geot_amd.ext import pointops_cuda
    _lib.load()
    return pointops_cuda


# ---- 1. the literal heap ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsample", [100, 200, 256, 257, 512, 1000, 1024])
def test_heap_matches_oracle(pops, oracle, nsample):
    # the last segment holds fewer points than nsample: its lists end in (1e10, start) entries
    xyz, q, off, noff = _ragged([2500, 1400, nsample // 2 + 1], start=40 + nsample)
    idx, d2 = _heap(pops, dev(xyz), dev(q), dev(off), dev(noff), nsample)
    wi, wd = oracle.knnquery_heap(nsample, xyz, q, off, noff)
    assert (wd == np.float32(1e10)).any()
    assert np.array_equal(host(idx), wi) and np.array_equal(host(d2), wd)


def test_heap_basic_impl_is_the_same_heap(pops, monkeypatch):
    """GEOT_NN_IMPL=basic keeps 64 lists per workgroup up to nsample 256 (128 KB of LDS): same mechanics, same output."""
    xyz, q, off, noff = _ragged([3000, 2000], start=5)
    args = (dev(xyz), dev(q), dev(off), dev(noff))
    for ns in (129, 256):
        a = _heap(pops, *args, ns)
        monkeypatch.setenv("GEOT_NN_IMPL", "basic")
        b = _heap(pops, *args, ns)
        monkeypatch.delenv("GEOT_NN_IMPL")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 2. pointops.knn: selection + certification + literal heap for the rest ---------------------------------------
@pytest.mark.parametrize("k", [64, 100, 257, 1000])
def test_pointops_knn_equals_literal_heap(pops, k):
    from geot_amd.pointops.functions import pointops
    B, N = 2, 3000
    xyz, _ = make_batch(B, N, start_index=70 + k, dup_frac=0.05)
    xyz[1] = (xyz[1] * 48).round() / 48                                  # quantised: many exact distance ties
    x = dev(xyz)
    idx, dist = pointops.knn(x, x, k)
    off = dev(np.array([N, 2 * N]), torch.int32)
    widx, wd2 = _heap(pops, x.reshape(-1, 3).contiguous(), x.reshape(-1, 3).contiguous(), off, off, k)
    want_local = widx.view(B, N, k).long() - (torch.arange(B, device=DEV) * N)[:, None, None]
    assert torch.equal(idx, want_local)
    assert torch.equal(dist, torch.sqrt(wd2).view(B, N, k))


def test_pointops_knn_fewer_points_than_k(pops):
    """No query can be certified (k + 1 > n): the literal heap serves all of them, sentinels included."""
    from geot_amd.pointops.functions import pointops
    xyz, _ = make_batch(2, 300, start_index=4, dup_frac=0.05)
    x = dev(xyz)
    idx, dist = pointops.knn(x[:, :100].contiguous(), x, 300)
    off = dev(np.array([300, 600]), torch.int32)
    widx, wd2 = _heap(pops, x.reshape(-1, 3).contiguous(), x[:, :100].reshape(-1, 3).contiguous(), off,
                      dev(np.array([100, 200]), torch.int32), 300)
    assert torch.equal(idx, widx.view(2, 100, 300).long() - (torch.arange(2, device=DEV) * 300)[:, None, None])
    assert torch.equal(dist, torch.sqrt(wd2).view(2, 100, 300))


# ---- 3. sorted kNN ------------------------------------------------------------------------------------------------
def _sorted_ref(oracle, q, ref, k):
    """The C oracle (insertion into a sorted list) where it is quick, the numpy restatement for long lists."""
    from oracle import np_ref
    if k <= 257:
        return oracle.knn_sorted(q, ref, k)
    return np_ref.knn_sorted(q, ref, k)


@pytest.mark.parametrize("k", [65, 129, 256, 257, 1000, 4096])
def test_sorted_matches_oracle(oracle, k):
    from geot_amd.knn_cuda import KNN, knn_sorted
    from geot_amd.openpoints.models.layers.knn import knn_point, KNN as OpKNN
    xyz, _ = make_batch(2, 5000, start_index=11 + k, dup_frac=0.05)
    xyz[1, 2500:] = (xyz[1, 2500:] * 32).round() / 32                   # lattice ties in half of one cloud
    q = xyz[:, ::50].copy()
    wi, wd = _sorted_ref(oracle, q, xyz, k)
    d2, idx = knn_sorted(dev(q), dev(xyz), k)
    assert np.array_equal(host(idx), wi) and np.array_equal(host(d2), wd)
    dist, idx = KNN(k, transpose_mode=True)(dev(xyz), dev(q))
    assert idx.dtype == torch.int64 and np.array_equal(host(idx), wi) and torch.equal(dist, torch.sqrt(d2))
    dist_t, idx_t = KNN(k, transpose_mode=False)(dev(xyz).transpose(1, 2).contiguous(), dev(q).transpose(1, 2).contiguous())
    assert torch.equal(idx_t.transpose(1, 2), idx) and torch.equal(dist_t.transpose(1, 2), dist)
    dist, idx = knn_point(k, dev(q), dev(xyz))
    assert np.array_equal(host(idx), wi) and torch.equal(dist, torch.sqrt(d2))
    dist, idx = OpKNN(k)(dev(q), dev(xyz))
    assert np.array_equal(host(idx), wi)


@pytest.mark.parametrize("k", [65, 1000, 4096])
def test_sorted_fewer_points_than_k(oracle, k):
    from oracle import np_ref
    from geot_amd.knn_cuda import knn_sorted
    xyz, _ = make_batch(2, 700, start_index=3, dup_frac=0.1)
    ref = xyz[:, :min(k - 1, 600)].copy()                                 # nr < k: tail slots are (inf, 0)
    q = xyz[:, ::7].copy()
    wi, wd = np_ref.knn_sorted(q, ref, k)
    d2, idx = knn_sorted(dev(q), dev(ref), k)
    assert np.isinf(wd[..., -1]).all()
    assert np.array_equal(host(idx), wi) and np.array_equal(host(d2), wd)


@pytest.mark.parametrize("k", [257, 4096])
def test_sorted_cloud_larger_than_lds(k):
    """40 000 points: the distances do not fit in LDS and are recomputed on every pass."""
    from oracle import np_ref
    from geot_amd.knn_cuda import knn_sorted
    xyz, _ = make_batch(1, 40000, start_index=17, dup_frac=0.05)
    q = xyz[:, ::1000].copy()
    wi, wd = np_ref.knn_sorted(q, xyz, k)
    d2, idx = knn_sorted(dev(q), dev(xyz), k)
    assert np.array_equal(host(idx), wi) and np.array_equal(host(d2), wd)


def test_sorted_basic_impl_agrees(monkeypatch):
    """The one-lane insertion kernel (GEOT_NN_IMPL=basic, launched with its LDS opt-in) and the selection kernel."""
    from geot_amd.knn_cuda import knn_sorted
    xyz, _ = make_batch(2, 3000, start_index=23, dup_frac=0.05)
    x, q = dev(xyz), dev(xyz[:, ::4])
    for k in (129, 256):
        a = knn_sorted(q, x, k)
        monkeypatch.setenv("GEOT_NN_IMPL", "basic")
        b = knn_sorted(q, x, k)
        monkeypatch.delenv("GEOT_NN_IMPL")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 4. full size -------------------------------------------------------------------------------------------------
def test_full_size(pops, oracle):
    from oracle import np_ref
    from geot_amd.knn_cuda import knn_sorted
    xyz, _ = make_batch(1, 24000, start_index=2, dup_frac=0.01)
    flat = xyz[0]
    off = np.array([24000], dtype=np.int32)
    idx, d2 = _heap(pops, dev(flat), dev(flat), dev(off), dev(off), 1000)
    wi, wd = oracle.knnquery_heap(1000, flat, flat, off, off)
    assert np.array_equal(host(idx), wi) and np.array_equal(host(d2), wd)
    d2, idx = knn_sorted(dev(xyz), dev(xyz), 512)
    pick = np.random.default_rng(0).choice(24000, 1000, replace=False)
    wi, wd = np_ref.knn_sorted(xyz[:, pick], xyz, 512)
    assert np.array_equal(host(idx)[:, pick], wi) and np.array_equal(host(d2)[:, pick], wd)


# ---- 5. graph capture ---------------------------------------------------------------------------------------------
def _capture_check(fn, inputs, fresh):
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream(DEV).wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    for _ in range(2):
        for dst, src in zip(inputs, fresh):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in out]
        want = fn()
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        fresh = [f.flip(0) if f.shape[0] > 1 else f for f in fresh]


def test_capture_long_lists():
    from geot_amd.knn_cuda import knn_sorted
    from geot_amd.pointops.functions import pointops

    def cloud(start):
        return torch.from_numpy(make_batch(2, 6000, start_index=start, dup_frac=0.02)[0]).to(DEV)
    x = cloud(0)
    q = x[:, ::8].contiguous()

    def fn():
        d2, i = knn_sorted(q, x, 1000)
        pi, pd = pointops.knn(q, x, 300)
        return d2, i, pi, pd
    y = cloud(9)
    _capture_check(fn, [x, q], [y, y[:, ::8].contiguous()])


# ---- 6. over the bounds -------------------------------------------------------------------------------------------
def test_over_the_bounds_raise_naming_them(pops):
    from geot_amd import _lib
    from geot_amd.knn_cuda import knn_sorted
    from geot_amd.pointops.functions import pointops
    H, S = _lib.KNN_KMAX_HEAP, _lib.KNN_KMAX_SORTED
    xyz, q, off, noff = _ragged([2000], start=1)
    with pytest.raises(RuntimeError, match=str(H)):
        _heap(pops, dev(xyz), dev(q), dev(off), dev(noff), H + 1)
    x = dev(make_batch(1, 5000, start_index=1)[0])
    with pytest.raises(RuntimeError, match=str(H)):
        pointops.knn(x, x, H + 1)
    with pytest.raises(RuntimeError, match=str(S)):
        knn_sorted(x[:, :10].contiguous(), x, S + 1)


# ---- the contracted-distance build ---------------------------------------------------------------------------------
def test_contracted_build_long_lists():
    from geot_amd import build as hip_build
    hip_build.build(variant="fma")
    env = dict(os.environ, GEOT_DISTANCE="fma")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_knn_large_k_contracted_check.py")], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "long-list contracted parity ok: fma" in r.stdout
