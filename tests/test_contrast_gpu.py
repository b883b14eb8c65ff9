"""The geot_contrast_* entry points and nativeContrastLoss_t on the GPU, every value and gradient element against the fp64
restatement tests/_contrast_ref.py within its derived bounds (a bound of zero demands an exact zero).  The entry points are
driven directly with outputs pre-filled with NaN (integer outputs with a sentinel); each family prints its largest
error / bound ratio."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _contrast_ref as cref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "contrast_loss_ref.npz")
DEV = "cuda:0"
SENTINEL = -7777
TH = 0.9


def _call(name, *args):
    from geot_amd.ext._common import call
    call(name, torch.device(DEV), *args)


def _ptr(t):
    return None if t is None else t.data_ptr()


def counter_tensor(value):
    return torch.tensor([value - (1 << 64) if value >= 1 << 63 else value], dtype=torch.long).to(DEV)


def counter_value(t):
    return int(t.item()) & 0xFFFFFFFFFFFFFFFF


def select_gpu(score, s, th=TH, perms=None, seed=0, counter=None):
    """-> dict of numpy outputs (+ the device tensors under "_dev")."""
    from geot_amd import _lib
    b, p = score.shape
    sc = torch.from_numpy(np.ascontiguousarray(score, dtype=np.float32)).to(DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    ws = torch.full((int(_lib.load().geot_contrast_select_ws_ints(b, p)),), SENTINEL, **i32)
    anchors, count = torch.full((b * s,), SENTINEL, **i32), torch.full((b + 1,), SENTINEL, **i32)
    rows, inv = torch.full((s,), SENTINEL, **i32), torch.full((b * p,), SENTINEL, **i32)
    perm = perm_q = None
    if perms is not None:
        perm = torch.zeros((b, s), dtype=torch.long)
        for c, row in enumerate(perms[0]):
            m = min(len(row), s)
            perm[c, :m] = torch.as_tensor(np.asarray(row[:m], dtype=np.int64))
        perm_q = torch.zeros(s, dtype=torch.long)
        m = min(len(perms[1]), s)
        perm_q[:m] = torch.as_tensor(np.asarray(perms[1][:m], dtype=np.int64))
        perm, perm_q = perm.to(DEV), perm_q.to(DEV)
    _call("geot_contrast_select", b, p, s, float(th), _ptr(sc), _ptr(perm), _ptr(perm_q), seed, _ptr(counter), _ptr(ws),
          _ptr(anchors), _ptr(count), _ptr(rows), _ptr(inv))
    torch.cuda.synchronize()
    return {"anchors": anchors.cpu().numpy(), "count": count.cpu().numpy(), "rows": rows.cpu().numpy(),
            "inv": inv.cpu().numpy(), "_dev": (anchors, count, rows, inv), "dims": (b, p, s)}


def loss_gpu(feat_s, feat_t, sel, bank, channels_first=False, g=1.0):
    """feat_* (B, P, D) numpy, point-major; handed over in the asked layout.  -> dict of numpy outputs, grad point-major."""
    from geot_amd import _lib
    b, p, s = sel["dims"]
    d = feat_s.shape[-1]
    cap = b * s
    anchors, count, rows, inv = sel["_dev"]

    def dev(x):
        x = np.ascontiguousarray(x.transpose(0, 2, 1) if channels_first else x, dtype=np.float32)
        return torch.from_numpy(x).to(DEV)
    fs, ft, bk = dev(feat_s), dev(feat_t), torch.from_numpy(np.ascontiguousarray(bank, dtype=np.float32)).to(DEV)
    nan = dict(dtype=torch.float32, device=DEV)
    xhat, that, gdir, rws = (torch.full((cap, d), float("nan"), **nan) for _ in range(4))
    norm, ell = torch.full((cap,), float("nan"), **nan), torch.full((cap,), float("nan"), **nan)
    ws = torch.full((int(_lib.load().geot_contrast_ws_floats(b, s, d)),), float("nan"), **nan)
    loss, grad = torch.full((1,), float("nan"), **nan), torch.full(tuple(fs.shape), float("nan"), **nan)
    up = torch.tensor([g], **nan)
    tau, tau_b = float(np.float32(0.1)), 1.0
    _call("geot_contrast_loss", b, p, d, s, int(channels_first), _ptr(fs), _ptr(ft), _ptr(anchors), _ptr(count), _ptr(bk), tau,
          tau_b, _ptr(xhat), _ptr(that), _ptr(norm), _ptr(ws), _ptr(ell), _ptr(gdir), _ptr(loss))
    _call("geot_contrast_loss_grad", b, p, d, s, int(channels_first), _ptr(count), _ptr(inv), _ptr(xhat), _ptr(norm),
          _ptr(gdir), _ptr(up), tau_b, _ptr(rws), _ptr(grad))
    torch.cuda.synchronize()
    gr = grad.cpu().numpy()
    return {"loss": float(loss.item()), "ell": ell.cpu().numpy(), "grad": gr.transpose(0, 2, 1) if channels_first else gr,
            "that": that.cpu().numpy(), "xhat": xhat.cpu().numpy(), "_that": that, "_bank": bk}


def scores_with_counts(rng, p, ks):
    score = (rng.random((len(ks), p)) * 0.89).astype(np.float32)
    for c, k in enumerate(ks):
        where = rng.permutation(p)[:k]
        score[c, where] = (0.9 + 0.0999 * rng.random(k)).astype(np.float32)
        if k:
            score[c, where[0]] = np.float32(TH)              # equal to the threshold exactly: a candidate
        rest = np.setdiff1d(np.arange(p), where)
        if len(rest):
            score[c, rest[0]] = np.nan                       # never a candidate
    return score


# ------------------------------------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("p", [1, 63, 64, 65, 255, 256, 257, 700])
def test_selection_matches_the_restatement_bit_for_bit(p):
    s, seed, start = 16, 0x1234567890ABCDEF, (1 << 64) - 3           # (the counter wraps inside the call)
    ks = [min(k, p) for k in (0, 1, s - 1, s, s + 1, p, 0, p)]         # an empty cloud beside a full one, twice
    rng = np.random.default_rng(p)
    score = scores_with_counts(rng, p, ks)
    b = len(ks)
    counter = counter_tensor(start)
    got = select_gpu(score, s, seed=seed, counter=counter)
    want = cref.select(score, TH, s, seed=seed, counter=start)
    a = want["A"]
    assert list(got["count"]) == list(want["m"]) + [a] and a == sum(min(k, s) for k in ks)
    assert np.array_equal(got["anchors"][:a], want["anchors"]) and (got["anchors"][a:] == -1).all()
    cnt = min(a, s)
    assert np.array_equal(got["rows"][:cnt], want["rows"]) and (got["rows"][cnt:] == -1).all()
    inv = np.full(b * p, -1)
    inv[want["anchors"]] = np.arange(a)
    assert np.array_equal(got["inv"], inv)
    assert len(set(got["anchors"][:a].tolist())) == a and len(set(got["rows"][:cnt].tolist())) == cnt     # distinct
    assert np.isnan(score).any() and all(np.isfinite(score.reshape(-1)[got["anchors"][:a]]))
    assert counter_value(counter) == (start + b + 1) & 0xFFFFFFFFFFFFFFFF
    again = select_gpu(score, s, seed=seed, counter=counter_tensor(start))          # the same counter: the same rows
    assert all(np.array_equal(got[k], again[k]) for k in ("anchors", "count", "rows", "inv"))
    moved = select_gpu(score, s, seed=seed, counter=counter)                        # the advanced one: other rows
    assert np.array_equal(moved["count"], got["count"])
    if p >= 255:
        assert not np.array_equal(moved["anchors"], got["anchors"])
    # the host mode: given permutations, the counter is neither read nor written
    perms = ([rng.permutation(k) for k in ks], rng.permutation(a))
    host = select_gpu(score, s, perms=perms)
    want = cref.select(score, TH, s, perms=perms)
    assert np.array_equal(host["anchors"][:a], want["anchors"]) and np.array_equal(host["rows"][:cnt], want["rows"])
    assert list(host["count"]) == list(want["m"]) + [a]


# ------------------------------------------------------------------------------------------------------- loss and gradient
def _case(rng, b, p, d, s, ks, special=True):
    score = scores_with_counts(rng, p, ks)
    feat_s = rng.standard_normal((b, p, d)).astype(np.float32)
    feat_t = (0.5 * feat_s + rng.standard_normal((b, p, d))).astype(np.float32)
    bank = rng.standard_normal((4 * s, d))
    bank = (bank / np.sqrt((bank * bank).sum(1, keepdims=True))).astype(np.float32)
    return score, feat_s, feat_t, bank


def _check(got, want, bd, tag, worst):
    a = len(want["anchors"])
    r = {"loss": cref.ratio(got["loss"] - want["loss"], bd["loss"]),
         "ell": cref.ratio(got["ell"][:a] - want["ell"], bd["ell"]),
         "grad": cref.ratio(got["grad"] - want["grad"], cref.grad_bound_dense(want["grad"].shape, want["anchors"], bd["grad"]))}
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)
    assert all(v <= 1 for v in r.values()), (tag, r)
    assert np.isnan(got["ell"][a:]).all(), tag           # slots beyond A idle


LOSS_CASES = [
    # d, s, clouds' candidate counts, p, channels_first, upstream
    (1, 16, (5, 20), 96, False, 1.0), (37, 16, (16, 3), 96, True, -2.5), (128, 16, (40, 17), 96, True, 1.0),
    (256, 16, (9, 16), 96, False, 0.375), (128, 64, (63, 0), 130, True, 1.0), (37, 64, (64, 0), 130, False, 3.0),
    (128, 64, (64, 1), 130, False, 1.0), (256, 64, (70, 1), 130, True, 1.0), (128, 1, (5, 0, 1), 40, True, 1.0),
    (64, 1, (1,), 7, False, 2.0), (192, 16, (1, 0), 33, True, 1.0),
]


@pytest.mark.parametrize("d,s,ks,p,cf,g", LOSS_CASES)
def test_loss_and_gradient_against_fp64(d, s, ks, p, cf, g):
    rng = np.random.default_rng((d, s, p))
    b = len(ks)
    score, feat_s, feat_t, bank = _case(rng, b, p, d, s, ks)
    perms = ([rng.permutation(k) for k in ks], rng.permutation(sum(min(k, s) for k in ks)))
    want_sel = cref.select(score, TH, s, perms=perms)
    anchors = want_sel["anchors"]
    flat_s, flat_t = feat_s.reshape(-1, d), feat_t.reshape(-1, d)
    if len(anchors) >= 1:
        flat_t[anchors[0]] = 3.0 * flat_s[anchors[0]]                 # parallel rows: u_aa = 1 / tau
        t0 = flat_t[anchors[0]].astype(np.float64)
        bank[1] = (t0 / max(np.sqrt((t0 * t0).sum()), 1e-12)).astype(np.float32)     # a bank row equal to a positive
    if len(anchors) >= 3:
        flat_s[anchors[2]] = 0.0                                      # a zero feature row: x^ = 0, the gradient dy / eps
    sel = select_gpu(score, s, perms=perms)
    got = loss_gpu(feat_s, feat_t, sel, bank, cf, g)
    want = cref.loss_grad(feat_s, feat_t, anchors, bank, g)
    want["anchors"] = anchors
    if len(anchors) >= 1:
        assert abs((want["xhat"][0] * want["that"][0]).sum() - 1.0) < 1e-6
    worst = {}
    _check(got, want, cref.bounds(d, len(anchors), s, want["norm"], g), (d, s, ks), worst)
    assert np.abs(want["grad"]).max() > 0
    print("loss/gradient d=%d s=%d A=%d %s: error / bound %s" % (d, s, len(anchors), "channel-first" if cf else "point-major", worst))


def test_default_shape_s1024_d128():
    b, p, d, s = 2, 2100, 128, 1024
    rng = np.random.default_rng(1024)
    ks = (1500, 900)
    score, feat_s, feat_t, bank = _case(rng, b, p, d, s, ks)
    seed, start = 5, 77
    sel = select_gpu(score, s, seed=seed, counter=counter_tensor(start))
    want_sel = cref.select(score, TH, s, seed=seed, counter=start)
    assert np.array_equal(sel["anchors"][:want_sel["A"]], want_sel["anchors"]) and want_sel["A"] == 1924
    got = loss_gpu(feat_s, feat_t, sel, bank, True, 1.0)
    want = cref.loss_grad(feat_s, feat_t, want_sel["anchors"], bank)
    want["anchors"] = want_sel["anchors"]
    worst = {}
    _check(got, want, cref.bounds(d, 1924, s, want["norm"]), "default", worst)
    print("default shape: error / bound", worst)


def test_no_anchor_and_one_anchor():
    b, p, d, s = 2, 50, 37, 16
    rng = np.random.default_rng(3)
    for ks in ((0, 0), (0, 1)):
        score, feat_s, feat_t, bank = _case(rng, b, p, d, s, ks)
        counter = counter_tensor(9)
        sel = select_gpu(score, s, seed=1, counter=counter)
        got = loss_gpu(feat_s, feat_t, sel, bank, False, 1.5)
        a = sum(ks)
        assert sel["count"][b] == a and counter_value(counter) == 9 + b + 1
        ptr = torch.tensor([13], dtype=torch.long, device=DEV)
        _call("geot_contrast_enqueue", b, d, s, _ptr(sel["_dev"][1]), _ptr(sel["_dev"][2]), _ptr(got["_that"]), _ptr(got["_bank"]),
              _ptr(ptr))
        torch.cuda.synchronize()
        if a == 0:
            assert got["loss"] == 0.0 and not got["grad"].any() and np.isnan(got["ell"]).all()
            assert np.array_equal(got["_bank"].cpu().numpy().view(np.uint32), bank.view(np.uint32)) and int(ptr) == 13
        else:
            want_sel = cref.select(score, TH, s, seed=1, counter=9)
            want = cref.loss_grad(feat_s, feat_t, want_sel["anchors"], bank, 1.5)
            want["anchors"] = want_sel["anchors"]
            _check(got, want, cref.bounds(d, 1, s, want["norm"], 1.5), "A=1", {})
            assert int(ptr) == 14


# ----------------------------------------------------------------------------------------------------------------- enqueue
@pytest.mark.parametrize("ptr0,ks,where,ptr1", [(0, (16, 5), (0, 16), 16), (48, (16, 16), (48, 64), 0), (57, (20, 3), (48, 64), 0),
                                                 (60, (2, 1), (60, 63), 63), (61, (2, 1), (61, 64), 0), (62, (2, 1), (61, 64), 0)])
def test_enqueue_rows_and_pointer(ptr0, ks, where, ptr1):
    b, p, d, s = 2, 96, 37, 16
    rng = np.random.default_rng(ptr0)
    score, feat_s, feat_t, bank = _case(rng, b, p, d, s, ks)
    sel = select_gpu(score, s, seed=2, counter=counter_tensor(ptr0))
    got = loss_gpu(feat_s, feat_t, sel, bank)
    want_sel = cref.select(score, TH, s, seed=2, counter=ptr0)
    want = cref.loss_grad(feat_s, feat_t, want_sel["anchors"], bank)
    ptr = torch.tensor([ptr0], dtype=torch.long, device=DEV)
    _call("geot_contrast_enqueue", b, d, s, _ptr(sel["_dev"][1]), _ptr(sel["_dev"][2]), _ptr(got["_that"]), _ptr(got["_bank"]),
          _ptr(ptr))
    torch.cuda.synchronize()
    new, ptr_want, rng_want = cref.enqueue(want["that"], want_sel["rows"], bank, ptr0, s)
    assert rng_want == where and ptr_want == ptr1 == int(ptr)
    out = got["_bank"].cpu().numpy()
    lo, hi = where
    outside = np.r_[0:lo, hi:4 * s]
    assert np.array_equal(out[outside].view(np.uint32), bank[outside].view(np.uint32))
    r = cref.ratio(out[lo:hi] - new[lo:hi], cref.bounds(d, want_sel["A"], s, want["norm"])["bank"])
    print("enqueue ptr %d -> %d rows [%d, %d): error / bound %.3g" % (ptr0, ptr1, lo, hi, r))
    assert r <= 1


# ------------------------------------------------------------------------------------------------------------------ module
def test_module_host_mode_follows_the_reference_over_six_calls():
    from geot_amd.utils.cluster_contrastloss import nativeContrastLoss_t
    z = np.load(FIXTURE)
    f = cref.FIXTURE
    torch.manual_seed(f["seed"])
    torch.randn((4 * f["S"], 128))            # what the reference's constructor draws before its bank is replaced
    mod = nativeContrastLoss_t(sample_nums=f["S"], dim=f["D"], th=f["th"], device=DEV, bank=torch.from_numpy(cref.fixture_bank()))
    queue, ptr_t = mod.point_queue, mod.point_queue_ptr
    ptr_t.fill_(f["ptr0"])
    ref = cref.Reference(f["S"], cref.fixture_bank(), f["th"])
    ref.ptr = f["ptr0"]
    worst = {}
    for i in range(len(f["K"])):
        feat_s, score, feat_t = (torch.from_numpy(a).to(DEV) for a in cref.fixture_inputs(i))
        feat_s.requires_grad_(True)
        ref.bank = mod.point_queue.cpu().numpy().astype(np.float64)
        out = mod(feat_s, score, feat_t)
        assert len(out) == 4 and out[2] is out[0] and int(out[1]) == 0 and int(out[3]) == 0
        out[0].backward()
        np_in = cref.fixture_inputs(i)
        want = ref(np_in[0], np_in[1], np_in[2], perms=(z["perm_%d" % i], z["perm_q_%d" % i]))
        assert int(mod.anchors) == want["A"]
        bd = cref.bounds(f["D"], want["A"], f["S"], want["norm"])
        lo, hi = want["written"]
        bank_bound = np.zeros((4 * f["S"], f["D"]))
        bank_bound[lo:hi] = bd["bank"]
        r = {"loss": cref.ratio(float(out[0].detach()) -want["loss"], bd["loss"]),
             "grad": cref.ratio(feat_s.grad.cpu().numpy() - want["grad"],
                                cref.grad_bound_dense(want["grad"].shape, want["anchors"], bd["grad"])),
             "bank": cref.ratio(mod.point_queue.cpu().numpy() - want["bank"], bank_bound),
             # ... and of the reference's own fp32 results: two implementations within the bound of one referee
             "loss_ref": cref.ratio(float(out[0].detach()) -float(z["loss_%d" % i]), 2 * bd["loss"]),
             "grad_ref": cref.ratio(feat_s.grad.cpu().numpy() - z["grad_%d" % i],
                                    2 * cref.grad_bound_dense(want["grad"].shape, want["anchors"], bd["grad"]))}
        assert all(v <= 1 for v in r.values()), (i, r)
        assert int(mod.point_queue_ptr) == int(z["ptr_%d" % i]) == want["ptr"]
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert mod.point_queue is queue and mod.point_queue_ptr is ptr_t          # never rebound
    print("module, host mode, six calls: error / bound", worst)


def test_module_refusals():
    from geot_amd.utils.cluster_contrastloss import nativeContrastLoss_t
    from geot_amd.openpoints.dataset.sample_draw import DeviceDraws
    mod = nativeContrastLoss_t(sample_nums=4, dim=8, device=DEV, draws=DeviceDraws(1))
    fs, sc = torch.randn(2, 10, 8, device=DEV), torch.rand(2, 10, device=DEV)
    with pytest.raises(ValueError, match="feat_t"):
        mod(fs, sc, fs.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="fp32"):
        mod(fs.double(), sc, fs.double())
    with pytest.raises(RuntimeError, match="contiguous"):
        mod(fs.transpose(1, 2), sc, fs.transpose(1, 2), channels_first=True)
    with pytest.raises(RuntimeError, match="channels"):
        mod(fs, sc[:, :8].contiguous(), fs, channels_first=True)          # read as (B, D = 10, P = 8)
    with pytest.raises(RuntimeError, match="score"):
        mod(fs, sc[:, :9].contiguous(), fs)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        mod(fs.cpu(), sc, fs)


def _device_inputs(i, b=2, p=300, d=128):
    rng = np.random.default_rng((77, i))
    score, feat_s, feat_t, _ = _case(rng, b, p, d, 16, (rng.integers(0, 40), rng.integers(10, 200)))
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (feat_s.transpose(0, 2, 1), score, feat_t.transpose(0, 2, 1))]


def _fresh(seed=11, counter=(1 << 63) + 5):
    from geot_amd.utils.cluster_contrastloss import nativeContrastLoss_t
    from geot_amd.openpoints.dataset.sample_draw import DeviceDraws
    bank = np.random.default_rng(5).standard_normal((64, 128))
    bank = torch.from_numpy((bank / np.sqrt((bank * bank).sum(1, keepdims=True))).astype(np.float32))
    mod = nativeContrastLoss_t(sample_nums=16, dim=128, device=DEV, draws=DeviceDraws(seed, counter), bank=bank)
    mod.point_queue_ptr.fill_(40)
    return mod


def _eager(mod, n=3):
    out = []
    for i in range(n):
        fs, sc, ft = _device_inputs(i)
        fs.requires_grad_(True)
        loss = mod(fs, sc, ft, channels_first=True)[0]
        (loss * 1.5).backward()
        out.append([t.clone() for t in (loss.detach(), fs.grad, mod.point_queue, mod.point_queue_ptr, mod.draw_counter, mod.anchors)])
    torch.cuda.synchronize()
    return out


def _same(a, b):
    return all(x.dtype == y.dtype and torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                                  y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))


def test_two_runs_are_bit_equal_and_a_captured_call_replays_like_eager_ones():
    first, second = _eager(_fresh()), _eager(_fresh())
    assert all(_same(a, b) for a, b in zip(first, second))
    assert [counter_value(c[4]) for c in first] == [(1 << 63) + 5 + 3 * (i + 1) for i in range(3)]
    assert len({int(c[3]) for c in first}) == 3 and all(0 < int(c[5]) <= 32 for c in first)
    assert not _same(first[0][:2], _eager(_fresh(seed=12), 1)[0][:2])                 # another seed: other anchors
    mod = _fresh()
    static = [t.clone() for t in _device_inputs(0)]
    static[0].requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            loss = mod(static[0], static[1], static[2], channels_first=True)[0]
            grad, = torch.autograd.grad(loss * 1.5, static[0])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    # (capture runs nothing: state is what _fresh() made)
    for i in range(3):
        with torch.no_grad():
            for dst, src in zip(static, _device_inputs(i)):
                dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        got = [loss.detach(), grad, mod.point_queue, mod.point_queue_ptr, mod.draw_counter, mod.anchors]
        assert _same(got, first[i]), i
