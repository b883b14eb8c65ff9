"""Teacher-student point contrastive loss -- mirror of utils/cluster_contrastloss.py's ``nativeContrastLoss_t``
(:1188-1408; train.py:267 builds it and hands it to train_one_epoch, which never calls it; the configured run keeps
``use_contrastive: False``).  The module's other three classes are not mirrored.

What the class computes, per call on feat_s (B, P, D), score (B, P), feat_t (B, P, D):

1. select (:1233-1264)  per cloud the points with score >= th in ascending order, K of them; m = min(K, sample_nums) anchors
   ``cand[perm[:m]]``, perm a permutation of [0, K); anchors packed cloud after cloud, A in all;
2. normalise (:1385, :1388)  x^ = F.normalize(x) of the A selected rows of feat_s, t^ of feat_t (the reference normalises
   all B * P rows and keeps at most sample_nums per cloud);
3. loss (:1337-1377)  u = x^ t^T / 0.1 over the A anchors, v = x^ Q^T / 0.1 over the 4 * sample_nums bank rows, each shifted
   by its OWN row maximum (detached): l_a = -(0.1 / 1) ((u_aa - max u_a) - log(sum_j exp(u_aj - max u_a) + sum_q exp(v_aq -
   max v_a))), loss = mean l_a.  Only the diagonal of the reference's (A, A) log_prob reaches the loss (its mask is the
   identity); neither matrix is materialised here;
4. enqueue (:1207-1220)  after the loss has read the bank: min(A, sample_nums) rows t^[perm_q], normalised once more, go
   to the bank at the pointer (or to its last rows, with the pointer back at 0, when they would pass the end).

The whole call is ten launches of csrc/contrast.hip (geot_contrast_select / _loss / _enqueue in the forward, _loss_grad in
the backward) behind ONE autograd Function; the bank write is part of the forward.  The gradient reaches feat_s alone:
feat_t is a constant (every use in the reference's loop is detached or under no_grad), one that requires grad is refused.

A = 0 is defined HERE: the loss is exactly 0, the gradient all zeros, bank and pointer untouched.  The reference raises
instead (IndexError in torch.max at :1351 on an empty matrix; its ``if feats_ is None`` branch at :1393 can never be taken,
len(X_) being the number of clouds).

Draws.  ``draws=None`` (the default) is the host mode: the counts are read back (one synchronisation) and
``torch.randperm(K_b)`` per cloud, then ``torch.randperm(A)``, come from the global torch generator in the reference's
order, so the same seed gives the reference's anchors.  ``draws=DeviceDraws(seed)`` is the device mode: the keyed bijection
of geot_sample_draw with the draw ids taken from a counter in device memory (cloud b: counter + b, the bank rows: counter
+ B; the call advances it by B + 1) -- no synchronisation, safe to capture, and a replayed graph draws a new subset
every time.  The DeviceDraws object gives the seed and the first counter value; afterwards the counter lives on the
device (``draw_counter``).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from ..ext._common import call, need, ptr
from ..openpoints.dataset.sample_draw import DeviceDraws

MAX_B, MAX_D, MAX_S = _lib.CONTRAST_MAX_B, _lib.CONTRAST_MAX_D, _lib.CONTRAST_MAX_S


def _check_inputs(feat_s, score, feat_t, dim, channels_first):
    for name, t in (("feat_s", feat_s), ("score", score), ("feat_t", feat_t)):
        if not torch.is_tensor(t):
            raise TypeError("nativeContrastLoss_t: %s must be a tensor, got %s" % (name, type(t).__name__))
        need(t.is_cuda, "nativeContrastLoss_t: CPU not supported (%s must live on the GPU)" % name)
        need(t.dtype == torch.float32, "nativeContrastLoss_t: %s must be fp32, got %s" % (name, t.dtype))
        need(t.is_contiguous(), "nativeContrastLoss_t: %s must be contiguous" % name)
        need(t.device == feat_s.device, "nativeContrastLoss_t: %s is on %s, feat_s on %s" % (name, t.device, feat_s.device))
    need(feat_s.dim() == 3 and score.dim() == 2 and feat_t.shape == feat_s.shape,
         "nativeContrastLoss_t: feat_s and feat_t must be two equal 3-d tensors and score 2-d, got %s, %s, %s"
         % (tuple(feat_s.shape), tuple(feat_t.shape), tuple(score.shape)))
    b, p, d = (feat_s.shape[0], feat_s.shape[2], feat_s.shape[1]) if channels_first else tuple(feat_s.shape)
    need(tuple(score.shape) == (b, p), "nativeContrastLoss_t: score must be (%d, %d), got %s" % (b, p, tuple(score.shape)))
    need(d == dim, "nativeContrastLoss_t: the features have %d channels, the bank %d" % (d, dim))
    need(1 <= b <= MAX_B and p >= 1 and b * p <= 2 ** 31 - 1,
         "nativeContrastLoss_t: 1 <= B <= %d, P >= 1, B * P < 2^31, got B = %d, P = %d" % (MAX_B, b, p))
    if feat_t.requires_grad:
        raise ValueError("nativeContrastLoss_t: feat_t is a constant of this loss; detach it (no gradient is formed for it)")
    return b, p, d


class _ContrastFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat_s, score, feat_t, owner, channels_first, perms):
        b, p, d = (feat_s.shape[0], feat_s.shape[2], feat_s.shape[1]) if channels_first else tuple(feat_s.shape)
        s, dev = owner.sample_nums, feat_s.device
        cap = b * s
        lib = _lib.load()
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        ws_i = torch.empty(int(lib.geot_contrast_select_ws_ints(b, p)), **i32)
        anchors, count = torch.empty(cap, **i32), torch.empty(b + 1, **i32)
        rows_q, inv = torch.empty(s, **i32), torch.empty(b * p, **i32)
        perm, perm_q = perms if perms is not None else (None, None)
        call("geot_contrast_select", dev, b, p, s, float(owner.th), ptr(score), ptr(perm), ptr(perm_q), owner.seed,
             None if perms is not None else ptr(owner.draw_counter), ptr(ws_i), ptr(anchors), ptr(count), ptr(rows_q), ptr(inv))
        xhat, that = torch.empty((cap, d), **f32), torch.empty((cap, d), **f32)
        norm, ell, gdir = torch.empty(cap, **f32), torch.empty(cap, **f32), torch.empty((cap, d), **f32)
        ws_f = torch.empty(int(lib.geot_contrast_ws_floats(b, s, d)), **f32)
        loss = torch.empty((), **f32)
        call("geot_contrast_loss", dev, b, p, d, s, int(channels_first), ptr(feat_s), ptr(feat_t), ptr(anchors), ptr(count),
             ptr(owner.point_queue), float(owner.temperature), float(owner.base_temperature), ptr(xhat), ptr(that), ptr(norm),
             ptr(ws_f), ptr(ell), ptr(gdir), ptr(loss))
        call("geot_contrast_enqueue", dev, b, d, s, ptr(count), ptr(rows_q), ptr(that), ptr(owner.point_queue),
             ptr(owner.point_queue_ptr))
        ctx.save_for_backward(count, inv, xhat, norm, gdir)
        ctx.dims = (b, p, d, s, bool(channels_first), float(owner.base_temperature), tuple(feat_s.shape))
        n_anchors = count[b]
        ctx.mark_non_differentiable(n_anchors)
        return loss, n_anchors

    @staticmethod
    def backward(ctx, grad_loss, _grad_count):
        count, inv, xhat, norm, gdir = ctx.saved_tensors
        b, p, d, s, channels_first, tau_b, shape = ctx.dims
        dev = xhat.device
        g = grad_loss.detach().to(torch.float32).contiguous()
        rows = torch.empty((b * s, d), dtype=torch.float32, device=dev)
        grad = torch.empty(shape, dtype=torch.float32, device=dev)
        call("geot_contrast_loss_grad", dev, b, p, d, s, int(channels_first), ptr(count), ptr(inv), ptr(xhat), ptr(norm),
             ptr(gdir), ptr(g), tau_b, ptr(rows), ptr(grad))
        return grad, None, None, None, None, None


class nativeContrastLoss_t(nn.Module):
    """``nativeContrastLoss_t(sample_nums)`` of the reference, on fused kernels (see the module docstring).

    sample_nums 1..1024, dim 1..256 (the reference: 128), th the selection threshold (the reference hard-wires 0.9, :1390).
    bank: the initial (4 * sample_nums, dim) bank; None: the reference's own statement, F.normalize(torch.randn(4 S, dim))
    from the global torch generator, drawn on the host and uploaded.  draws: None (host mode) or a DeviceDraws (device
    mode).  Attributes as in the reference: point_queue, point_queue_ptr (a device int64 tensor that is never rebound),
    temperature, base_temperature; anchors: A of the last call (a device tensor)."""

    def __init__(self, sample_nums=1024, dim=128, th=0.9, device=None, draws=None, bank=None):
        super().__init__()
        for name, v, hi in (("sample_nums", sample_nums, MAX_S), ("dim", dim, MAX_D)):
            if not isinstance(v, int) or isinstance(v, bool):
                raise TypeError("nativeContrastLoss_t: %s must be an int, got %r" % (name, v))
            if not 1 <= v <= hi:
                raise ValueError("nativeContrastLoss_t: %s must be in 1..%d, got %r" % (name, hi, v))
        if isinstance(th, bool) or not isinstance(th, (int, float)) or not 0.0 < float(th) <= 1.0:
            raise ValueError("nativeContrastLoss_t: th must be a number in (0, 1], got %r" % (th,))
        if draws is not None and not isinstance(draws, DeviceDraws):
            raise TypeError("nativeContrastLoss_t: draws must be a DeviceDraws (or None: the reference's host draws)")
        self.sample_nums, self.dim, self.th = sample_nums, dim, float(th)
        self.temperature = 0.1
        self.base_temperature = 1
        self.ignore_label = 255
        self.num_classes = 17
        self.pixel_update_freq = sample_nums
        self.pixel_size = sample_nums * 4
        device = torch.device("cuda" if device is None else device)
        if device.type != "cuda":
            raise RuntimeError("nativeContrastLoss_t: CPU not supported (the loss runs on the GPU)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if bank is None:
            bank = F.normalize(torch.randn((self.pixel_size, dim)), p=2, dim=1)
        else:
            need(torch.is_tensor(bank) and tuple(bank.shape) == (self.pixel_size, dim) and bank.dtype == torch.float32,
                 "nativeContrastLoss_t: bank must be a (%d, %d) fp32 tensor" % (self.pixel_size, dim))
        self.point_queue = bank.detach().to(device).contiguous().clone()
        self.point_queue_ptr = torch.zeros(1, dtype=torch.long, device=device)
        self.draws = draws
        self.seed = draws.seed if draws is not None else 0
        # the draw counter on the device, two's complement of the unsigned 64-bit value
        first = draws.counter if draws is not None else 0
        self.draw_counter = torch.tensor([first - (1 << 64) if first >= 1 << 63 else first], dtype=torch.long).to(device)
        self.anchors = None

    def state_dict(self, *args, **kw):
        """What the loss carries from call to call: the bank, the queue pointer and the draw counter on the device (copies
        made on the current stream, no synchronisation), and the draws' seed.  (The bank is a plain attribute as in the
        reference, no registered buffer: nn.Module's own state_dict -- what any argument asks for -- is empty.)"""
        if args or kw:
            return super().state_dict(*args, **kw)
        from .. import checkpoint as ck
        ck.refuse_capture("nativeContrastLoss_t")
        return {"point_queue": ck.copied(self.point_queue), "point_queue_ptr": ck.copied(self.point_queue_ptr),
                "draw_counter": ck.copied(self.draw_counter), "seed": self.seed}

    def restore(self, r, state, key="contrast"):
        """The first half of load_state_dict: check `state` and hand the writes to r (a checkpoint.Restore)."""
        r.keys(state, ("point_queue", "point_queue_ptr", "draw_counter", "seed"), key)
        if state["seed"] != self.seed:
            raise ValueError("%s.seed: the state was saved with %r, the loss is built with %r (cfg contrast_seed)"
                             % (key, state["seed"], self.seed))
        for k in ("point_queue", "point_queue_ptr", "draw_counter"):
            r.tensor("%s.%s" % (key, k), getattr(self, k), state[k])

    def load_state_dict(self, state, *args, **kw):
        """Checked first (ValueError naming the key), then copied into the three device tensors, none of which is rebound."""
        if args or kw:
            return super().load_state_dict(state, *args, **kw)
        from .. import checkpoint as ck
        r = ck.Restore()
        self.restore(r, state)
        r.commit()

    def _host_perms(self, score, b, s):
        """The reference's draws: the counts are read back, randperm(K_b) per cloud and then randperm(A) from the global
        generator, in that order (:1249, :1210)."""
        counts = (score >= self.th).sum(1).tolist()          # the one synchronisation of the host mode
        perm = torch.zeros((b, s), dtype=torch.long)
        total = 0
        for c, k in enumerate(counts):
            m = min(k, s)
            perm[c, :m] = torch.randperm(k)[:m]
            total += m
        perm_q = torch.zeros(s, dtype=torch.long)
        if total > 0:        # (the reference does not get this far with A = 0: nothing is drawn)
            cnt = min(total, s)
            perm_q[:cnt] = torch.randperm(total)[:cnt]
        return perm.to(score.device), perm_q.to(score.device)

    def forward(self, feat_s, score, feat_t, cur=None, channels_first=False, perms=None):
        """feat_s, feat_t (B, P, D) -- or (B, D, P) with channels_first=True, read in place -- and score (B, P), all fp32,
        contiguous, on the bank's device.  Returns the reference's 4-tuple (loss, pcc_loss, ppc_loss, pcc_top2_loss), :1408.
        perms: (perm (B, S) int64, perm_q (S) int64) on the device replaces the host mode's draws (geot_contrast_select)."""
        b, p, d = _check_inputs(feat_s, score, feat_t, self.dim, channels_first)
        need(feat_s.device == self.point_queue.device,
             "nativeContrastLoss_t: the features are on %s, the bank on %s" % (feat_s.device, self.point_queue.device))
        s = self.sample_nums
        if perms is not None:
            need(len(perms) == 2 and all(torch.is_tensor(t) and t.dtype == torch.long and t.is_contiguous()
                                         and t.device == feat_s.device for t in perms)
                 and tuple(perms[0].shape) == (b, s) and tuple(perms[1].shape) == (s,),
                 "nativeContrastLoss_t: perms must be ((%d, %d), (%d,)) int64 tensors on %s" % (b, s, s, feat_s.device))
        elif self.draws is None:
            perms = self._host_perms(score, b, s)
        loss, self.anchors = _ContrastFunction.apply(feat_s, score.detach(), feat_t, self, bool(channels_first), perms)
        ppc_loss = loss
        pcc_loss = torch.tensor(0)
        pcc_top2_loss = torch.tensor(0)
        return loss, pcc_loss, ppc_loss, pcc_top2_loss
