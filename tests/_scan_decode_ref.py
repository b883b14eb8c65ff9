"""numpy restatement of geot_scan_decode_front / geot_scan_decode_finish (include/geot_hip.h, csrc/scan_decode.hip) and of the
rest of PointTransformer_seg_T's last decoder stage, with an operation-count error bound beside every value.

What is fp32 and what is fp64, and why:
  * the query position q and the squared distances are restated in float32, operation by operation: the neighbour CHOICE is
    a discrete function of those bits, so the reference must form the same bits (IEEE subtract, divide, multiply, add and
    square root are correctly rounded on both sides);
  * everything continuous -- the row z, the second stage, the head -- is float64, and every returned value comes with a
    bound on |fp32 result - fp64 value|.  For one row (front_rows) it holds for ANY order in which a correct fp32
    implementation may round; for the whole stage (last_stage) it is the probabilistic bound stated above linear().  With
    u = 2^-24 and gamma(k) = k u / (1 - k u), a value formed from terms t_i by at most k roundings per term lies within
    gamma(k) * sum |t_i| of the exact sum (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1); an input
    bound e_x passes through a linear map as |W| e_x and through ReLU unchanged (ReLU is 1-Lipschitz).
The bounds are derived from the counts and the magnitudes of the addends, never from what a kernel returned.
"""
import numpy as np

U = 2.0 ** -24
F32 = np.float32


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- the discrete part, float32 -----------------------------------------------------------------------------------------------
def query_positions(points, center, scale, view_center, view_scale):
    """(V, 3) float32 vertices of one slot -> q (V, 3) float32: pc_norm, then the view's centre-and-normalise; four single
    fp32 operations per coordinate."""
    p = np.asarray(points, F32)
    r = ((p - np.asarray(center, F32)) / F32(scale)).astype(F32)
    return ((r - np.asarray(view_center, F32)) / F32(view_scale)).astype(F32)


def sqdist(q, known):
    """(V, 3), (m, 3) float32 -> (V, m) float32, ((dx dx) + (dy dy)) + (dz dz) with every operation rounded."""
    d = (q[:, None, :].astype(F32) - known[None, :, :].astype(F32)).astype(F32)
    s = (d[..., 0] * d[..., 0]).astype(F32)
    s = (s + (d[..., 1] * d[..., 1]).astype(F32)).astype(F32)
    return (s + (d[..., 2] * d[..., 2]).astype(F32)).astype(F32)


def three_nn(q, known):
    """geot_three_nn's contract: the three smallest by (d2, index); a distance that is not below +inf (a NaN vertex) never
    enters, leaving (+inf, index 0) -> (d2 (V, 3) float32, idx (V, 3) int32)."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = sqdist(q, known)
    key = np.where(d < np.inf, d, np.inf)                 # NaN and +inf never pass `d < best`
    order = np.argsort(key, axis=1, kind="stable")[:, :3]  # stable: ties by ascending index
    d2 = np.take_along_axis(key, order, 1).astype(F32)
    idx = np.where(d2 < np.inf, order, 0).astype(np.int32)
    return d2, idx


def three_nn_fp64(q, known):
    """The same choice by brute force in float64 on the float32 positions (for inputs without near-ties)."""
    d = ((q[:, None, :].astype(np.float64) - known[None, :, :].astype(np.float64)) ** 2).sum(-1)
    return np.argsort(d, axis=1, kind="stable")[:, :3].astype(np.int32), np.sort(d, axis=1)[:, :4]


def fp_weights(d2):
    """geot_fp_weights statement for statement, float32."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (F32(1.0) / (np.sqrt(d2.astype(F32)).astype(F32) + F32(1e-8)).astype(F32)).astype(F32)
        norm = ((r[:, 0] + r[:, 1]).astype(F32) + r[:, 2]).astype(F32)
        return (r / norm[:, None]).astype(F32)


# ---- the continuous part, float64 with bounds ------------------------------------------------------------------------------------
def front_rows(q, idx, weight, a, skip_const, w_xyz, ch_scale, ch_shift, relu):
    """One slot's rows: q (V, 3), idx (V, 3), weight (V, 3), a (m, c_out), skip_const (c_out), w_xyz (c_out, 3), ch_scale /
    ch_shift (c_out) -> (z (V, c_out) float64, bound (V, c_out)).
    t = w0 a0 + w1 a1 + w2 a2 + skip + (Wx qx + Wy qy + Wz qz): seven addends; the longest chain a product sees is its own
    multiply and five additions (k = 6).  z = scale t + shift adds a multiply and an addition to every addend (k = 8) and two
    roundings to shift (covered by the same gamma).  ReLU does not round."""
    q, w, a = q.astype(np.float64), weight.astype(np.float64), a.astype(np.float64)
    sc, sh = ch_scale.astype(np.float64), ch_shift.astype(np.float64)
    g = a[idx]                                                     # (V, 3, c_out)
    interp = (w[:, :, None] * g).sum(1)
    mag = (np.abs(w)[:, :, None] * np.abs(g)).sum(1)
    xyz = q @ w_xyz.astype(np.float64).T
    mag = mag + np.abs(q) @ np.abs(w_xyz.astype(np.float64)).T + np.abs(skip_const.astype(np.float64))[None]
    t = interp + skip_const.astype(np.float64)[None] + xyz
    z = sc[None] * t + sh[None]
    bound = gamma(8) * (np.abs(sc)[None] * mag + np.abs(sh)[None])
    if relu:
        z = np.where(np.isnan(z), z, np.maximum(z, 0.0))
    return z, bound


# Through the whole stage (1536-, 384- and 128-term dot products, four layers) the worst-case form above is vacuous at the model's
# width: K u sum |t_i| per dot product and |W| e_x per layer give a bound of about 2 on logits of about 5.  The stage is
# bounded in the standard probabilistic model of rounding instead (Higham and Mary, "A new approach to probabilistic rounding
# error analysis", SIAM J. Sci. Comput. 41 (2019)): the relative roundings delta_j, |delta_j| <= u, are independent with mean
# zero.  An fp32 value is then its fp64 value plus a sum of independent bounded zero-mean terms c_j delta_j, and by Hoeffding's
# inequality  P(|sum c_j delta_j| > lambda u sqrt(sum c_j^2)) <= 2 exp(-lambda^2 / 2).  Every value therefore carries a SCALE
# s = u sqrt(sum c_j^2), propagated layer by layer, and the bound is LAMBDA s at the end (lambda enters once, not per layer):
#   * a dot product of K terms in any order: its K partial sums are each at most S = sum |t_i| in magnitude, one rounding each
#     (the products' own roundings are K more terms of at most max |t_i|): scale u sqrt(2 K) S at most;
#   * input scales pass through a linear map as sqrt(sum_i w_i^2 s_i^2) (independent terms add in quadrature), through a
#     per-channel affine as |scale| s, through ReLU unchanged (1-Lipschitz);
#   * the handful of roundings of a BatchNorm fold and apply, and of the seven-addend first stage, are taken at their worst case
#     (gamma(k) times the magnitudes) and added to the scale as they are: an over-estimate.
# LAMBDA = 8: 2 exp(-32) = 2.5e-14 per element, against some 5e5 elements per test.
LAMBDA = 8.0


def linear(w, x, sx, bias=None):
    """y = W x (+ bias) over the last axis of x (V, K), x with scale sx -> (y, s_y)."""
    w = w.astype(np.float64)
    k = w.shape[1]
    y = x @ w.T
    mag = np.abs(x) @ np.abs(w).T
    sy = np.sqrt((sx * sx) @ (w * w).T)
    if bias is not None:
        y = y + bias.astype(np.float64)[None]
        mag = mag + np.abs(bias.astype(np.float64))[None]
    return y, sy + U * np.sqrt(2.0 * (k + 1)) * mag


def batch_norm(x, sx, weight, bias, mean, var, eps, pre_bias=None, relu=False):
    """Eval BatchNorm over the channels (last axis), optionally with the bias of the convolution in front folded in:
    y = s (x + pre_bias - mean) + beta, s = weight / sqrt(var + eps).  An fp32 implementation folds (s, shift) in some order
    and applies s x + shift: var + eps, the reciprocal square root (2 ulp allowed), the product with weight, mean - pre_bias,
    the product with s, the subtraction from beta, then the apply's multiply and add -- no term sees more than 10 roundings;
    gamma(12) times the magnitudes covers any such order, worst case."""
    f = lambda v: np.asarray(v, np.float64)
    s = f(weight) / np.sqrt(f(var) + eps)
    pb = np.zeros_like(s) if pre_bias is None else f(pre_bias)
    y = s[None] * (x + pb[None] - f(mean)[None]) + f(bias)[None]
    mag = np.abs(s)[None] * (np.abs(x) + np.abs(pb)[None] + np.abs(f(mean))[None]) + np.abs(f(bias))[None]
    sy = np.abs(s)[None] * sx + gamma(12) * mag
    if relu:
        y = np.maximum(y, 0.0)
    return y, sy


def last_stage(params, f_l1, known, jaw, q, idx, weight):
    """The whole last stage of one slot in float64 from the kept features: params -- the numpy parameters of propogation_0 and
    seg_head (stage_params below); f_l1 (c, m) the centres' features; jaw 0 / 1; q, idx, weight (V, 3) the search
    -> (logits (V, C) float64, bound (V, C)), bound = LAMBDA times the propagated scale (the probabilistic model above)."""
    p = params
    c = f_l1.shape[0]
    w0 = p["w0"].astype(np.float64)
    a, sa = linear(w0[:, :c], f_l1.T.astype(np.float64), np.zeros(f_l1.T.shape))      # (m, c_out)
    g, sg = a[idx], sa[idx]
    qd, wd = q.astype(np.float64), weight.astype(np.float64)
    wx = w0[:, c + 2:c + 5]
    t = (wd[:, :, None] * g).sum(1) + w0[:, c + jaw][None] + qd @ wx.T
    mag = (np.abs(wd)[:, :, None] * np.abs(g)).sum(1) + np.abs(w0[:, c + jaw])[None] + np.abs(qd) @ np.abs(wx).T
    # seven addends, each through at most a multiply and six additions (whatever the order: interpolation first or the skip
    # columns first), worst case, on top of the first convolution's scale
    st = np.sqrt(((wd * wd)[:, :, None] * (sg * sg)).sum(1)) + gamma(7) * mag
    x, sx = batch_norm(t, st, *p["bn0"], relu=p["relu0"])
    for w, bn, relu in p["rest"]:
        x, sx = linear(w, x, sx)
        x, sx = batch_norm(x, sx, *bn, relu=relu)
    x, sx = linear(p["head_w0"], x, sx)
    x, sx = batch_norm(x, sx, *p["head_bn"], pre_bias=p["head_b0"])
    y, sy = linear(p["head_w1"], x, sx, bias=p["head_b1"])
    return y, LAMBDA * sy


def stage_params(model):
    """The parameters last_stage reads, as numpy arrays, from a PointTransformer_seg_T (any device)."""
    n = lambda t: t.detach().cpu().numpy().astype(np.float64)
    bn = lambda m: (n(m.weight), n(m.bias), n(m.running_mean), n(m.running_var), m.eps)
    layers = list(model.propogation_0.mlp.children())
    rest = [(n(l.conv.weight).reshape(l.conv.out_channels, -1), bn(l.bn.bn), hasattr(l, "activation")) for l in layers[1:]]
    head = model.seg_head
    return {"w0": n(layers[0].conv.weight).reshape(layers[0].conv.out_channels, -1), "bn0": bn(layers[0].bn.bn),
            "relu0": hasattr(layers[0], "activation"), "rest": rest,
            "head_w0": n(head[0].weight).reshape(head[0].out_channels, -1), "head_b0": n(head[0].bias), "head_bn": bn(head[1]),
            "head_w1": n(head[3].weight).reshape(head[3].out_channels, -1), "head_b1": n(head[3].bias)}


def argmax_rule(logits):
    """torch.argmax's rule per row of (V, C): the first NaN if there is one, else the first maximum."""
    nan = np.isnan(logits)
    return np.where(nan.any(1), nan.argmax(1), np.where(nan, -np.inf, logits).argmax(1)).astype(np.int64)


def near_ties(logits, bound):
    """Rows whose fp64 top-1 / top-2 margin is within twice the bound (the larger of the two classes' bounds): an fp32
    implementation inside its bound may pick either class there -> bool (V,)."""
    if logits.shape[1] < 2:
        return np.zeros(logits.shape[0], bool)
    order = np.argsort(-logits, axis=1, kind="stable")[:, :2]
    top = np.take_along_axis(logits, order, 1)
    b = np.take_along_axis(bound, order, 1).max(1)
    return (top[:, 0] - top[:, 1]) <= 2.0 * b


LABEL_CAP = 0.02        # the largest share of near-tie vertices a label comparison may leave out


def confusion_counts(pred, label, c):
    """geot_seg_confusion's row for one scan: (c (c + 1) + 1,) int64."""
    out = np.zeros(c * (c + 1) + 1, np.int64)
    for p, l in zip(pred.tolist(), label.tolist()):
        if l < 0 or l >= c:
            out[c * (c + 1)] += 1
        else:
            out[l * (c + 1) + (p if 0 <= p < c else c)] += 1
    return out


# ---- seeded fixtures shared by the CPU and GPU tests ---------------------------------------------------------------------------------
SCAN_SIZES = [150, 97]          # the model-level scans
# the smallest model that runs a forward pass: the EdgeConv stages are 384 wide, everything else is tiny
TINY = dict(trans_dim=384, depth=3, num_heads=4, group_size=4, num_group=8, encoder_dims=32, nclasses=17, drop_path_rate=0.0,
            downsample_targets=[32, 16, 8], extract_layers=[1, 2, 3])
N_SAMPLE = 64
MODEL_SEED = 20


def tiny_model():
    """The tiny eval model of the model-level tests, built on the CPU from a fixed seed (the caller moves it), with the
    BatchNorms of the last stage and the head given non-trivial running statistics and affine parameters."""
    import torch
    from geot_amd.openpoints.models.backbone.transformer import PointTransformer_seg_T
    gen_state = torch.random.get_rng_state()
    torch.manual_seed(MODEL_SEED)
    model = PointTransformer_seg_T(**TINY)
    g = torch.Generator().manual_seed(MODEL_SEED + 1)
    bns = [l.bn.bn for l in model.propogation_0.mlp.children()] + [model.seg_head[1]]
    for bn in bns:
        c = bn.num_features
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.3)
        bn.running_var.copy_(torch.rand(c, generator=g) * 1.5 + 0.25)
        bn.weight.data.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.data.copy_(torch.randn(c, generator=g) * 0.2)
    model.seg_head[0].bias.data.copy_(torch.randn(128, generator=g) * 0.1)
    model.seg_head[3].bias.data.copy_(torch.randn(17, generator=g) * 0.1)
    torch.random.set_rng_state(gen_state)
    return model.eval()


def tiny_scans(seed=77):
    """Two scans in scan coordinates (millimetres, away from the origin): [(points (M, 3) float32, labels (M,) int32)]."""
    rng = np.random.default_rng(seed)
    out = []
    for m in SCAN_SIZES:
        p = (rng.normal(size=(m, 3)) * np.array([9.0, 6.0, 4.0]) + np.array([14.0, -37.0, 61.0])).astype(F32)
        out.append((p, rng.integers(0, 17, size=m).astype(np.int32)))
    return out
