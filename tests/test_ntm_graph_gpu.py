"""GPU suite: the graph-loss kernels of the FixMatch+NTM loop (threeD_space_loss, feature_space_loss; csrc/ntm.hip) at every
launch and in-kernel branch, EVERY per-point value and EVERY gradient element against the fp64 helper tests/_ntm_graph_ref.py.

The C entry points are driven directly, with the test's own neighbour lists, orders and buffers (no kNN): outputs the kernel
must write in full are pre-filled with NaN, the accumulate-contract gradients get zeros.  Branches: the XCD-chunked walk and
its tails (one-point-per-wave and G = 2, 3, 4, 6 points per wave), its second trip, k = 1..64 (seg_shift, masked lanes, all
64 lanes live), in-degrees at the 64-slot capacity of the forward-built reverse lists (overflow list) and of the CSR form
(tail loop), the CSR offsets across the scan chunk of 4096, the register buckets of the run-time class count, sigma other than
1 (1/(2 s^2) != 1/(2 s)), an upstream gradient other than 1 in each of the four places it is applied, every processing order,
the workspace fall-backs and the argument checks.

Tolerance: derived in _ntm_graph_ref.py (forward (5 k + 38) u2 |terms|, gradient (terms + 32) u2 cond, + terms 2^-40 scale
|upstream| on the fixed-point path; a zero bound demands an exact zero), the same for every kernel and never fitted to one.
One correction to the first derivation: the signed (feature-space) forward subtracts, so its bound is relative to the sum of
the magnitudes of the point's terms, not to the cancelled value; for the unsigned loss the two are the same number.

Walk-tail clouds of fewer than 4 points run k = N - 1 (k = 3 distinct other points do not exist there).

Findings recorded here: the sorted kNN kernels leave (inf, id 0) in slots past the N references (in range; see
threeD_space_loss's docstring), so k >= N is refused on the host, as the reference's topk refuses it.

Largest error / bound per family (each test prints its own figures, pytest -s), MI355X, 2026-10-17:
walk tails grouped 0.068, walk tails one point per wave 0.055, second trip 0.080, k 0.068, in-degree 0.058, labels 0.063,
sigma 0.161, upstream 0.061, order 0.058, CSR scan 0.072, R buckets 0.061, fall-backs 0.058.  No kernel exceeded its bound.
Wall time of the large cases: 131 077 points (G = 2, forward + gather backward) 1.2 s, 65 569 points 0.2 s and 0.1 s."""
import numpy as np
import pytest
import torch

import _ntm_graph_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 17
INVALID = 1            # hipErrorInvalidValue


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def note(family, what, ratio):
    print("ntm-graph-ratio | %s | %s | %.4f" % (family, what, ratio))


class Case:
    """One graph on the device plus its fp64 references (computed once per (sigma, signed, upstream) and kept)."""

    def __init__(self, rng, b, n, k, c=C, labels="mixed", nbr=None, feat_dim=None, T=None):
        self.b, self.n, self.k, self.c, self.t = b, n, k, c, b * n
        t = self.t
        self.pos = rng.random((t, 3), dtype=np.float32)                                   # the unit cube: |x| <= 3 / (2 s^2)
        self.fd = feat_dim if feat_dim is not None else 5
        self.feats = rng.random((t, self.fd), dtype=np.float32) / np.float32(np.sqrt(self.fd))      # |f_i - f_j|^2 <= 1
        self.labels = labels if isinstance(labels, np.ndarray) else {
            "mixed": lambda: R.labels_mixed(rng, t), "equal": lambda: R.labels_equal(t),
            "different": lambda: R.labels_all_different(t)}[labels]()
        self.T = T if T is not None else R.row_stochastic(rng, t, c)
        self.nbr = nbr if nbr is not None else R.random_out_lists(rng, b, n, k)
        assert self.nbr.shape == (b, n, k) and self.nbr.dtype == np.int32 and self.nbr.min() >= 0 and self.nbr.max() < n
        self.g = R.to_global(self.nbr)
        self.d_pos, self.d_feats, self.d_lab = dev(self.pos), dev(self.feats), dev(self.labels.astype(np.int32))
        self.d_T, self.d_nbr = dev(self.T), dev(self.nbr)
        self._refs = {}

    def ref(self, sigma=1.0, signed=False, upstream=1.0, want_grad=True):
        key = (sigma, signed, upstream, want_grad)
        if key not in self._refs:
            scale = 1.0 / (self.t * self.k) if signed else 1.0 / self.t
            self._refs[key] = R.graph_loss(self.feats if signed else self.pos, self.labels, self.T, self.g, sigma, signed,
                                           upstream, scale, want_grad=want_grad)
        return self._refs[key]

    # ---- the entry points, one call each; every output buffer is the call's own ----
    def _call(self, name, *args):
        from geot_amd.ext._common import call
        call(name, self.d_T.device, *args)

    def fwd_plain(self, sigma=1.0):
        out = nan(self.t)
        self._call("geot_ntm_threed_loss", self.b, self.n, self.c, self.k, sigma, self.d_pos.data_ptr(), self.d_lab.data_ptr(),
                   self.d_T.data_ptr(), self.d_nbr.data_ptr(), out.data_ptr())
        return out

    def fwd_ord(self, sigma=1.0, order=None):
        out = nan(self.t)
        self._call("geot_ntm_threed_loss_ord", self.b, self.n, self.c, self.k, sigma, self.d_pos.data_ptr(),
                   self.d_lab.data_ptr(), self.d_T.data_ptr(), self.d_nbr.data_ptr(), _p(order), out.data_ptr())
        return out

    def graph_bytes(self):
        from geot_amd import _lib
        return int(_lib.load().geot_ntm_threed_graph_bytes(self.b, self.n, self.k))

    def fwd_graph(self, sigma=1.0, order=None):
        out = nan(self.t)
        gb = self.graph_bytes()
        graph = torch.full((gb,), 0xFF, dtype=torch.uint8, device=DEV)                   # all-ones words: NaNs and -1s
        self._call("geot_ntm_threed_loss_fwd_graph", self.b, self.n, self.c, self.k, sigma, self.d_pos.data_ptr(),
                   self.d_lab.data_ptr(), self.d_T.data_ptr(), self.d_nbr.data_ptr(), _p(order), out.data_ptr(),
                   graph.data_ptr(), gb)
        return out, graph

    def grad_graph(self, graph, order=None, upstream=None):
        g = nan(self.t, self.c * self.c)
        up = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device=DEV)
        self._call("geot_ntm_threed_loss_grad_graph", self.b, self.n, self.c, self.k, 1.0 / self.t, _p(up), self.d_T.data_ptr(),
                   self.d_nbr.data_ptr(), _p(order), graph.data_ptr(), graph.numel(), g.data_ptr())
        return g

    def ws_bytes(self):
        from geot_amd import _lib
        return int(_lib.load().geot_ntm_threed_loss_ws_bytes(self.b, self.n, self.k))

    def grad_ws(self, sigma=1.0, order=None, short=0, null_ws=False):
        g = torch.zeros(self.t, self.c * self.c, dtype=torch.float32, device=DEV)
        nb = self.ws_bytes()
        ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=DEV)
        self._call("geot_ntm_threed_loss_grad_ws", self.b, self.n, self.c, self.k, sigma, 1.0 / self.t, self.d_pos.data_ptr(),
                   self.d_lab.data_ptr(), self.d_T.data_ptr(), self.d_nbr.data_ptr(), _p(order), g.data_ptr(),
                   None if null_ws else ws.data_ptr(), nb - short)
        return g

    def grad_atomic(self, sigma=1.0):
        g = torch.zeros(self.t, self.c * self.c, dtype=torch.float32, device=DEV)
        self._call("geot_ntm_threed_loss_grad", self.b, self.n, self.c, self.k, sigma, 1.0 / self.t, self.d_pos.data_ptr(),
                   self.d_lab.data_ptr(), self.d_T.data_ptr(), self.d_nbr.data_ptr(), g.data_ptr())
        return g

    def feat_fwd(self, sigma=1.0):
        out = nan(self.t)
        self._call("geot_ntm_feature_loss", self.b, self.n, self.c, self.k, self.fd, sigma, self.d_feats.data_ptr(),
                   self.d_lab.data_ptr(), self.d_T.data_ptr(), self.d_nbr.data_ptr(), out.data_ptr())
        return out

    def feat_grad_atomic(self, sigma=1.0):
        g = torch.zeros(self.t, self.c * self.c, dtype=torch.float32, device=DEV)
        self._call("geot_ntm_feature_loss_grad", self.b, self.n, self.c, self.k, self.fd, sigma, 1.0 / (self.t * self.k),
                   self.d_feats.data_ptr(), self.d_lab.data_ptr(), self.d_T.data_ptr(), self.d_nbr.data_ptr(), g.data_ptr())
        return g

    def feat_grad_det(self, sigma=1.0, upstream=None):
        g = nan(self.t, self.c * self.c)
        acc = torch.zeros(self.t * self.c * self.c, dtype=torch.int64, device=DEV)
        up = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device=DEV)
        self._call("geot_ntm_feature_loss_grad_det", self.b, self.n, self.c, self.k, self.fd, sigma, 1.0 / (self.t * self.k),
                   self.d_feats.data_ptr(), self.d_lab.data_ptr(), self.d_T.data_ptr(), self.d_nbr.data_ptr(), acc.data_ptr(),
                   _p(up), g.data_ptr())
        return g

    # ---- families of calls against the reference ----
    def check_threed(self, family, tag, sigma=1.0, order=None, plain=True, grouped=True, atomic=True, want_grad=True):
        """Forward and the three backward forms of the 3-D loss; returns the grouped forward's values."""
        ref = self.ref(sigma, want_grad=want_grad)
        pp = None
        if plain and order is None:
            note(family, tag + " threed_loss", R.check_forward(host(self.fwd_plain(sigma)), ref, tag + " threed_loss"))
        if grouped or self.c != C:
            pp = self.fwd_ord(sigma, order)
            note(family, tag + " threed_loss_ord", R.check_forward(host(pp), ref, tag + " threed_loss_ord"))
        if grouped and self.c == C:
            pg, graph = self.fwd_graph(sigma, order)
            note(family, tag + " fwd_graph", R.check_forward(host(pg), ref, tag + " fwd_graph"))
            if want_grad:
                note(family, tag + " grad_graph", R.check_grad(host(self.grad_graph(graph, order)), ref, tag + " grad_graph"))
        if grouped and want_grad:
            note(family, tag + " grad_ws", R.check_grad(host(self.grad_ws(sigma, order)), ref, tag + " grad_ws"))
        if atomic and want_grad and order is None:
            note(family, tag + " threed_loss_grad", R.check_grad(host(self.grad_atomic(sigma)), ref, tag + " threed_loss_grad"))
        return pp

    def check_feature(self, family, tag, sigma=1.0, atomic=False):
        ref = self.ref(sigma, signed=True)
        note(family, tag + " feature_loss", R.check_forward(host(self.feat_fwd(sigma)), ref, tag + " feature_loss"))
        note(family, tag + " feature_loss_grad_det",
             R.check_grad(host(self.feat_grad_det(sigma)), ref, tag + " feature_loss_grad_det", fixed=1.0 / (self.t * self.k)))
        if atomic:
            note(family, tag + " feature_loss_grad",
                 R.check_grad(host(self.feat_grad_atomic(sigma)), ref, tag + " feature_loss_grad"))


def _p(t):
    return None if t is None else t.data_ptr()


def host(t):
    return t.detach().cpu().numpy()


def orders(case, rng):
    """Every kind of processing order: NULL, identity, reversed, a random permutation of all points, the Morton order."""
    from geot_amd.ntm import spatial_order
    t = case.t
    morton = spatial_order(case.d_pos.view(case.b, case.n, 3))
    assert morton is not None and np.array_equal(np.sort(host(morton)), np.arange(t))
    return {"null": None, "identity": dev(np.arange(t, dtype=np.int32)), "reversed": dev(np.arange(t, dtype=np.int32)[::-1]),
            "random": dev(rng.permutation(t).astype(np.int32)), "morton": morton}


# ---- walk tails ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [2, 3, 4, 6])
@pytest.mark.parametrize("shape", ["2", "17", "31", "32", "33", "3x11", "8*4G-1", "8*4G", "8*4G+1"])
def test_walk_tails_of_the_grouped_kernels(G, shape, monkeypatch):
    """The last group of an XCD chunk and of the whole walk: slots past total_pts, slots past the chunk, cloud boundaries
    inside a group.  GEOT_NTM_G selects the instantiation of threed_loss_ord and grad_ws; the graph pair is built for G = 4."""
    monkeypatch.setenv("GEOT_NTM_G", str(G))
    edge = {"8*4G-1": 32 * G - 1, "8*4G": 32 * G, "8*4G+1": 32 * G + 1}
    b, n = (3, 11) if shape == "3x11" else (1, edge[shape] if shape in edge else int(shape))
    rng = np.random.default_rng(100 * G + b * n)
    case = Case(rng, b, n, min(3, n - 1))
    pp = case.check_threed("walk tails, grouped", "G=%d t=%s" % (G, shape), plain=False, atomic=False)
    if G == 4:          # the same kernel with BUILD on or off: the same bits
        assert torch.equal(case.fwd_graph()[0], pp)


@pytest.mark.parametrize("t", [2, 31, 32, 33, 65])
def test_walk_tails_of_the_one_point_per_wave_kernels(t):
    rng = np.random.default_rng(t)
    case = Case(rng, 1, t, min(3, t - 1))
    case.check_threed("walk tails, one point per wave", "t=%d" % t, grouped=False)
    case.check_feature("walk tails, one point per wave", "t=%d" % t)


# ---- the persistent loop's second trip ----------------------------------------------------------------------------------------
def test_second_trip_of_the_plain_walk_two_classes():
    """65 569 points = 16 384 workgroups x 4 waves + 33: the t += gridDim.x >> 3 step, forward and atomic backward (C = 2)."""
    rng = np.random.default_rng(7)
    Case(rng, 1, 65569, 3, c=2).check_threed("second trip", "C=2 N=65569", grouped=False)


def test_second_trip_of_the_plain_walk_17_classes_forward():
    rng = np.random.default_rng(8)
    Case(rng, 1, 65569, 3).check_threed("second trip", "C=17 N=65569", grouped=False, atomic=False, want_grad=False)


def test_second_trip_of_the_grouped_walk(monkeypatch):
    """G = 2: 131 077 points = 16 384 workgroups x 4 waves x 2 points + 5, forward and the CSR gather backward."""
    monkeypatch.setenv("GEOT_NTM_G", "2")
    rng = np.random.default_rng(9)
    case = Case(rng, 1, 131077, 2)
    ref = case.ref()
    note("second trip", "G=2 N=131077 threed_loss_ord", R.check_forward(host(case.fwd_ord()), ref, "threed_loss_ord"))
    note("second trip", "G=2 N=131077 grad_ws", R.check_grad(host(case.grad_ws()), ref, "grad_ws"))


# ---- k ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 31, 32, 33, 63, 64])
def test_every_k_at_which_the_lane_masks_change(k):
    """seg_shift of the edge-parallel pre-pass changes after k = 1, 2, 32; lanes l >= k are masked; at k = 64 with one label
    all 64 lanes are live."""
    rng = np.random.default_rng(k)
    case = Case(rng, 2, 130, k, labels="equal" if k == 64 else "mixed")
    if k == 64:
        assert (case.ref()["w"] != 0).all()
    case.check_threed("k", "k=%d" % k)
    case.check_feature("k", "k=%d" % k, atomic=True)


# ---- in-degrees at the capacity edge ------------------------------------------------------------------------------------------
HUB = 123


@pytest.mark.parametrize("d", [0, 1, 63, 64, 65, 128, 129, 299])
def test_planted_in_degree(d):
    """One target listed by exactly d points (one label: every edge is live).  Graph mode: the 64 slots of the forward-built
    list, the first overflow entry at 65.  Gather mode: the lanes hold 64 in-edges, the tail loop takes the rest in trips of
    64 (128: one whole trip, 129: a trip of one)."""
    rng = np.random.default_rng(1000 + d)
    nbr = R.planted_in_degree(rng, 300, 8, HUB, d)
    case = Case(rng, 1, 300, 8, labels="equal", nbr=nbr)
    assert R.in_degrees(case.g)[HUB] == d and case.ref()["terms"][HUB] == 8 + d
    case.check_threed("in-degree", "d=%d" % d, plain=False)
    if d <= 64:
        assert R.in_degrees(case.g).max() <= 64
        _, g1 = case.fwd_graph()
        _, g2 = case.fwd_graph()            # the slots are handed out in arrival order; the sort makes the sum's order fixed
        assert torch.equal(case.grad_graph(g1), case.grad_graph(g2)) and torch.equal(case.grad_graph(g1), case.grad_graph(g1))
    a, b = case.feat_grad_det(), case.feat_grad_det()
    assert torch.equal(a, b)                # integer sums: the same bits always, hubs included


def test_special_edges():
    """A point with only dead out-edges that nobody lists (its gradient row must still be written: zeros), a mutual pair, a
    one-way edge, a self-edge, and a row that is an out-neighbour of one point of a group and an in-neighbour of another."""
    rng = np.random.default_rng(11)
    n, k = 300, 8
    nbr = R.random_out_lists(rng, 1, n, k, exclude=(10,))
    lab = R.labels_mixed(rng, n)
    lab[10] = 99                                           # no other point has it: all of point 10's out-edges are dead
    keep = (10, 20, 21, 30, 31, 40, 48, 49, 60)
    R.ensure_edge(nbr, 0, 20, 21)
    R.ensure_edge(nbr, 0, 21, 20)
    lab[21] = lab[20]
    R.ensure_edge(nbr, 0, 30, 31)
    R.remove_edge(nbr, rng, 0, 31, 30, avoid=keep)
    lab[31] = lab[30]
    nbr[0, 40, 0] = 40                                     # self-edge: weight 1 in S, no difference
    # identity order, G = 4: points 48..51 share a wave (the chunk of XCD 1 starts at 48 for t = 300)
    R.ensure_edge(nbr, 0, 48, 60)
    R.ensure_edge(nbr, 0, 60, 49, slot=1)
    R.remove_edge(nbr, rng, 0, 49, 60, avoid=keep)
    lab[48] = lab[49] = lab[60]
    case = Case(rng, 1, n, k, labels=lab, nbr=nbr)
    ref = case.ref()
    assert ref["terms"][10] == 0 and ref["per_point"][10] == 0 and not ref["cond"][10].any()
    assert 60 in nbr[0, 48] and 49 in nbr[0, 60] and 60 not in nbr[0, 49] and 30 not in nbr[0, 31]
    case.check_threed("in-degree", "special edges, NULL order")
    case.check_threed("in-degree", "special edges, identity order", order=dev(np.arange(n, dtype=np.int32)))
    case.check_feature("in-degree", "special edges", atomic=True)


# ---- labels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", ["equal", "different", "mixed"])
def test_label_patterns(labels):
    rng = np.random.default_rng(12)
    case = Case(rng, 2, 130, 7, labels=labels)
    case.check_threed("labels", labels)
    case.check_feature("labels", labels, atomic=True)
    if labels == "different":       # every weight 0: per_point 0, gradient 0 (both exact, by the zero bounds), S = 0.001
        ref = case.ref()
        assert not ref["per_point"].any() and not ref["cond"].any()
        _, graph = case.fwd_graph()
        S = graph[:4 * case.t].view(torch.float32)
        assert torch.equal(S, torch.full_like(S, 0.001))


# ---- sigma --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.35, 1.0, 2.0])
def test_sigma_in_every_entry_point(sigma):
    """1 / (2 sigma^2) and 1 / (2 sigma) agree at sigma = 1 only."""
    rng = np.random.default_rng(13)
    case = Case(rng, 2, 130, 7)
    case.check_threed("sigma", "sigma=%g" % sigma, sigma=sigma)
    case.check_feature("sigma", "sigma=%g" % sigma, sigma=sigma, atomic=True)
    generic = Case(rng, 1, 130, 5, c=12)            # the run-time-C launch of threed_loss_ord
    generic.check_threed("sigma", "C=12 sigma=%g" % sigma, sigma=sigma, grouped=False)


# ---- upstream -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hub_case():
    rng = np.random.default_rng(14)
    case = Case(rng, 1, 300, 8, labels="equal", nbr=R.planted_in_degree(rng, 300, 8, HUB, 129))
    assert R.in_degrees(case.g)[HUB] == 129
    return case


@pytest.mark.parametrize("upstream", [-2.5, 0.0])
@pytest.mark.parametrize("mode", ["graph", "gather", "atomic"])
def test_upstream_gradient_through_the_threed_function(hub_case, mode, upstream, monkeypatch):
    """graph: applied in the gather kernel and, for the 65 in-edges past the hub's 64 slots, in the overflow kernel; gather
    and atomic: applied by the autograd glue."""
    from geot_amd.ntm import _ThreeDLossFn
    monkeypatch.setenv("GEOT_NTM_GRAD", mode)
    c = hub_case
    T = c.d_T.clone().requires_grad_(True)
    loss = _ThreeDLossFn.apply(c.d_pos.view(1, c.n, 3), c.d_lab.view(1, c.n), T, c.d_nbr, 1.0, None)
    ref = c.ref(upstream=upstream)
    assert abs(loss.item() - ref["per_point"].mean()) <= (5 * c.k + 38 + 300) * R.U2 * ref["per_point"].mean()
    loss.backward(torch.tensor(upstream, device=DEV))
    note("upstream", "%s %g" % (mode, upstream), R.check_grad(host(T.grad), ref, "threeD %s upstream %g" % (mode, upstream)))
    if upstream == 0.0:
        assert not T.grad.any()


@pytest.mark.parametrize("upstream", [-2.5, 0.0])
def test_upstream_gradient_through_the_feature_function(hub_case, upstream):
    from geot_amd.ntm import _FeatureLossFn
    c = hub_case
    T = c.d_T.clone().requires_grad_(True)
    loss = _FeatureLossFn.apply(c.d_feats.view(1, c.n, c.fd), c.d_lab.view(1, c.n), T, c.d_nbr, 1.0)
    loss.backward(torch.tensor(upstream, device=DEV))
    ref = c.ref(signed=True, upstream=upstream)
    note("upstream", "feature %g" % upstream, R.check_grad(host(T.grad), ref, "feature upstream %g" % upstream,
                                                             fixed=abs(upstream) / (c.t * c.k)))
    # and the entry point itself with the device scalar
    note("upstream", "feature_loss_grad_det %g" % upstream,
         R.check_grad(host(c.feat_grad_det(upstream=upstream)), ref, "grad_det", fixed=abs(upstream) / (c.t * c.k)))


def test_upstream_in_the_graph_entry_point(hub_case):
    c = hub_case
    _, graph = c.fwd_graph()
    note("upstream", "grad_graph -2.5", R.check_grad(host(c.grad_graph(graph, upstream=-2.5)), c.ref(upstream=-2.5), "grad_graph"))


# ---- order --------------------------------------------------------------------------------------------------------------------
def test_every_processing_order(monkeypatch):
    """Any mapping of walk position to point is correct; it moves only which points share a wave."""
    from geot_amd.ntm import spatial_order
    rng = np.random.default_rng(15)
    case = Case(rng, 3, 77, 6)
    with monkeypatch.context() as m:
        m.setenv("GEOT_NTM_ORDER", "off")
        assert spatial_order(case.d_pos.view(3, 77, 3)) is None
    for name, od in orders(case, rng).items():
        pp = case.check_threed("order", name, order=od, plain=False, atomic=False)
        assert torch.equal(case.fwd_graph(order=od)[0], pp)       # BUILD on / off: the same bits for the same order
    # the one-point-per-wave kernel (reached with an order at class counts other than 17): the same bits for every order
    generic = Case(rng, 3, 77, 6, c=12)
    got = {name: generic.fwd_ord(order=od) for name, od in orders(generic, rng).items()}
    note("order", "C=12 threed_loss_ord", R.check_forward(host(got["null"]), generic.ref(), "C=12 threed_loss_ord"))
    for name, pp in got.items():
        assert torch.equal(pp, got["null"]), name
    assert torch.equal(generic.fwd_plain(), got["null"])


# ---- CSR scan -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [4095, 4096, 4097])
def test_csr_offsets_across_the_scan_chunk(t):
    """t + 1 offsets: one scan block, exactly one, and a second block of one and two entries."""
    rng = np.random.default_rng(t)
    case = Case(rng, 1, t, 2)
    note("CSR scan", "t=%d grad_ws" % t, R.check_grad(host(case.grad_ws()), case.ref(), "grad_ws t=%d" % t))


# ---- register buckets ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [11, 12, 17, 18, 22, 23])
def test_register_bucket_edges(c):
    """ceil(C^2 / 64) registers per lane, instantiated for 2, 5, 8 and 16: the edges fall at C = 11|12, 17|18 and 22|23."""
    rng = np.random.default_rng(c)
    case = Case(rng, 1, 130, 5, c=c, feat_dim=c)
    case.check_threed("R buckets", "C=%d" % c, grouped=False)
    case.check_feature("R buckets", "C=%d" % c)


# ---- fall-backs and argument checks -------------------------------------------------------------------------------------------
def test_grad_ws_without_enough_workspace_takes_the_atomic_form():
    rng = np.random.default_rng(16)
    case = Case(rng, 2, 130, 7)
    ref = case.ref()
    note("fallbacks", "ws one byte short", R.check_grad(host(case.grad_ws(short=1)), ref, "grad_ws, one byte short"))
    note("fallbacks", "NULL workspace", R.check_grad(host(case.grad_ws(null_ws=True)), ref, "grad_ws, NULL workspace"))


def test_bad_arguments_are_refused_before_any_launch():
    from geot_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(17)
    case = Case(rng, 1, 40, 3)
    b, n, c, k = 1, 40, C, 3
    P, F, L, Tm, N = (x.data_ptr() for x in (case.d_pos, case.d_feats, case.d_lab, case.d_T, case.d_nbr))
    out, g = nan(n), nan(n, c * c)
    gb, wb = case.graph_bytes(), case.ws_bytes()
    graph = torch.zeros(gb, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(wb, dtype=torch.uint8, device=DEV)
    acc = torch.zeros(n * c * c, dtype=torch.int64, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    for kk, sg, cc in ((0, 1.0, c), (65, 1.0, c), (k, 0.0, c), (k, -1.0, c), (k, 1.0, 33)):
        assert lib.geot_ntm_threed_loss(b, n, cc, kk, sg, P, L, Tm, N, out.data_ptr(), s) == INVALID
        assert lib.geot_ntm_threed_loss_ord(b, n, cc, kk, sg, P, L, Tm, N, None, out.data_ptr(), s) == INVALID
        assert lib.geot_ntm_threed_loss_fwd_graph(b, n, cc, kk, sg, P, L, Tm, N, None, out.data_ptr(), graph.data_ptr(), gb, s) == INVALID
        assert lib.geot_ntm_threed_loss_grad(b, n, cc, kk, sg, 1.0, P, L, Tm, N, g.data_ptr(), s) == INVALID
        assert lib.geot_ntm_threed_loss_grad_ws(b, n, cc, kk, sg, 1.0, P, L, Tm, N, None, g.data_ptr(), ws.data_ptr(), wb, s) == INVALID
        assert lib.geot_ntm_feature_loss(b, n, cc, kk, case.fd, sg, F, L, Tm, N, out.data_ptr(), s) == INVALID
        assert lib.geot_ntm_feature_loss_grad(b, n, cc, kk, case.fd, sg, 1.0, F, L, Tm, N, g.data_ptr(), s) == INVALID
        assert lib.geot_ntm_feature_loss_grad_det(b, n, cc, kk, case.fd, sg, 1.0, F, L, Tm, N, acc.data_ptr(), None, g.data_ptr(), s) == INVALID
        if sg > 0:      # (the graph backward takes no sigma)
            assert lib.geot_ntm_threed_loss_grad_graph(b, n, cc, kk, 1.0, None, Tm, N, None, graph.data_ptr(), gb, g.data_ptr(), s) == INVALID
    assert lib.geot_ntm_threed_loss_fwd_graph(b, n, c, k, 1.0, P, L, Tm, N, None, out.data_ptr(), graph.data_ptr(), gb - 1, s) == INVALID
    assert lib.geot_ntm_threed_loss_grad_graph(b, n, c, k, 1.0, None, Tm, N, None, graph.data_ptr(), gb - 1, g.data_ptr(), s) == INVALID
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(g).all() and not acc.any() and not graph.any()      # nothing was launched


# ---- the host-side checks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [40, -1])
def test_debug_flag_checks_the_callers_neighbour_ids(bad, monkeypatch):
    """GEOT_DEBUG=1: an id equal to n or -1 raises IndexError on the host, before any launch."""
    from geot_amd.ntm import feature_space_loss, threeD_space_loss
    monkeypatch.setenv("GEOT_DEBUG", "1")
    rng = np.random.default_rng(18)
    case = Case(rng, 1, 40, 3)
    nbr = case.nbr.copy()
    nbr[0, 17, 1] = bad
    lab = case.d_lab.view(1, 40).long()
    with pytest.raises(IndexError, match="threeD_space_loss nbr"):
        threeD_space_loss(k=3)(case.d_pos.view(1, 40, 3), lab, case.d_T, nbr=dev(nbr))
    logits = case.d_feats.view(1, 40, case.fd).permute(0, 2, 1).contiguous()
    with pytest.raises(IndexError, match="feature_space_loss nbr"):
        feature_space_loss(k=3)(logits, lab, case.d_T, nbr=dev(nbr))
    threeD_space_loss(k=3)(case.d_pos.view(1, 40, 3), lab, case.d_T, nbr=case.d_nbr)        # a good list passes the check


def test_more_neighbours_than_other_points_is_refused():
    """k + 1 > N: the reference's topk raises; here the kNN would pad the lists with id 0 (repeated ids)."""
    from geot_amd.ntm import feature_space_loss, threeD_space_loss
    pos = torch.rand(2, 7, 3, device=DEV)
    with pytest.raises(RuntimeError, match="k = 7 neighbours need more than 7 points"):
        threeD_space_loss(k=7).neighbours(pos)
    assert threeD_space_loss(k=6).neighbours(pos).shape == (2, 7, 6)
    logits = torch.rand(2, C, 7, device=DEV)
    with pytest.raises(RuntimeError, match="k = 7 neighbours need more than 7 points"):
        feature_space_loss(k=7)(logits, torch.zeros(2, 7, dtype=torch.long, device=DEV), torch.rand(14, C, C, device=DEV))
