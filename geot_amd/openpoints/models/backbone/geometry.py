"""The look-ahead geometry: everything PointTransformer_seg_T.forward derives from the COORDINATES of a batch alone -- Group,
the 8192-sample FPS, the index plan of the decoder -- as one typed object (PointTransformer_seg_T.prefetch_geometry makes it,
forward(geometry=) takes it), with the one answer to "does this geometry describe these tensors".  This module alone knows
the layout; the models, the training steps and graph_step.py go through its records and methods."""
from collections import namedtuple

# three_nn + inverse-distance weights of one FP module; point-major layout: + the Morton sequence of the unknown points
# (fused_norm.local_spatial_order) and, in training, the ReverseIndex of (idx, weight) for the gradient
FpEntry = namedtuple("FpEntry", "idx weight order rix", defaults=(None, None))
# the kNN ids (B, Nq, k) of one EdgeConv layer and, in training, the reverse index its fused gradient walks
EdgeEntry = namedtuple("EdgeEntry", "idx rix", defaults=(None,))
# the sampled clouds, the three FP entries and the two EdgeConv stages' pairs of graphs (queries among the sources, queries
# among themselves); an entry that is None is computed in line by its module
IndexPlan = namedtuple("IndexPlan", "center_pts center_pts_trans center_trans fp2 fp1 fp0 dg2 dg1", defaults=(None,) * 6)


def _cut(t, lo, hi):
    return None if t is None else t[lo:hi]


class Geometry:
    """pts: the (B, N, 3) tensor the work was done on; group: Group's (neighborhood, center, idx); plan: the IndexPlan;
    training / fp_layout: the mode of the model that made it (the plan's contents depend on both); static: on the current
    stream, in memory, for a caller that vouches for it (graph_step.py refills its buffers itself: a replay has no tensor
    identities to check); grouped / ready: side-stream events behind Group / behind everything (a queued geometry);
    sources: the caller's tensors `pts` was assembled from, with their version counters (default: pts itself)."""

    def __init__(self, pts, group, plan, training, fp_layout, static=False, grouped=None, ready=None, sources=None, version=None):
        self.pts, self.group, self.plan = pts, group, plan
        self.training, self.fp_layout, self.static = training, fp_layout, static
        self.grouped, self.ready = grouped, ready
        self.version = None if static else (pts._version if version is None else version)
        self.sources = None if static else ((pts, self.version),) if sources is None else tuple((t, t._version) for t in sources)

    def tree_fields(self):
        """(attributes that hold buffers, attributes that hold identities) for graph_step.py: it clones / refills the tensors
        inside the former and never copies the latter (tensor identities, events); every other attribute is a python scalar
        that must agree between two geometries of one captured graph."""
        return ("group", "plan"), ("pts", "version", "sources", "grouped", "ready")

    def describes(self, tensors):
        """Was this geometry computed from exactly these tensors -- the same objects, not edited since (a batch of the same
        SHAPE is not the same batch)?  `tensors`: the caller's sources in order, or [pts].  A static geometry is vouched for;
        one whose identities were dropped (graph_step.tree_clone) describes nothing."""
        def same(src):
            return src is not None and len(src) == len(tensors) and all(t is s and t._version == v for t, (s, v) in zip(tensors, src))
        return self.static or same(self.sources) or same(((self.pts, self.version),))

    def usable(self, pts, training, fp_layout, can_wait):
        """By a model in this mode, for this tensor?  can_wait: the model has a side stream to wait for (a queued geometry's
        work is still in flight there; a static one is memory)."""
        return (self.training == training and self.fp_layout == fp_layout and (self.static or can_wait)
                and self.describes([pts]))

    def positions(self, pts):
        """The tensor to hand the model together with this geometry: the one the work was done on, which usable() recognises
        (a static geometry is keyed to no tensor: pts itself)."""
        return pts if self.static else self.pts

    def slice(self, lo, hi, sources=None):
        """The geometry of clouds [lo, hi) of the batch, for a model in EVAL mode: every entry is per cloud -- sample ids,
        neighbour ids and Morton orders are cloud-local -- so the slices are exactly what prefetch_geometry(pts[lo:hi]) of an
        eval-mode model would compute; the training-only entries (the reverse indices of the gradients) are dropped.
        FixMatch's frozen teacher sees the weak view, which is also the last third of the student's batch: its geometry -- an
        8192-sample FPS, Group, the index plan -- need not be computed twice.  sources: the caller's tensors the slice
        stands for (default: the slice of pts)."""
        b, n = self.pts.shape[0], self.pts.shape[1]
        neighborhood, center, idx = self.group
        flat = None if idx is None else (idx.view(b, -1)[lo:hi] - lo * n).reshape(-1)
        p = self.plan

        def fp(e):
            return FpEntry(_cut(e.idx, lo, hi), _cut(e.weight, lo, hi), _cut(e.order, lo, hi))

        def graphs(pair):
            return tuple(EdgeEntry(_cut(e.idx, lo, hi)) for e in pair)
        plan = IndexPlan([_cut(t, lo, hi) for t in p.center_pts], [_cut(t, lo, hi) for t in p.center_pts_trans],
                         _cut(p.center_trans, lo, hi), fp(p.fp2), fp(p.fp1), fp(p.fp0), graphs(p.dg2), graphs(p.dg1))
        return Geometry(self.pts[lo:hi], (neighborhood[lo:hi], center[lo:hi], flat), plan, False, self.fp_layout, self.static,
                        self.grouped, self.ready, sources, self.version)
