"""Validation batches for test-time voting, built on the GPU from scans that already live there: val_batch's batch with the
configured `vote` transform list (cfgs/tooth_semi/*.yaml datatransforms.vote: [PointCloudScaling]) applied on top of the `val`
list [PointsToTensor, PointCloudCenterAndNormalize].  The reference carries both config keys and uses neither
(train.py:716 validate(model, val_loader, cfg, num_votes=0, data_transform=None)); what they mean here:

    pos (B, m, 3)  x (B, 3, m)     the VOTED view, `val` list then `vote` list: what the model sees
    pos_search (B, m, 3)           the `val` view's pos: what get_pred_whole de-normalises with center / scale -- the sampled
                                   points in the scan's coordinates, where the whole scan's neighbour search has to run
    every other key as ValBatcher's

Per slot two ViewProgram jobs read the same sampled row -- the `val` list, and the `val` list followed by the `vote` list --
in ONE geot_view_program launch; a batch costs what a ValBatcher batch costs.  view_program.py's aliasing rule applies
unchanged: x separates from pos at the normalisation, so an in-place vote transform (PointCloudScaling) does not reach it, and
x is the un-voted batch's x.  Each call samples the scans afresh, so V calls on the same scans are V votes
(validation.vote_scans, validate_scans_voted).

Host draws by default: per item np.random.choice, then the vote list's draws (ViewProgram.draw), in the reference's per-item
order.  draws=DeviceDraws(seed) draws the samples on the device, DeviceDraws(seed, views=True) the vote parameters too: a slot's
two jobs draw under the slot's own draw id (views 0 and 1), as FixMatchBatcher's weak / strong pair does.
"""
from ...ext._common import need
from .fixmatch_batch import TOOTH_VIEW_KWARGS
from .sample_draw import ViewDrawHandle
from .val_batch import ScanBatcher
from .view_program import ViewProgram

VAL_LIST = ["PointsToTensor", "PointCloudCenterAndNormalize"]       # the yaml's datatransforms.val
DEFAULT_VOTE = ("PointCloudScaling",)                               # the yaml's datatransforms.vote


class VoteBatcher(ScanBatcher):
    """`batch(idx)` returns the dict of the module text for the scans `idx` of the set, in freshly allocated tensors.  An
    empty `vote` list is allowed: pos_search then equals pos.  A list ViewProgram refuses (RandomDropout, ...) raises its
    NotImplementedError here, before any device call.

    stream / draws: as ValBatcher's; with DeviceDraws(seed, views=True) the vote list's parameters are device draws too, and
    an explicit params= still wins.  Call `join(batch)` before the current stream reads a batch built on a side stream.
    curvatures=True adds "curvatures" (B, m) float32 to every batch, the covering ones too (Batcher's class text)."""

    join_keys = ScanBatcher.join_keys + ("pos_search",)

    def __init__(self, scans, num_points, num_classes=17, vote=DEFAULT_VOTE, kwargs=TOOTH_VIEW_KWARGS, stream=None, draws=None,
                 curvatures=False):
        need(not isinstance(vote, str), "VoteBatcher: vote is a list of transform class names")
        self.vote = list(vote)
        self.val_program = ViewProgram(VAL_LIST, kwargs)
        self.program = ViewProgram(VAL_LIST + self.vote, kwargs)       # NotImplementedError for what the kernel cannot do
        super().__init__(scans, num_points, num_classes, kwargs, stream, draws, curvatures)

    def batch(self, idx, sel=None, params=None, check=False, draws=None, affine=False):
        """idx: scan numbers within the set; sel (B, m) vertex indices per scan and params (per scan one ViewProgram.draw
        result of the `val` + `vote` list, VoteBatcher.program) default to the reference's draws; draws: a DeviceDraws for
        this call (default: the constructor's).  check=True reads the bad-index flags back (one host sync) and raises
        IndexError.  affine=True adds view_center (B, 3) / view_scale (B,) of the `val` views -- the affine behind pos_search,
        not behind the voted pos; the default key set is unchanged."""
        ids = self._ids(idx)
        sel, params, ids_dev = self._draw(ids, (("sel", sel, len(ids)),), params, draws, lambda slot: self.program.draw(self.m))
        if not isinstance(params, ViewDrawHandle):          # per job: the `val` views (nothing is drawn), then the voted ones
            params = [self.val_program.draw(self.m)] * len(ids) + params
        return self._batch(ids, (len(ids),), sel, params, ids_dev, check, affine)

    def _cover_params(self, ids, draws, base):
        """The view parameters of one covering pass (ScanBatcher.cover): the vote list applied per pass, as batch() does."""
        if draws.views:     # drawn where they are used, under the slots' ids
            return ViewDrawHandle(draws.seed, base, len(ids))
        return [self.val_program.draw(self.m)] * len(ids) + [self.program.draw(self.m) for _ in ids]

    def _jobs(self, b):
        """Output rows [0, b) the `val` views, [b, 2 b) the voted ones; a slot's two jobs draw under the slot's id."""
        jobs = [(i, i, self.val_program) for i in range(b)] + [(i, b + i, self.program) for i in range(b)]
        return jobs, b, 2 * b, [0] * b + [1] * b, 2 * list(range(b))

    def _result(self, s, v, cls, ids, b):
        return {"pos": v["pos"][b:], "x": v["x"][b:], "pos_search": v["pos"][:b], **self._scan_keys(s, cls, ids)}
