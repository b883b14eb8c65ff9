"""Supervised training batches built on the GPU from scans that already live there -- what the reference's labelled training
loader does per item on CPU workers in the supervised stage (openpoints/dataset/tooth_semi/tooth_dataset.py:116-206 for
split 'train', the `train` transform list of cfgs/tooth_semi/default.yaml, default collation) plus the `.cuda()` /
`transpose` lines of examples/segmentation/train.py:442-445:

    pos (B, m, 3)   x (B, 3, m)   heights (B, m, 1)   y (B, m) int64   cls (B, 1) int64   class_weights (B, C)

A batch is geot_cloud_sample_batch (5 launches), ONE geot_view_program launch for whatever the transform list holds, one
gather of the jaw flags and three small pinned host-to-device copies; it never synchronises with the host.  The list is
given by the reference's class names and kwargs (view_program.ViewProgram); per item the host draws np.random.choice and
then the list's draws, in the reference's order.  With `draws=DeviceDraws(seed)` the np.random.choice of every item is one
geot_sample_draw launch in front of the five instead (sample_draw.py; not numpy's stream); the list's draws stay on the host
unless it is a DeviceDraws(seed, views=True): then ONE geot_view_draw launch (view_draw.py) draws every scale, jitter noise
row and drop of the batch on the device, from the slots' own draw ids, and nothing but the scan ids is copied from the host.

Kept from the reference: data['x'] IS data['pos'] until a transform rebinds pos.  With the default list x is the SCALED,
un-centred, un-jittered cloud (PointCloudCenterAndNormalize separates the two), and ChromaticDropGPU -- there are no colour
channels, x[:, :3] is all of x -- zeroes it with probability color_drop.
"""
from ...ext._common import need
from .batcher import Batcher
from .view_program import ViewProgram

# cfgs/tooth_semi/default.yaml datatransforms: the `train` list and its kwargs (`angle` is read by nothing in this list)
DEFAULT_TRAIN = ["PointsToTensor", "PointCloudScaling", "PointCloudCenterAndNormalize", "PointCloudJitter", "ChromaticDropGPU"]
DEFAULT_TRAIN_KWARGS = {"jitter_sigma": 0.001, "jitter_clip": 0.005, "scale": [0.8, 1.2], "gravity_dim": 1, "angle": [0, 1.0, 0]}


class SupervisedBatcher(Batcher):
    """Replaces the reference's labelled training DataLoader of the supervised stage: `batch(idx)` returns the dict of the
    module text for the scans `idx` of the set (what the sampler would yield) in freshly allocated tensors, so the `pos`
    handed to SupervisedStep(..., next_pos=) passes the model's identity and version check one call later.  `heights` is
    missing when the list has no PointCloudCenterAndNormalize, as in the reference.

    stream: queue every batch on that side stream.  A batch depends on the scans alone, so it does not wait for what the
    current stream has queued; call `join(data)` before the current stream (or a step) reads the tensors.

    draws: None keeps the reference's np.random.choice per item on the host; a sample_draw.DeviceDraws draws the vertex
    samples of a batch in one geot_sample_draw launch on the batcher's stream (one draw id per slot) and np.random.choice
    is not called.  Given here it serves every batch, given to batch() / draw() that call; an explicit sel= still wins.
    With DeviceDraws(seed, views=True) the list's parameters are device draws too: no host generator is read, draw()
    returns a ViewDrawHandle in place of the parameters, and batch(params=handle) replays it; an explicit params= wins.

    curvatures=True adds "curvatures" (B, m) float32 (Batcher's class text)."""

    def __init__(self, scans, num_points, num_classes=17, transforms=DEFAULT_TRAIN, kwargs=DEFAULT_TRAIN_KWARGS, stream=None,
                 draws=None, curvatures=False):
        self.program = ViewProgram(transforms, kwargs)          # NotImplementedError for what the kernel cannot do
        super().__init__(scans, num_points, num_classes, stream, draws, curvatures)

    def __len__(self):
        return len(self.scans)

    def draw(self, idx, sel=None, params=None, draws=None):
        """The host half of batch(): (sel (B, m) int64, params) with everything not given drawn in the reference's per-item
        order -- np.random.choice (tooth_dataset.py:134-135), then the list's draws (ViewProgram.draw).  With draws (a
        DeviceDraws; default: the constructor's) and no sel, geot_sample_draw draws the rows on the batcher's stream and sel
        is that (B, m) int64 DEVICE tensor."""
        return self._draw_slots(idx, sel, params, draws)[:2]

    def _draw_slots(self, idx, sel, params, draws):
        """draw() and, third, the scan ids on the device when the device drew (None otherwise)."""
        idx = [int(i) for i in idx]
        return self._draw(idx, (("sel", sel, len(idx)),), params, draws, lambda slot: self.program.draw(self.m))

    def batch(self, idx, sel=None, params=None, check=False, draws=None):
        """idx: scan numbers within the set; sel (B, m) vertex indices per scan and params (one ViewProgram.draw result per
        scan) default to the reference's draws; draws: a DeviceDraws for this call (default: the constructor's).
        check=True reads the bad-index flags back (one host sync) and raises IndexError."""
        idx = [int(i) for i in idx]
        need(len(idx) >= 1, "SupervisedBatcher.batch: at least one scan")
        need(all(0 <= i < len(self.scans) for i in idx), "SupervisedBatcher.batch: idx must lie in [0, %d)" % len(self.scans))
        sel, params, ids_dev = self._draw_slots(idx, sel, params, draws)
        return self._batch(idx, (len(idx),), sel, params, ids_dev, check)

    def _jobs(self, b):
        return [(i, i, self.program) for i in range(b)], b, b, None, None

    def _result(self, s, v, cls, ids, b):
        data = {"pos": v["pos"], "x": v["x"], "y": s["y"], "cls": cls, "class_weights": s["class_weights"]}
        if v["heights"] is not None:
            data["heights"] = v["heights"]
        return data

    def join(self, data):
        """Hand a batch built on the side stream to the CURRENT stream (Batcher._join)."""
        self._join(data.values())
